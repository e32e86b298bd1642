"""No GPU: the model of moments_stack against a plain loop, the device='cpu' path against the model on every case of the GPU tests, the
restated plan against the constants of vt_internal.h, utils.patch_moments and utils.normalized_scores (the formula in longdouble, the
zero rule), find_shifts(normalized=True) recovering shifts that the raw scores miss, the refusals Python makes itself, and the symbol."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import correlate_stack_model as csm
import moments_stack_model as msm
import moments_stack_cases as msc


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [(1, 1), (2, 3), (5, 1), (1, 7)])
@pytest.mark.parametrize('max_shift', [(0, 0), (1, 2), (4, 6)])
def test_model_is_the_plain_loop(max_shift, grid):
    img = np.random.default_rng(3).standard_normal((5, 7)).astype(np.float32)
    vals, bounds = msm.model(img[None], max_shift, grid)
    want = msm.naive(img, max_shift, grid)
    assert vals.shape == (1,) + want.shape
    assert (np.abs(vals[0] - want) <= bounds[0]).all() and np.abs(vals[0] - want).max() < 1e-13


def test_model_is_correlation_with_ones_and_nan_sets():
    """[..., 0] is correlate_stack's model against a reference of ones, [..., 1] the same on the squared stack (integers: exactly); a
    NaN pixel reaches exactly the (patch, shift) pairs whose window covers it."""
    s = msc.stack('small', True).copy()
    ones = np.ones(s.shape[1:], np.float32)
    vals, _ = msm.model(s, (2, 7), (3, 5))
    assert np.array_equal(vals[..., 0], csm.model(s, ones, (2, 7), (3, 5))[0])
    assert np.array_equal(vals[..., 1], csm.model(s * s, ones, (2, 7), (3, 5))[0])
    s[1, 6, 35] = np.nan
    bad = np.isnan(msm.model(s, (2, 7), (3, 5))[0])
    assert not bad[[0, 2, 3, 4]].any()
    hit = msm.covered(19, 37, (2, 7), (3, 5), 6, 35)
    assert 0 < hit.sum() < hit.size and np.array_equal(bad[1, ..., 0], hit) and np.array_equal(bad[1, ..., 1], hit)


def test_plan_names_its_edges_and_matches_the_source():
    """The constants the plan is restated with are vt_internal.h's, and the plan function's own arithmetic is the source's."""
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'voltools_amd', 'csrc')
    with open(os.path.join(root, 'vt_internal.h')) as f:
        text = f.read()
    const = {k: int(v) for k, v in re.findall(r'constexpr int (kMom\w+) = (\d+);', text)}
    assert const == dict(kMomChunk=msm.CHUNK, kMomGroup=msm.GROUP, kMomMaxRuns=msm.MAX_RUNS)
    with open(os.path.join(root, 'vt_kernels_momentsstack.hip')) as f:
        src = f.read()
    assert 'm.rows_wave = 64 / m.runs;' in src and f'm.rows_wg = {msm.WAVES} * m.rows_wave;' in src
    assert 'm.pitch = kMomChunk + m.runs * m.cv;' in src and 'm.lds_bytes = m.rows_wg * m.pitch * 4;' in src
    assert '__launch_bounds__(256) void moments_rows_kernel' in src and msm.WAVES * 64 == 256
    assert msm.max_lds_bytes() == 44032 <= 64 * 1024
    edges = msm.plan_edges(97, 150, 60)
    p = lambda rw: msm.plan(97, 150, (0, rw), (1, 1))
    assert {p(rw)['runs'] for rw in range(61)} == set(range(1, 8))
    assert {p(rw)['row_blocks'] for rw in range(61)} == {1, 2, 3} and {p(rw)['blocks_v'] for rw in range(61)} == {1, 2}
    names = {c['name'] for c in msc.CASES}
    for rw in edges:
        assert p(rw) != p(rw + 1) and {f'pieces-edge-{rw}', f'pieces-edge-{rw + 1}'} <= names
    for q in (msm.plan(512, 512, (8, 8), (1, 1)), msm.plan(1024, 1024, (16, 16), (8, 8)), msm.plan(19, 37, (18, 36), (19, 37))):
        assert q['runs'] * (q['rows_wg'] // 4) <= 64 and q['cv'] in (9, 11) and q['lds_bytes'] <= 44032
    one = msm.plan(97, 150, (3, 3), (1, 1))['unit_part_bytes']
    assert one == 97 * 7 * 2 * 8 and msm.launches(97, 150, (3, 3), (1, 1), 5, cap=2 * one) == (2, 1)
    assert msm.launches(97, 150, (3, 3), (1, 1), 5, cap=one - 8) == (1, 1) and msm.launches(97, 150, (3, 3), (1, 1), 5) == (5, 5)


# ---- the CPU path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', msc.CASES, ids=[c['name'] for c in msc.CASES])
def test_cpu_path_matches_the_model(c):
    for integers in (False, True):
        s, kw = msc.arguments(c, integers)
        got = vt.StaticVolume(s, device='cpu').moments_stack(c['max_shift'], c['grid'], **kw)
        vals, bounds = msm.model(s, c['max_shift'], c['grid'], kw['planes'])
        if integers:
            assert np.array_equal(got, vals), c['name']          # every partial sum is an integer below 2^53
        else:
            msm.check(got, vals, bounds, c['name'])


def test_cpu_path_fills_output():
    s = msc.stack('small', True)
    vals, _ = msm.model(s, (2, 3), (3, 5))
    sv = vt.StaticVolume(s, device='cpu')
    out = np.full(vals.shape, 7.0)
    assert sv.moments_stack((2, 3), (3, 5), output=out) is out and np.array_equal(out, vals)


# ---- utils ----------------------------------------------------------------------------------------------------------------------------
def test_patch_moments():
    s = msc.stack('small', True)
    for grid in ((1, 1), (3, 5), (19, 37)):
        got = vt.utils.patch_moments(s, grid)
        assert got.shape == (5,) + grid + (2,) and got.dtype == np.float64
        assert np.array_equal(got, msm.model(s, (0, 0), grid)[0][:, :, :, 0, 0, :])
    assert np.array_equal(vt.utils.patch_moments(s[2], (3, 5)), vt.utils.patch_moments(s, (3, 5))[2:3])
    f = msc.stack('small')
    vals, bounds = msm.model(f, (0, 0), (2, 3))
    assert (np.abs(vt.utils.patch_moments(f, (2, 3)) - vals[:, :, :, 0, 0, :]) <= bounds[:, :, :, 0, 0, :]).all()
    for bad in (dict(images=np.zeros((2, 2, 3, 3)), patch_grid=(1, 1)), dict(images=s, patch_grid=(0, 1)), dict(images=s, patch_grid=(1, 38)),
                dict(images=s, patch_grid=3), dict(images=np.zeros((0, 3, 3)), patch_grid=(1, 1))):
        with pytest.raises(ValueError):
            vt.utils.patch_moments(**bad)


def test_normalized_scores_against_longdouble():
    """The CPU path's coefficients against the same formula evaluated in longdouble on longdouble sums, on the 18 image pairs of the
    shift-recovery test (all nine patches, all 121 shifts).  Each of the five float64 sums carries a relative error of at most
    N 2^-53 of its magnitude sum, the centring divides by D = sum of squares - (sum)^2 / N, which amplifies by kappa = max(sum r^2 / D_r,
    sum s^2 / D_s), and a coefficient is at most 1: the derived tolerance is 16 N 2^-53 kappa per coefficient.
    Measured here: max |error| 2.8e-14, at most 0.0004 of its tolerance (tolerances between 3.9e-12 and 1.1e-10)."""
    worst = worst_ratio = 0.0
    tols = []
    for seed in msc.SEEDS:
        for d in msc.SHIFTS:
            ref, img = msc.bright_series(seed, d)
            got = vt.StaticVolume(img[None], device='cpu').correlate_stack_normalized(ref, msc.WINDOW, msc.GRID)
            c, _ = csm.correlate_image(img, ref, msc.WINDOW, msc.GRID)
            m, _ = msm.moments_image(img, msc.WINDOW, msc.GRID)
            r, _ = msm.moments_image(ref, (0, 0), msc.GRID)
            pixels = np.outer(np.diff(csm.patch_edges(60, 3)), np.diff(csm.patch_edges(72, 3)))[None, :, :, None, None]
            want, kappa = msm.coefficient(c[None], m[None], r[None, :, :, 0, 0, :], pixels)
            tol = (16 * pixels * 2.0 ** -53 * kappa).astype(np.float64)
            err = np.abs(got - want.astype(np.float64))
            assert got.shape == (1, 3, 3, 11, 11) and np.isfinite(want).all() and (np.abs(got) <= 1 + tol).all()
            worst, worst_ratio = max(worst, float(err.max())), max(worst_ratio, float((err / tol).max()))
            tols += [float(tol.min()), float(tol.max())]
            assert (err <= tol).all(), (seed, d, float((err / tol).max()))
    print(f'max |ncc - longdouble| {worst:.3e}, worst error / tolerance {worst_ratio:.4f}, tolerances {min(tols):.2e} .. {max(tols):.2e}')


def test_normalized_scores_zero_rule_and_arguments():
    rng = np.random.default_rng(8)
    img = rng.standard_normal((1, 12, 15)).astype(np.float32)
    img[0, 4:8, 5:10] = 3.0                                                              # patch (1, 1) of the 3 x 3 grid: constant
    ref = rng.standard_normal((12, 15)).astype(np.float32)
    sv = vt.StaticVolume(img, device='cpu')
    scores, moments = sv.correlate_stack(ref, (1, 1), (3, 3)), sv.moments_stack((1, 1), (3, 3))
    rm = vt.utils.patch_moments(ref, (3, 3))
    ncc = vt.utils.normalized_scores(scores, moments, rm, image_shape=(12, 15))
    assert ncc.shape == scores.shape and ncc.dtype == np.float64 and np.isfinite(ncc).all() and (np.abs(ncc) <= 1 + 1e-12).all()
    assert ncc[0, 1, 1, 1, 1] == 0 and np.count_nonzero(ncc) == ncc.size - 1            # constant samples under the patch at shift 0 alone
    assert np.array_equal(ncc, vt.utils.normalized_scores(scores, moments, rm, pixels=np.full((3, 3), 20.0)))
    assert np.array_equal(ncc, vt.utils.normalized_scores(scores, moments, rm, pixels=20))
    assert np.array_equal(ncc, sv.correlate_stack_normalized(ref, (1, 1), (3, 3)))
    flat = ref.copy()
    flat[0:4, 0:5] = -2.0                                                                # a constant patch of the reference
    got = sv.correlate_stack_normalized(flat, (1, 1), (3, 3))
    assert not got[0, 0, 0].any() and got[0, 0, 1].all()
    for value in (np.nan, np.inf, -np.inf):                                              # a non-finite moment
        m2 = moments.copy()
        m2[0, 2, 0, 1, 2, 0] = value
        got = vt.utils.normalized_scores(scores, m2, rm, image_shape=(12, 15))
        assert got[0, 2, 0, 1, 2] == 0 and np.isfinite(got).all()
        keep = np.ones(ncc.shape, bool)
        keep[0, 2, 0, 1, 2] = False
        assert np.array_equal(got[keep], ncc[keep])
        s2 = scores.copy()
        s2[0, 0, 2, 0, 0] = value
        assert vt.utils.normalized_scores(s2, moments, rm, image_shape=(12, 15))[0, 0, 2, 0, 0] == 0
    # an image with a NaN pixel: 0 exactly where its window covers the pixel
    bad = img.copy()
    bad[0, 2, 13] = np.nan
    got = vt.StaticVolume(bad, device='cpu').correlate_stack_normalized(ref, (1, 1), (3, 3))
    hit = msm.covered(12, 15, (1, 1), (3, 3), 2, 13)
    assert np.isfinite(got).all() and not got[0][hit].any() and hit.any()
    for kw in (dict(), dict(image_shape=(12, 15), pixels=20), dict(pixels=0)):
        with pytest.raises(ValueError):
            vt.utils.normalized_scores(scores, moments, rm, **kw)
    with pytest.raises(ValueError):
        vt.utils.normalized_scores(scores, moments[..., :1], rm, pixels=20)
    with pytest.raises(ValueError):
        vt.utils.normalized_scores(scores, moments, rm[:, :2], pixels=20)


def test_normalized_find_shifts_recovers_what_raw_scores_miss():
    """Images of mean 10 with a bright blob beside the centre patch: the raw product sum peaks where the blob slides under the patch,
    on the rim of the +-5 window in all 18 trials (6 seeds x 3 true shifts); the correlation coefficient peaks at the true shift with
    value 1 and a runner-up of at most 0.26."""
    msc.check_recovery(msc.recovery('cpu'))


# ---- refusals and the symbol ----------------------------------------------------------------------------------------------------------
def test_python_refusals():
    s = msc.stack('small')
    T, H, W = s.shape
    sv = vt.StaticVolume(s, device='cpu')
    ok = sv.moments_stack((1, 1))
    assert ok.shape == (T, 1, 1, 3, 3, 2) and ok.dtype == np.float64
    bad = [
        dict(max_shift=(H, 0)), dict(max_shift=(0, W)), dict(max_shift=(-1, 0)), dict(max_shift=3), dict(max_shift=(1.0, 1)),
        dict(max_shift=(1, 1, 1)), dict(patch_grid=(0, 1)), dict(patch_grid=(H + 1, 1)), dict(patch_grid=(1, W + 1)), dict(patch_grid=(True, 1)),
        dict(planes=[T]), dict(planes=[-1]), dict(planes=[0.5]), dict(planes=[]),
        dict(output=np.zeros((T, 1, 1, 3, 3, 2), np.float32), max_shift=(1, 1)), dict(output=np.zeros((T, 1, 1, 3, 3)), max_shift=(1, 1)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            sv.moments_stack(**kw)
    # the texts are correlate_stack's
    ref = np.zeros((H, W), np.float32)
    for kw in (dict(max_shift=(H, 0)), dict(patch_grid=(0, 1)), dict(planes=[T]), dict(max_shift=3)):
        with pytest.raises(ValueError) as mine:
            sv.moments_stack(**kw)
        with pytest.raises(ValueError) as theirs:
            sv.correlate_stack(ref, **kw)
        assert str(mine.value) == str(theirs.value)
    with pytest.raises(ValueError, match='linear'):
        vt.StaticVolume(s, 'filt_bspline', device='cpu').moments_stack()
    with pytest.raises(ValueError, match='2\\^31'):
        vt.StaticVolume(np.zeros((1, 300, 300), np.float32), device='cpu').moments_stack((299, 299), planes=np.zeros(3000, int))
    with pytest.raises(ValueError):
        sv.correlate_stack_normalized(ref, (1, 1), output=np.zeros((T, 1, 1, 3, 3), np.float32))
    with pytest.raises(ValueError):
        sv.correlate_stack_normalized()
    assert np.array_equal(sv.moments_stack((1, 1)), ok)


def test_resident_references_on_the_cpu_path():
    s = msc.stack('small')
    sv = vt.StaticVolume(s, device='cpu')
    rp = np.array([1, 2, 3, 4, 0])
    a = sv.correlate_stack_normalized(max_shift=(2, 3), patch_grid=(2, 2), reference_planes=rp)
    b = sv.correlate_stack_normalized(s[rp], (2, 3), (2, 2))
    assert np.array_equal(a, b) and a.shape == (5, 2, 2, 5, 7)
    assert np.array_equal(sv.find_shifts(max_shift=(2, 3), reference_planes=np.arange(5), normalized=True, subpixel=False), np.zeros((5, 1, 1, 2)))


def test_symbol_is_declared():
    assert 'vt_volume_moments_stack' in _native.SYMBOLS
    with open(_native.__file__) as f:
        assert 'L.vt_volume_moments_stack.argtypes' in f.read()
    assert vt.utils.patch_moments is vt.utils.correlation.patch_moments and vt.utils.normalized_scores is vt.utils.correlation.normalized_scores
