"""No GPU: the model of correlate_stack against a plain loop and scipy.signal.correlate2d, the device='cpu' path against the model on
every case of the GPU tests, utils.patch_bounds, utils.peak_shifts, find_shifts recovering known shifts and align_stack undoing them,
the refusals Python makes itself, and the symbol."""
import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import correlate_stack_model as csm
import correlate_stack_cases as csc

try:
    from scipy.signal import correlate2d
except ImportError:                                           # the loop alone
    correlate2d = None


# ---- the model ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', [(1, 1), (2, 3), (5, 1), (1, 7)])
@pytest.mark.parametrize('max_shift', [(0, 0), (1, 2), (4, 6)])
def test_model_is_the_plain_loop(max_shift, grid):
    rng = np.random.default_rng(3)
    img = rng.standard_normal((5, 7)).astype(np.float32)
    ref = rng.standard_normal((5, 7)).astype(np.float32)
    vals, bounds = csm.model(img[None], ref, max_shift, grid)
    want = csm.naive(img, ref, max_shift, grid)
    assert vals.shape == (1,) + want.shape
    assert (np.abs(vals[0] - want) <= bounds[0]).all() and np.abs(vals[0] - want).max() < 1e-13


@pytest.mark.skipif(correlate2d is None, reason='scipy.signal is not installed')
def test_model_is_scipy_correlate2d():
    """The (1, 1) grid at the full window is scipy.signal.correlate2d(image, reference, 'full'): its entry [k, l] is
    sum r[y, x] s[y + k - (H - 1), x + l - (W - 1)]."""
    s = csc.stack('small')
    ref = csc.references('small', 1)[0]
    H, W = s.shape[1:]
    vals, bounds = csm.model(s, ref, (H - 1, W - 1), (1, 1))
    for i in range(s.shape[0]):
        want = correlate2d(s[i].astype(np.float64), ref.astype(np.float64), 'full')
        assert (np.abs(vals[i, 0, 0] - want) <= 2 * bounds[i, 0, 0] + 1e-300).all()
    # a smaller window is the centre of the larger one
    small, _ = csm.model(s, ref, (2, 7), (1, 1))
    assert np.array_equal(small, vals[:, :, :, H - 1 - 2:H - 1 + 3, W - 1 - 7:W - 1 + 8])


def test_model_patches_add_up_and_nan_sets():
    s = csc.stack('small').copy()
    ref = csc.references('small', 1)[0]
    whole, _ = csm.model(s, ref, (2, 3), (1, 1))
    parts, _ = csm.model(s, ref, (2, 3), (3, 5))
    assert np.allclose(parts.sum(axis=(1, 2)), whole[:, 0, 0], rtol=0, atol=1e-11)
    # a NaN image pixel reaches the (patch, shift) pairs whose window covers it; outside zeros are multiplied, so a NaN reference pixel
    # takes its whole patch
    s[1, 6, 12] = np.nan
    vals, _ = csm.model(s, ref, (2, 3), (3, 5))
    bad = np.isnan(vals)
    assert not bad[[0, 2, 3, 4]].any() and bad[1].any()
    ye, xe = vt.utils.patch_bounds(19, 3), vt.utils.patch_bounds(37, 5)
    for a in range(3):
        for b in range(5):
            for u in range(5):
                for v in range(7):
                    y, x = 6 - (u - 2), 12 - (v - 3)                                    # the reference pixel that meets the NaN
                    assert bad[1, a, b, u, v] == (ye[a] <= y < ye[a + 1] and xe[b] <= x < xe[b + 1])
    r2 = ref.copy()
    r2[0, 36] = np.inf                                                                   # at every shift: inf times a sample or a zero
    vals, _ = csm.model(csc.stack('small'), r2, (2, 3), (3, 5))
    assert not np.isfinite(vals[:, 0, 4]).any() and np.isfinite(np.delete(vals.reshape(5, 15, 5, 7), 4, axis=1)).all()


def test_plan_names_its_edges():
    assert csm.max_lds_bytes() == 56992 <= 64 * 1024
    ev, eu = csm.block_edges_v(60), csm.block_edges_u(40, 60)
    assert ev and {csm.plan(41, 61, (0, rw), (1, 1))['runs'] for _, rw in eu} == set(range(1, 8))
    for rw in ev:
        assert csm.plan(1, 200, (0, rw), (1, 1))['blocks_v'] != csm.plan(1, 200, (0, rw + 1), (1, 1))['blocks_v']
    for rh, rw in eu:
        assert csm.plan(99, 99, (rh, rw), (1, 1))['blocks_u'] == 1 and csm.plan(99, 99, (rh + 1, rw), (1, 1))['blocks_u'] == 2
    names = {c['name'] for c in csc.CASES}
    for rw in ev:
        assert {f'pieces-v-edge-{rw}', f'pieces-v-edge-{rw + 1}'} <= names
    for p in (csm.plan(512, 512, (8, 8), (1, 1)), csm.plan(1024, 1024, (16, 16), (8, 8)), csm.plan(19, 37, (18, 36), (19, 37))):
        assert p['rows_blk'] * p['runs'] <= 64 and p['cv'] in (9, 11) and p['lds_bytes'] <= 56992
    assert csm.launches(97, 150, (3, 3), (1, 1), 5, cap=2 * 6 * 49 * 8) == (2, 1)


# ---- the CPU path ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('c', csc.CASES, ids=[c['name'] for c in csc.CASES])
def test_cpu_path_matches_the_model(c):
    s, refs, kw = csc.arguments(c)
    got = vt.StaticVolume(s, device='cpu').correlate_stack(refs, c['max_shift'], c['grid'], **kw)
    csm.check(got, *csm.model(s, refs, c['max_shift'], c['grid'], kw['planes'], kw.get('reference_planes')), c['name'])


def test_cpu_path_on_integers_is_exact_and_fills_output():
    c = next(c for c in csc.CASES if c['name'] == 'small-g35')
    s, refs, kw = csc.arguments(c, integers=True)
    vals, _ = csm.model(s, refs, c['max_shift'], c['grid'], kw['planes'])
    sv = vt.StaticVolume(s, device='cpu')
    assert np.array_equal(sv.correlate_stack(refs, c['max_shift'], c['grid'], **kw), vals)
    out = np.full(vals.shape, 7.0)
    assert sv.correlate_stack(refs, c['max_shift'], c['grid'], output=out, **kw) is out and np.array_equal(out, vals)


# ---- utils ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('extent', [1, 2, 19, 37, 64, 97])
def test_patch_bounds(extent):
    for g in {1, 2, 3, 5, extent // 2, extent - 1, extent} - {0}:
        if g > extent:
            continue
        e = vt.utils.patch_bounds(extent, g)
        assert e.shape == (g + 1,) and e[0] == 0 and e[-1] == extent and (np.diff(e) >= 1).all()       # disjoint, none empty, the union
        assert list(e) == csm.patch_edges(extent, g)
        assert np.diff(e).max() - np.diff(e).min() <= 1
    assert list(vt.utils.patch_bounds(extent, 1)) == [0, extent]
    assert list(vt.utils.patch_bounds(extent, extent)) == list(range(extent + 1))
    for bad in (0, extent + 1, -1, 1.5, True):
        with pytest.raises(ValueError):
            vt.utils.patch_bounds(extent, bad)


def test_peak_shifts_finds_a_planted_peak_everywhere():
    rh, rw = 2, 3
    rng = np.random.default_rng(11)
    base = rng.uniform(-1, 0, (2 * rh + 1, 2 * rw + 1))
    scores = np.empty((2 * rh + 1, 2 * rw + 1) + base.shape)
    for u in range(2 * rh + 1):
        for v in range(2 * rw + 1):
            scores[u, v] = base
            scores[u, v, u, v] = 5.0
    whole = vt.utils.peak_shifts(scores, subpixel=False)
    fine = vt.utils.peak_shifts(scores)
    assert whole.shape == fine.shape == (2 * rh + 1, 2 * rw + 1, 2) and whole.dtype == fine.dtype == np.float64
    for u in range(2 * rh + 1):
        for v in range(2 * rw + 1):
            assert tuple(whole[u, v]) == (u - rh, v - rw)
            d = fine[u, v] - whole[u, v]
            assert (np.abs(d) < 0.5).all()
            if u in (0, 2 * rh):
                assert d[0] == 0                                                         # on the rim: no parabola along that axis
            if v in (0, 2 * rw):
                assert d[1] == 0


def test_peak_shifts_refinement():
    y, x = np.mgrid[-3:4, -4:5].astype(np.float64)
    sym = -(y ** 2) - 2 * x ** 2                                                         # symmetric about the centre: exactly 0
    assert np.array_equal(vt.utils.peak_shifts(sym), [0.0, 0.0])
    par = -((y - 1.25) ** 2) - 2 * (x + 0.75) ** 2                                       # a parabola is recovered exactly
    assert np.allclose(vt.utils.peak_shifts(par), [1.25, -0.75], rtol=0, atol=1e-12)
    flat = np.zeros((5, 5))                                                              # denominator 0: nothing added, first maximum
    assert np.array_equal(vt.utils.peak_shifts(flat), [-2.0, -2.0])
    tie = np.zeros((1, 5))
    tie[0, 2] = tie[0, 3] = 1.0                                                          # the half-way point stays inside (-0.5, 0.5)
    d = vt.utils.peak_shifts(tie)
    assert d[0] == 0 and 0.49 < d[1] < 0.5
    rng = np.random.default_rng(5)
    r = vt.utils.peak_shifts(rng.standard_normal((200, 7, 9)))
    assert (np.abs(r - np.round(r)) < 0.5).all() and (np.abs(r[:, 0]) <= 3.5).all() and (np.abs(r[:, 1]) <= 4.5).all()
    assert vt.utils.peak_shifts(np.zeros((0, 3, 3))).shape == (0, 2)
    with pytest.raises(ValueError):
        vt.utils.peak_shifts(np.zeros((3, 4)))


# ---- find_shifts ----------------------------------------------------------------------------------------------------------------------
def shifted_series(grid, patch=(32, 40), R=4, n=3, seed=0):
    """A reference cut from a larger zero-mean white field, and n images whose patch (a, b) shows the field displaced by its own
    integer d[i, a, b]: image[y + d] == reference[y] for every y of the patch whose y + d stays inside the patch's own cell.  Cells are
    cut from the field by slicing (no wrap-around), so image and reference truly overlap."""
    rng = np.random.default_rng(seed)
    gh, gw = grid
    H, W = gh * patch[0], gw * patch[1]
    field = rng.standard_normal((H + 2 * R, W + 2 * R)).astype(np.float32)
    ref = field[R:R + H, R:R + W]
    d = rng.integers(-R, R + 1, (n, gh, gw, 2))
    imgs = np.empty((n, H, W), np.float32)
    for i in range(n):
        for a in range(gh):
            for b in range(gw):
                y0, x0 = a * patch[0], b * patch[1]
                dy, dx = d[i, a, b]
                # image[y] = field[R + y - d]: image[y + d] = field[R + y] = ref[y]
                imgs[i, y0:y0 + patch[0], x0:x0 + patch[1]] = field[R + y0 - dy:R + y0 - dy + patch[0], R + x0 - dx:R + x0 - dx + patch[1]]
    return np.ascontiguousarray(ref), imgs, d


@pytest.mark.parametrize('grid', [(1, 1), (2, 3)])
def test_find_shifts_recovers_known_shifts(grid):
    R = 4
    ref, imgs, d = shifted_series(grid, R=R)
    # the model alone meets the premise: on white data the peak stands well above every other score of its window
    vals, _ = csm.model(imgs, ref, (R, R), grid)
    flat = vals.reshape(vals.shape[:3] + (-1,))
    top2 = np.sort(flat, axis=-1)[..., -2:]
    assert (top2[..., 1] > 3 * np.abs(top2[..., 0])).all(), float((top2[..., 1] / np.abs(top2[..., 0])).min())
    assert np.array_equal(vt.utils.peak_shifts(vals, subpixel=False), d)
    sv = vt.StaticVolume(imgs, device='cpu')
    got = sv.find_shifts(ref, (R, R), grid)
    assert got.shape == d.shape and got.dtype == np.float64
    assert np.array_equal(np.round(got), d) and (np.abs(got - d) < 0.5).all()
    assert np.array_equal(sv.find_shifts(ref, (R, R), grid, subpixel=False), d)
    # against a resident reference: the series appended to its own reference
    both = np.concatenate([ref[None], imgs])
    sv2 = vt.StaticVolume(both, device='cpu')
    n = imgs.shape[0]
    got2 = sv2.find_shifts(max_shift=(R, R), patch_grid=grid, planes=np.arange(1, n + 1), reference_planes=np.zeros(n, int))
    assert np.array_equal(got2, got)


def test_align_stack_with_minus_d_restores_the_reference():
    R = 4
    ref, imgs, d = shifted_series((1, 1), patch=(40, 48), R=R)
    sv = vt.StaticVolume(imgs, device='cpu', stack=True)
    found = sv.find_shifts(ref, (R, R), subpixel=False)
    assert np.array_equal(found, d)
    back = sv.align_stack(shifts=-found[:, 0, 0])
    inner = (slice(None), slice(R, -R), slice(R, -R))                                   # the overlap whatever d is
    assert np.abs(back[inner] - ref[None][inner]).max() < 1e-5


# ---- refusals and the symbol ----------------------------------------------------------------------------------------------------------
def test_python_refusals():
    s = csc.stack('small')
    T, H, W = s.shape
    ref = csc.references('small', 1)[0]
    sv = vt.StaticVolume(s, device='cpu')
    ok = sv.correlate_stack(ref, (1, 1))
    assert ok.shape == (T, 1, 1, 3, 3) and ok.dtype == np.float64
    bad = [
        dict(),                                                                           # neither reference
        dict(references=ref, reference_planes=[0] * T),                                   # both
        dict(references=ref[:-1]), dict(references=np.zeros((0, H, W))), dict(references=np.zeros((2, 2, H, W))),
        dict(references=np.full((H, W), np.nan)), dict(references=np.where(np.arange(W) == 3, np.inf, ref)),
        dict(references=np.stack([ref] * 3)),                                             # n = 3 != T without planes
        dict(references=np.stack([ref] * 3), planes=[0, 1]),
        dict(references=ref, max_shift=(H, 0)), dict(references=ref, max_shift=(0, W)), dict(references=ref, max_shift=(-1, 0)),
        dict(references=ref, max_shift=3), dict(references=ref, max_shift=(1.0, 1)), dict(references=ref, max_shift=(1, 1, 1)),
        dict(references=ref, patch_grid=(0, 1)), dict(references=ref, patch_grid=(H + 1, 1)), dict(references=ref, patch_grid=(1, W + 1)),
        dict(references=ref, patch_grid=(True, 1)),
        dict(references=ref, planes=[T]), dict(references=ref, planes=[-1]), dict(references=ref, planes=[0.5]), dict(references=ref, planes=[]),
        dict(reference_planes=[T] * T), dict(reference_planes=[0, 1]), dict(reference_planes=[0, 1], planes=[0, 1, 2]),
        dict(references=ref, output=np.zeros((T, 1, 1, 3, 3), np.float32), max_shift=(1, 1)),
        dict(references=ref, output=np.zeros((T, 1, 1, 3, 5)), max_shift=(1, 1)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            sv.correlate_stack(**kw)
    with pytest.raises(ValueError, match='linear'):
        vt.StaticVolume(s, 'filt_bspline', device='cpu').correlate_stack(ref)
    with pytest.raises(ValueError, match='2\\^31'):
        vt.StaticVolume(np.zeros((1, 300, 300), np.float32), device='cpu').correlate_stack(          # 6000 x 599 x 599 scores
            np.zeros((300, 300)), (299, 299), planes=np.zeros(6000, int))
    assert np.array_equal(sv.correlate_stack(ref, (1, 1)), ok)


def test_symbol_is_declared():
    assert 'vt_volume_correlate_stack' in _native.SYMBOLS
    with open(_native.__file__) as f:
        assert 'L.vt_volume_correlate_stack.argtypes' in f.read()
