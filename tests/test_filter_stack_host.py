"""No GPU: the float64 model of filter_stack against scipy, the device='cpu' path against the model, utils.ramp_taps, ramp_filter's axis
choice, the refusals Python makes itself, and the reason the call exists: a ramp-filtered series back-projects closer to its phantom."""
import numpy as np
import pytest
from scipy.ndimage import convolve1d

import voltools_amd as vt

import filter_stack_model as fm

STACK = (5, 19, 37)
PLANES = np.array([0, 4, 2, 2, 3, 1, 0])
WEIGHTS = np.array([0.75, -1.5, 2.0, 0.0, 1.25, -0.5, 1.0])
ASYM9 = np.array([0.5, -1.25, 0.0, 2.0, 0.75, 0.0, -0.375, 1.5, 0.25])


def data(shape=STACK, seed=5):
    return np.random.RandomState(seed).random_sample(shape).astype(np.float32)


@pytest.mark.parametrize('pad', ['zero', 'edge'])
@pytest.mark.parametrize('axis', [1, 2])
def test_model_is_scipy_convolve1d(axis, pad):
    s = data()
    for taps in (np.array([1.0, 2.0, 3.0]), ASYM9, vt.utils.ramp_taps(STACK[axis])):
        vals, bounds = fm.model(s, taps, axis, pad)
        want = convolve1d(s.astype(np.float64), taps, axis=axis, mode='constant' if pad == 'zero' else 'nearest', origin=0)
        assert np.abs(vals - want).max() <= 1e-13 * np.abs(taps).sum()
        assert (bounds > 0).all()
    # the orientation, spelled out: numpy.convolve(line, t, 'same')
    line = s[1, 3] if axis == 2 else s[1, :, 3]
    got = fm.model(s, [1.0, 2.0, 3.0], axis, 'zero')[0][1]
    got = got[3] if axis == 2 else got[:, 3]
    assert np.allclose(got, np.convolve(line.astype(np.float64), [1.0, 2.0, 3.0], 'same'), rtol=0, atol=1e-14)


def test_model_skips_zero_taps_and_pad_zero_taps_outside():
    s = data()
    s[2, 7, 0] = np.nan
    taps = vt.utils.ramp_taps(STACK[2], half_width=4)
    vals, _ = fm.model(s, taps, 2, 'zero')
    bad = np.isnan(vals[2, 7])
    assert np.array_equal(np.flatnonzero(bad), [0, 1, 3])                     # offsets 0, 1, 3: the non-zero taps of a Ram-Lak row
    assert not np.isnan(vals[2, 6]).any()


@pytest.mark.parametrize('pad', ['zero', 'edge'])
@pytest.mark.parametrize('axis', [1, 2])
def test_cpu_path_matches_the_model(axis, pad):
    s = data()
    sv = vt.StaticVolume(s, device='cpu')
    per_entry = np.random.RandomState(9).uniform(-1, 1, (len(PLANES), 9))
    per_entry[3, 2:5] = 0
    for taps in (ASYM9, per_entry, vt.utils.ramp_taps(STACK[axis])):
        got = sv.filter_stack(taps, axis, WEIGHTS, pad, planes=PLANES)
        vals, bounds = fm.model(s, taps, axis, pad, PLANES, WEIGHTS)
        fm.check(got, vals, bounds, ('cpu', axis, pad, np.shape(taps)))
    got = sv.filter_stack(ASYM9, axis, pad=pad)                                 # planes None: n = T, weights None: ones
    fm.check(got, *fm.model(s, ASYM9, axis, pad), ('cpu, defaults', axis, pad))
    out = np.zeros(STACK, np.float32)
    assert sv.filter_stack(ASYM9, axis, pad=pad, output=out) is out and np.array_equal(out, got)


def test_ramp_taps_closed_forms():
    t = vt.utils.ramp_taps(32)
    assert t.dtype == np.float64 and t.shape == (63,)
    want = [0.25, -1 / np.pi ** 2, 0.0, -1 / (3 * np.pi) ** 2, 0.0, -1 / (5 * np.pi) ** 2]
    for m, v in enumerate(want):
        assert t[31 + m] == pytest.approx(v, rel=1e-15, abs=0) and t[31 - m] == t[31 + m]
    m = np.arange(-31, 32)
    assert (t[(m % 2 == 0) & (m != 0)] == 0).all() and (t[m % 2 != 0] < 0).all()
    s = vt.utils.ramp_taps(32, 'shepp-logan')
    for k in range(6):
        assert s[31 + k] == pytest.approx(-2 / (np.pi ** 2 * (4 * k * k - 1)), rel=1e-15, abs=0)
    assert s[31] == pytest.approx(2 / np.pi ** 2, rel=1e-15)


@pytest.mark.parametrize('window', vt.utils.AVAILABLE_WINDOWS)
@pytest.mark.parametrize('extent', [1, 2, 31, 32, 100])
def test_ramp_taps_symmetry_and_half_width(window, extent):
    t = vt.utils.ramp_taps(extent, window)
    assert t.dtype == np.float64 and t.shape == (2 * extent - 1,) and np.isfinite(t).all()
    assert np.array_equal(t, t[::-1])
    assert t[extent - 1] > 0
    for hw in {0, min(3, extent - 1), extent - 1}:
        cut = vt.utils.ramp_taps(extent, window, half_width=hw)
        assert cut.shape == (2 * hw + 1,) and np.array_equal(cut, t[extent - 1 - hw:extent + hw])


@pytest.mark.parametrize('extent', [31, 32, 33, 64])
def test_hann_response_at_nyquist(extent):
    """The Hann window is 0 at f = 1/2, so the windowed ring sums to 0 against (-1)^m.  Multiplying by the window over frequency is a
    convolution of the Ram-Lak taps with (1/4, 1/2, 1/4) over m, which reaches one tap beyond the 2 extent - 1 that are returned: the row
    itself sums to (-1)^r t_ramp[r] / 2 with r = extent - 1, which is exactly 0 for odd extents (even r).  The tolerance is float64
    rounding: two transforms of `size` points (a few log2(size) ulps of the row's 1-norm, at most 1/2) and the sum of 2r + 1 terms."""
    r = extent - 1
    t = vt.utils.ramp_taps(extent, 'hann')
    ramp = vt.utils.ramp_taps(extent)
    size = 1 << int(np.ceil(np.log2(2 * extent)))
    tol = 2.0 ** -53 * (8 * np.log2(size) + (2 * r + 1)) * np.abs(ramp).sum()
    m = np.arange(-r, r + 1)
    nyquist = float(np.sum(t * (-1.0) ** m))
    print(f'extent {extent}: response at Nyquist {nyquist:.3e}, truncation term {0.5 * (-1.0) ** r * ramp[-1]:.3e}, tolerance {tol:.3e}')
    assert abs(nyquist - 0.5 * (-1.0) ** r * ramp[-1]) <= tol
    if extent % 2:
        assert ramp[-1] == 0 and abs(nyquist) <= tol
    # and the response at frequency 0 is that of the ramp itself, the window being 1 there
    assert abs(t.sum() - (ramp.sum() - 0.5 * ramp[-1])) <= tol


def test_ramp_taps_refusals():
    for bad in (0, -3, 2.5, True, None):
        with pytest.raises(ValueError):
            vt.utils.ramp_taps(bad)
    with pytest.raises(ValueError):
        vt.utils.ramp_taps(8, 'boxcar')
    for hw in (-1, 8, 1.5):
        with pytest.raises(ValueError):
            vt.utils.ramp_taps(8, half_width=hw)


def test_ramp_filter_picks_the_axis_across_the_tilt_axis():
    s = data()
    sv = vt.StaticVolume(s, device='cpu')
    w = np.linspace(0.5, 1.5, STACK[0])
    for tilt_axis, axis in ((1, 2), (2, 1)):
        for window, hw in (('ramp', None), ('hann', 5)):
            got = sv.ramp_filter(tilt_axis, window, hw, w)
            want = sv.filter_stack(vt.utils.ramp_taps(STACK[axis], window, hw), axis, w, 'edge')
            assert np.array_equal(got, want)
        assert np.array_equal(sv.ramp_filter(tilt_axis, pad='zero'), sv.filter_stack(vt.utils.ramp_taps(STACK[axis]), axis, pad='zero'))
    assert np.array_equal(sv.ramp_filter(), sv.ramp_filter(1))
    for bad in (0, 3, True):
        with pytest.raises(ValueError):
            sv.ramp_filter(bad)


def test_python_side_refusals():
    s = data()
    sv = vt.StaticVolume(s, device='cpu')
    good = np.array([1.0, 2.0, 1.0])
    assert sv.filter_stack(good).shape == STACK
    bad_calls = [
        dict(taps=np.ones(4)),                                    # even
        dict(taps=np.ones(2 * STACK[2] + 1)),                     # beyond 2L - 1
        dict(taps=np.ones(2 * STACK[1] + 1), axis=1),
        dict(taps=np.ones((2, 2, 3))), dict(taps=np.ones(0)), dict(taps=np.ones((0, 3))),
        dict(taps=[1.0, np.nan, 1.0]), dict(taps=[1.0, np.inf, 1.0]),
        dict(taps=good, axis=0), dict(taps=good, axis=3), dict(taps=good, pad='reflect'), dict(taps=good, pad=0),
        dict(taps=np.ones((3, 3))),                               # three rows, five images, no planes
        dict(taps=np.ones((3, 3)), planes=[0, 1]),                # rows != entries
        dict(taps=good, planes=[0, 5]), dict(taps=good, planes=[-1]), dict(taps=good, planes=[0.5]), dict(taps=good, planes=[]),
        dict(taps=good, weights=np.ones(4)), dict(taps=good, weights=[1, 1, np.nan, 1, 1]),
        dict(taps=good, output=np.zeros((5, 19, 36), np.float32)),
    ]
    for kw in bad_calls:
        with pytest.raises(ValueError):
            sv.filter_stack(**kw)
    assert sv.filter_stack(np.ones(2 * STACK[2] - 1)).shape == STACK            # the longest row that reaches anything
    for interp in ('filt_bspline', 'filt_bspline_simple'):
        for stack in (False, True):
            with pytest.raises(ValueError, match='linear'):
                vt.StaticVolume(s, interpolation=interp, device='cpu', stack=stack).filter_stack(good)
    assert vt.StaticVolume(s, interpolation='bspline', device='cpu').filter_stack(good).shape == STACK


@pytest.mark.parametrize('tilt_axis', [1, 2])
def test_ramp_filtered_series_reconstructs_closer_to_the_phantom(tilt_axis):
    plain, filtered = fm.pipeline_correlations(vt, 'cpu', tilt_axis)
    print(f'tilt_axis {tilt_axis}: correlation with the phantom {plain:.3f} unfiltered, {filtered:.3f} ramp-filtered')
    assert filtered > plain
