"""StaticVolume.place / place_at and utils.place_matrices without a GPU: the matrices against box_matrices, the CPU device against
extract_sum at box_shape = output_shape, accumulation, argument errors, and the C entry points' symbols, flags and argument codes."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
SHAPE = (9, 11, 10)                    # the small map the handle holds
OUT = (20, 22, 24)
POS = np.array([[9.5, 10.25, 12.0], [6.0, 14.5, 8.75], [12.25, 9.0, 15.5], [10.0, 11.0, 22.5], [40.0, 50.0, 60.0]])   # the fourth hangs over a face, the fifth is outside
ROT = np.array([[10.0, 20.0, 30.0], [0.0, 0.0, 0.0], [-40.0, 15.0, 80.0], [5.0, -10.0, 20.0], [90.0, 45.0, -30.0]])
W = np.array([0.5, -1.25, 2.0, 1.0, 0.75])


@pytest.fixture(scope='module')
def vol():
    return np.random.RandomState(52).random_sample(SHAPE).astype(np.float32)


@pytest.mark.parametrize('units', ['deg', 'rad'])
@pytest.mark.parametrize('order', ['rzxz', 'sxyz'])
@pytest.mark.parametrize('box', [(16, 16, 16), (9, 12, 17)])
def test_place_matrices_invert_box_matrices(box, order, units):
    rs = np.random.RandomState(7)
    pos = rs.uniform(-50, 1000, (20, 3))
    rot = rs.uniform(-180, 180, (20, 3)) if units == 'deg' else rs.uniform(-np.pi, np.pi, (20, 3))
    place = vt.utils.place_matrices(pos, rot, box, rotation_units=units, rotation_order=order)
    pull = vt.utils.box_matrices(pos, rot, box, rotation_units=units, rotation_order=order)
    assert place.shape == (20, 4, 4) and place.dtype == np.float64
    c = (np.asarray(box, np.float64) - 1) / 2
    for i in range(20):
        assert np.abs(place[i] @ pull[i] - np.eye(4)).max() <= 1e-12, i
        assert np.abs(pull[i] @ place[i] - np.eye(4)).max() <= 1e-12, i
        r3 = vt.utils.rotation_matrix(rot[i], units, order, dtype=np.float64)[:3, :3]
        assert np.array_equal(place[i, :3, :3], r3.T) and np.array_equal(place[i, 3], [0, 0, 0, 1])
        assert np.abs(place[i, :3, :3] @ pos[i] + place[i, :3, 3] - c).max() <= 1e-12      # the copy's centre lands at the position


def test_place_matrices_without_rotation_and_argument_errors():
    box = (6, 7, 8)
    c = (np.asarray(box) - 1) / 2
    starts = np.array([[3, 4, 5], [-2, 20, 25]])
    ms = vt.utils.place_matrices(starts + c, None, box)
    for i in range(2):
        assert np.array_equal(ms[i, :3, :3], np.eye(3)) and np.array_equal(ms[i, :3, 3], -starts[i].astype(np.float64))
    with pytest.raises(ValueError):
        vt.utils.place_matrices(np.zeros((0, 3)), None, box)
    with pytest.raises(ValueError):
        vt.utils.place_matrices(np.zeros((2, 3)), np.zeros((3, 3)), box)
    with pytest.raises(ValueError):
        vt.utils.place_matrices(np.zeros((2, 3)), None, (6, 0, 8))


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_place_equals_extract_sum_at_the_output_shape(interp, vol):
    ms = vt.utils.place_matrices(POS, ROT, SHAPE)
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.place(ms, OUT, W)
    assert got.shape == OUT and got.dtype == np.float32 and np.abs(got).max() > 0.5
    assert np.array_equal(got, sv.extract_sum(ms, OUT, W))
    assert np.array_equal(sv.place(ms, OUT), sv.extract_sum(ms, OUT))                      # no weights: ones
    assert np.array_equal(got, sv.place(ms[:4], OUT, W[:4]))                               # the copy outside adds nothing
    assert np.array_equal(sv.place_at(POS, ROT, OUT, W), got)
    assert np.array_equal(sv.place_at(POS, None, OUT, rotation_order='sxyz'), sv.place(vt.utils.place_matrices(POS, None, SHAPE), OUT))
    out = np.full(OUT, 7, np.float32)
    assert sv.place(ms, OUT, W, output=out) is out and np.array_equal(out, got)


def test_cpu_place_at_puts_an_axis_aligned_copy_where_the_crop_was(vol):
    sv = vt.StaticVolume(vol, interpolation='linear', device='cpu')
    c = (np.asarray(SHAPE) - 1) / 2
    start = np.array([4, 5, 6])
    got = sv.place_at((start + c)[None], None, OUT, [2.0])
    want = np.zeros(OUT, np.float32)
    want[4:4 + SHAPE[0], 5:5 + SHAPE[1], 6:6 + SHAPE[2]] = 2.0 * vol
    assert np.array_equal(got, want)


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_accumulate_starts_from_the_output(interp, vol):
    ms = vt.utils.place_matrices(POS, ROT, SHAPE)
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    base = np.random.RandomState(53).standard_normal(OUT).astype(np.float32)
    out = base.copy()
    assert sv.place(ms, OUT, W, output=out, accumulate=True) is out
    order = 1 if interp == 'linear' else 3
    from scipy.ndimage import affine_transform, spline_filter
    data = vol if interp == 'linear' else spline_filter(vol, 3, output=np.float64, mode='constant')
    acc = base.astype(np.float64)
    one = np.empty(OUT, np.float32)
    for i in range(len(ms)):
        affine_transform(data, ms[i], output_shape=OUT, output=one, order=order, prefilter=False)
        acc += W[i] * one.astype(np.float64)
    assert np.array_equal(out, acc.astype(np.float32))
    assert not np.array_equal(out, base)
    untouched = sv.place(ms, OUT, W) == 0
    assert untouched.any() and np.array_equal(out[untouched], base[untouched])             # adding +0 changes nothing
    # subtracting what was added gives the base back to rounding
    assert sv.place(ms, OUT, -W, output=out, accumulate=True) is out
    assert np.abs(out - base).max() <= 1e-5
    out2 = base.copy()
    sv.place_at(POS, ROT, OUT, W, output=out2, accumulate=True)
    assert np.array_equal(out2, acc.astype(np.float32))


def test_argument_errors(vol):
    sv = vt.StaticVolume(vol, device='cpu')
    ms = vt.utils.place_matrices(POS, ROT, SHAPE)
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.place(bad, OUT)
    with pytest.raises(ValueError):
        sv.place(ms, OUT, W[:4])
    with pytest.raises(ValueError):
        sv.place(ms, OUT, np.ones((5, 1)))
    for bad in (np.nan, np.inf):
        w = W.copy()
        w[2] = bad
        with pytest.raises(ValueError):
            sv.place(ms, OUT, w)
        with pytest.raises(ValueError):
            sv.place_at(POS, ROT, OUT, w)
    with pytest.raises(ValueError):
        sv.place(ms, OUT, W, output=np.zeros((20, 22, 25), np.float32))
    with pytest.raises(ValueError):
        sv.place(ms, OUT, W, output=np.zeros((5,) + OUT, np.float32))
    for shape in ((20, 0, 24), (20, 22), (20, 22, 24.0), None):
        with pytest.raises(ValueError):
            sv.place(ms, shape)
    with pytest.raises(ValueError):
        sv.place(ms, OUT, W, accumulate=True)                                              # nothing to add into
    with pytest.raises(ValueError):
        sv.place_at(POS, ROT, OUT, W, accumulate=True)
    with pytest.raises(ValueError):
        sv.place_at(POS[:4], ROT, OUT)


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    w = np.ones(1)
    out = np.zeros((4, 4, 4), np.float32)
    assert lib.vt_volume_place(None, 1, m32.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_place_f64(None, 1, m64.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_place_f64(None, 1, m64.ctypes.data, None, 4, 4, 4, out.ctypes.data, _native.ACCUMULATE) == VT_EINVAL
    assert lib.vt_last_error()


def header_flags():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    body = re.search(r'enum vt_flags \{(.*?)\};', header, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    return {k: int(val) for k, val in re.findall(r'\b(VT_[A-Z_]+)\s*=\s*(\d+)', body)}


def test_symbols_and_flags_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_place', 'vt_volume_place_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 9
    assert '17 posed weighted copies summed into one map' in header     # the last_kernel comment names the new kernel
    flags = header_flags()
    assert flags['VT_ACCUMULATE'] == _native.ACCUMULATE and flags['VT_PLACE_DENSE'] == _native.PLACE_DENSE
    # free bits: the two new values are single bits no other flag uses, and every earlier flag kept its value
    values = list(flags.values())
    assert len(set(values)) == len(values) and all(val & (val - 1) == 0 for val in values)
    assert flags['VT_NO_PLANSHARE'] == _native.NO_PLANSHARE == 131072 and flags['VT_OUT_DEVICE'] == 1 and flags['VT_FORCE_DIRECT'] == 4
