"""StaticVolume.extract_dot / correlate_at without a GPU: the CPU device against float64 numpy sums over its own extract,
the correlation coefficient of a template cut from the volume, argument errors, and the C entry points' argument codes."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
SHAPE = (20, 22, 24)
BOX = (9, 13, 11)
POS = np.array([[9.5, 10.25, 12.0], [6.0, 14.5, 8.75], [12.25, 9.0, 15.5], [10.0, 11.0, 22.5], [8.5, 12.5, 10.5]])   # the fourth hangs over a face
ROT = np.array([[10.0, 20.0, 30.0], [0.0, 0.0, 0.0], [-40.0, 15.0, 80.0], [5.0, -10.0, 20.0], [90.0, 45.0, -30.0]])


@pytest.fixture(scope='module')
def vol():
    return np.random.RandomState(51).random_sample(SHAPE).astype(np.float32)


def _matrices():
    return vt.utils.box_matrices(POS, ROT, BOX)


def _template_and_mask():
    rs = np.random.RandomState(52)
    tmpl = rs.uniform(-1, 1, BOX).astype(np.float32)
    mask = rs.uniform(0, 1, BOX).astype(np.float32)
    mask[0, 0, 0] = mask[-1, -1, -1] = 0
    return tmpl, mask


def _sums(boxes, tmpl, mask):
    b = boxes.astype(np.float64)
    t, m = tmpl.astype(np.float64), mask.astype(np.float64)
    return np.stack([(m * b).sum(axis=(1, 2, 3)), (m * b * b).sum(axis=(1, 2, 3)), (t * b).sum(axis=(1, 2, 3))], axis=1)


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_dot_equals_numpy_sums_over_extract(interp, vol):
    ms = _matrices()
    tmpl, mask = _template_and_mask()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    boxes = sv.extract(ms, BOX)
    assert (boxes[3] == 0).any() and boxes[3].any()              # the box over the face is cut, not empty
    got = sv.extract_dot(ms, tmpl, mask)
    assert got.shape == (5, 3) and got.dtype == np.float64
    want = _sums(boxes, tmpl, mask)
    assert np.abs(want).min() > 0
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all(), (interp, float(np.abs(got / want - 1).max()))
    out = np.full((5, 3), 7.0)
    assert sv.extract_dot(ms, tmpl, mask, output=out) is out and np.array_equal(out, got)


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_no_mask_means_ones(interp, vol):
    ms = _matrices()
    tmpl, _ = _template_and_mask()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.extract_dot(ms, tmpl)
    assert np.array_equal(got, sv.extract_dot(ms, tmpl, np.ones(BOX, np.float32)))
    assert np.array_equal(got, sv.extract_dot(ms, tmpl.astype(np.float64), np.ones(BOX, int)))      # anything that converts to float32
    want = _sums(sv.extract(ms, BOX), tmpl, np.ones(BOX, np.float32))
    assert (np.abs(got - want) <= 1e-12 * np.abs(want)).all()


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_correlate_at_finds_the_pose_the_template_was_cut_at(interp, vol):
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    p, r = POS[0], ROT[0]
    template = sv.extract_at(p[None], r[None], BOX)[0]
    _, mask = _template_and_mask()
    pos = np.stack([p, p + (1.5, 0, 0), p - (0, 2.0, 1.0), p, POS[2]])
    rot = np.stack([r, r, r, r + (25.0, 0, 0), ROT[2]])
    for m in (None, mask):
        cc = sv.correlate_at(pos, rot, template, m)
        assert cc.shape == (5,) and cc.dtype == np.float64
        assert abs(cc[0] - 1.0) <= 1e-6, (interp, cc)
        assert (cc[1:] < cc[0]).all() and (np.abs(cc) <= 1 + 1e-6).all(), (interp, cc)
    # a box with no variance under the mask scores 0, not NaN
    flat = vt.StaticVolume(np.zeros(SHAPE, np.float32), interpolation=interp, device='cpu')
    assert np.array_equal(flat.correlate_at(pos, rot, template, mask), np.zeros(5))


def test_argument_errors(vol):
    sv = vt.StaticVolume(vol, device='cpu')
    ms = _matrices()
    tmpl, mask = _template_and_mask()
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl[0])                                      # template not 3-D
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask[:, :, :-1])                        # mask of another shape
    nan = tmpl.copy()
    nan[1, 2, 3] = np.nan
    with pytest.raises(ValueError):
        sv.extract_dot(ms, nan, mask)
    inf = mask.copy()
    inf[1, 2, 3] = np.inf
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, inf)
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=np.zeros((5, 3), np.float32))
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=np.zeros((5, 4), np.float64))
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=np.zeros((4, 3), np.float64))
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.extract_dot(bad, tmpl)
    with pytest.raises(ValueError):
        sv.correlate_at(POS, ROT, tmpl, np.zeros(BOX, np.float32))       # N = 0
    with pytest.raises(ValueError):
        sv.correlate_at(POS, ROT, np.full(BOX, 2.0, np.float32), mask)   # sigma_t = 0
    with pytest.raises(ValueError):
        sv.correlate_at(POS, ROT, nan, mask)
    with pytest.raises(ValueError):
        sv.correlate_at(POS, ROT)


def test_float64_outputs_are_checked_by_the_shim():
    out = np.zeros((5, 3), np.float64)
    ptr, is_dev, arr = _native.resolve_output(out, (5, 3), 0, dtype=np.float64)
    assert ptr == out.ctypes.data and not is_dev and arr is out
    for bad in (np.zeros((5, 3), np.float32), np.zeros((3, 5), np.float64).T, np.zeros((5, 4), np.float64)):
        with pytest.raises(ValueError):
            _native.resolve_output(bad, (5, 3), 0, dtype=np.float64)

    class Dev:                                                           # what vt.empty arrays expose: float32
        __cuda_array_interface__ = {'shape': (5, 3), 'typestr': '<f4', 'data': (4096, False), 'version': 2, 'strides': None}

    with pytest.raises(ValueError):
        _native.resolve_output(Dev(), (5, 3), 0, dtype=np.float64)
    Dev.__cuda_array_interface__ = dict(Dev.__cuda_array_interface__, typestr='<f8')
    assert _native.resolve_output(Dev(), (5, 3), 0, dtype=np.float64) == (4096, True, None)
    with pytest.raises(ValueError):
        _native.resolve_output(Dev(), (5, 3), 0)                         # the float32 entry points still refuse float64


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    t = np.ones((4, 4, 4), np.float32)
    out = np.zeros((1, 3), np.float64)
    assert lib.vt_volume_extract_dot(None, 1, m32.ctypes.data, t.ctypes.data, t.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_extract_dot_f64(None, 1, m64.ctypes.data, t.ctypes.data, t.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_extract_dot_f64(None, 1, m64.ctypes.data, t.ctypes.data, None, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_extract_dot', 'vt_volume_extract_dot_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 10
    assert '14 per-box template scores' in header                   # the last_kernel comment names the new kernel
    assert '13 weighted sum of extracted boxes' in header
