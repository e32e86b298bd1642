"""StaticVolume.extract_sum / average_at without a GPU: the CPU device against the weighted float64 sum of its own extract,
argument errors, and the C entry points' argument codes."""
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
W = np.array([0.5, -1.25, 2.0, 1.0, 0.75])


@pytest.fixture(scope='module')
def vol():
    return np.random.RandomState(51).random_sample(SHAPE).astype(np.float32)


def _matrices():
    return vt.utils.box_matrices(POS, ROT, BOX)


def _weighted(boxes, w):
    return (w[:, None, None, None] * boxes.astype(np.float64)).sum(0).astype(np.float32)


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_sum_equals_weighted_sum_of_extract(interp, vol):
    ms = _matrices()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    boxes = sv.extract(ms, BOX)
    assert (boxes[3] == 0).any() and boxes[3].any()              # the box over the face is cut, not empty
    got = sv.extract_sum(ms, BOX, W)
    assert got.shape == BOX and got.dtype == np.float32
    want = _weighted(boxes, W)
    assert np.abs(want).max() > 0.5
    assert np.array_equal(got, want), (interp, float(np.abs(got - want).max()))
    out = np.full(BOX, 7, np.float32)
    assert sv.extract_sum(ms, BOX, W, output=out) is out and np.array_equal(out, got)


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_no_weights_means_ones(interp, vol):
    ms = _matrices()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.extract_sum(ms, BOX)
    assert np.array_equal(got, sv.extract_sum(ms, BOX, np.ones(len(ms))))
    assert np.array_equal(got, _weighted(sv.extract(ms, BOX), np.ones(len(ms))))
    assert np.array_equal(got, sv.extract_sum(ms, BOX, [1, 1, 1, 1, 1]))          # anything that converts to float64


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_average_at_is_extract_sum_with_normalised_weights(interp, vol):
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.average_at(POS, ROT, BOX, W)
    assert np.array_equal(got, sv.extract_sum(_matrices(), BOX, W / W.sum()))
    assert np.array_equal(sv.average_at(POS, ROT, BOX), sv.extract_sum(_matrices(), BOX, np.full(5, 1.0) / 5.0))
    plain = sv.average_at(POS, None, BOX, rotation_order='sxyz')
    assert np.array_equal(plain, sv.extract_sum(vt.utils.box_matrices(POS, None, BOX), BOX, np.full(5, 0.2)))


def test_argument_errors(vol):
    sv = vt.StaticVolume(vol, device='cpu')
    ms = _matrices()
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.extract_sum(bad, BOX)
    with pytest.raises(ValueError):
        sv.extract_sum(ms, BOX, W[:4])
    with pytest.raises(ValueError):
        sv.extract_sum(ms, BOX, np.ones((5, 1)))
    nan = W.copy()
    nan[2] = np.nan
    with pytest.raises(ValueError):
        sv.extract_sum(ms, BOX, nan)
    with pytest.raises(ValueError):
        sv.average_at(POS, ROT, BOX, nan)
    with pytest.raises(ValueError):
        sv.average_at(POS, ROT, BOX, [1.0, -1.0, 2.0, -2.0, 0.0])
    with pytest.raises(ValueError):
        sv.average_at(POS, ROT, BOX, W[:4])
    with pytest.raises(ValueError):
        sv.extract_sum(ms, BOX, W, output=np.zeros((9, 13, 12), np.float32))
    with pytest.raises(ValueError):
        sv.extract_sum(ms, BOX, W, output=np.zeros((5,) + BOX, np.float32))
    with pytest.raises(ValueError):
        sv.extract_sum(ms, (9, 0, 11))


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    w = np.ones(1)
    out = np.zeros((4, 4, 4), np.float32)
    assert lib.vt_volume_extract_sum(None, 1, m32.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_extract_sum_f64(None, 1, m64.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_extract_sum_f64(None, 1, m64.ctypes.data, None, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_extract_sum', 'vt_volume_extract_sum_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 9
    assert '13 weighted sum of extracted boxes' in header           # the last_kernel comment names the new kernel
