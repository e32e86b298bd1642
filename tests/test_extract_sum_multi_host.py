"""StaticVolume.extract_sum_multi / class_averages_at without a GPU: the CPU device against extract_sum and average_at column by column,
argument errors, and the C entry points' declarations and argument codes."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
SHAPE = (20, 22, 24)
BOX = (7, 9, 11)
N, G = 6, 3
POS = np.array([[9.5, 10.25, 12.0], [6.0, 14.5, 8.75], [12.25, 9.0, 15.5], [10.0, 11.0, 22.5], [8.5, 12.5, 10.5],
                [11.0, 8.0, 9.25]])                                    # the fourth hangs over a face
ROT = np.array([[10.0, 20.0, 30.0], [0.0, 0.0, 0.0], [-40.0, 15.0, 80.0], [5.0, -10.0, 20.0], [90.0, 45.0, -30.0], [33.0, 66.0, 99.0]])


@pytest.fixture(scope='module')
def vol():
    return np.random.RandomState(61).random_sample(SHAPE).astype(np.float32)


def _matrices():
    return vt.utils.box_matrices(POS, ROT, BOX)


def _weights():
    w = np.random.RandomState(63).uniform(-1, 2, (N, G))
    w[2] = 0            # a matrix no column uses
    w[4, 1] = 0
    return w


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_columns_equal_extract_sum(interp, vol):
    ms, w = _matrices(), _weights()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.extract_sum_multi(ms, BOX, w)
    assert got.shape == (G,) + BOX and got.dtype == np.float32 and got.any()
    for j in range(G):
        assert np.array_equal(got[j], sv.extract_sum(ms, BOX, w[:, j])), (interp, j)
    # a column does not depend on the others, on G or on its place
    assert np.array_equal(sv.extract_sum_multi(ms, BOX, w[:, [2, 0]]), got[[2, 0]])
    assert np.array_equal(sv.extract_sum_multi(ms, BOX, w[:, 1:2]), got[1:2])
    assert np.array_equal(sv.extract_sum_multi(ms, BOX, w.astype(np.float32).astype(np.float64).tolist()),
                          sv.extract_sum_multi(ms, BOX, w.astype(np.float32)))              # anything that converts to float64


def test_cpu_output_is_filled_and_returned(vol):
    ms, w = _matrices(), _weights()
    sv = vt.StaticVolume(vol, device='cpu')
    want = sv.extract_sum_multi(ms, BOX, w)
    out = np.full((G,) + BOX, 7, np.float32)
    assert sv.extract_sum_multi(ms, BOX, w, output=out) is out and np.array_equal(out, want)
    one = np.full(BOX, 7, np.float32)
    assert sv.extract_sum(ms, BOX, w[:, 0], output=one) is one and np.array_equal(one, want[0])     # as extract_sum does


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_class_averages_at(interp, vol):
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    labels = np.array([0, 2, 0, 1, 2, 2])
    got = sv.class_averages_at(POS, ROT, BOX, labels=labels)
    assert got.shape == (3,) + BOX and got.dtype == np.float32
    for c in range(3):
        sel = labels == c
        # the CPU device adds the boxes one after the other: the members meet the weight 1 / n_c in the same order, the others add 0 * box
        assert np.array_equal(got[c], sv.average_at(POS[sel], ROT[sel], BOX)), (interp, c)
    # an empty class is a zero box, not an error; n_classes may exceed max + 1
    wide = sv.class_averages_at(POS, ROT, BOX, labels=labels, n_classes=5)
    assert wide.shape == (5,) + BOX and np.array_equal(wide[:3], got) and not wide[3:].any()
    gap = sv.class_averages_at(POS, ROT, BOX, labels=np.array([0, 2, 0, 2, 2, 2]))
    assert gap.shape == (3,) + BOX and gap[0].any() and gap[2].any() and not gap[1].any()
    # soft weights: every column divided by its sum, a column of zeros stays zero
    w = np.abs(_weights())
    w[:, 1] = 0
    soft = sv.class_averages_at(POS, ROT, BOX, weights=w)
    assert soft.shape == (G,) + BOX and not soft[1].any()
    for j in (0, 2):
        assert np.array_equal(soft[j], sv.average_at(POS, ROT, BOX, weights=w[:, j])), (interp, j)
    assert np.array_equal(w[:, 1], np.zeros(N)) and w[:, 0].sum() != 1.0             # the caller's array is not normalised in place
    # one class holding every box is average_at, bit for bit
    same = sv.class_averages_at(POS, ROT, BOX, labels=np.zeros(N, int), n_classes=1)
    assert np.array_equal(same, sv.average_at(POS, ROT, BOX)[None])
    out = np.full((3,) + BOX, 7, np.float32)
    assert sv.class_averages_at(POS, ROT, BOX, labels=labels, output=out) is out and np.array_equal(out, got)


def test_argument_errors(vol):
    sv = vt.StaticVolume(vol, device='cpu')
    ms, w = _matrices(), _weights()
    for bad in (w[:, 0], np.zeros((N + 1, G)), np.zeros((N, 0)), w[None]):
        with pytest.raises(ValueError):
            sv.extract_sum_multi(ms, BOX, bad)
    for bad_value in (np.nan, np.inf):
        bad = w.copy()
        bad[3, 1] = bad_value
        with pytest.raises(ValueError):
            sv.extract_sum_multi(ms, BOX, bad)
        with pytest.raises(ValueError):
            sv.class_averages_at(POS, ROT, BOX, weights=bad)
    for bad in (np.zeros(BOX, np.float32), np.zeros((G + 1,) + BOX, np.float32), np.zeros((G, 7, 9, 12), np.float32)):
        with pytest.raises(ValueError):
            sv.extract_sum_multi(ms, BOX, w, output=bad)
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.extract_sum_multi(bad, BOX, w)
    labels = np.array([0, 1, 0, 1, 2, 2])
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX)                                  # neither
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, labels=labels, weights=w)        # both
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, labels=labels, n_classes=2)      # a label beyond the classes
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, labels=labels - 1)               # a negative label
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, labels=labels[:-1])
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, labels=labels.astype(np.float64))
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, weights=w[:, 0])
    with pytest.raises(ValueError):
        sv.class_averages_at(POS, ROT, BOX, labels=labels, output=np.zeros((2,) + BOX, np.float32))


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    w = np.ones((1, 2))
    out = np.zeros((2, 4, 4, 4), np.float32)
    assert lib.vt_volume_extract_sum_multi(None, 1, m32.ctypes.data, 2, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()
    assert lib.vt_volume_extract_sum_multi_f64(None, 1, m64.ctypes.data, 2, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()
    # g <= 0 and NULL weights are refused before the handle is looked at: any non-NULL pointer will do, it is never dereferenced
    fake = out.ctypes.data
    for g in (0, -2):
        assert lib.vt_volume_extract_sum_multi(fake, 1, m32.ctypes.data, g, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
        assert b'column count' in lib.vt_last_error()
        assert lib.vt_volume_extract_sum_multi_f64(fake, 1, m64.ctypes.data, g, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
        assert b'column count' in lib.vt_last_error()
    assert lib.vt_volume_extract_sum_multi(fake, 1, m32.ctypes.data, 2, None, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert b'weights' in lib.vt_last_error()
    assert lib.vt_volume_extract_sum_multi_f64(fake, 0, m64.ctypes.data, 2, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert not out.any()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_extract_sum_multi', 'vt_volume_extract_sum_multi_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 10
    assert '16 g weighted sums of the same extracted boxes' in header    # the last_kernel comment names the new kernel
    assert '13 weighted sum of extracted boxes' in header
