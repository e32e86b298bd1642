"""StaticVolume.extract_dot_multi / correlate_templates_at without a GPU: the CPU device against the stacked columns of extract_dot and
of correlate_at, argument errors, the shim's float64 outputs, and the C entry points' declarations and argument codes."""
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
K = 5
POS = np.array([[9.5, 10.25, 12.0], [6.0, 14.5, 8.75], [12.25, 9.0, 15.5], [10.0, 11.0, 22.5], [8.5, 12.5, 10.5]])   # the fourth hangs over a face
ROT = np.array([[10.0, 20.0, 30.0], [0.0, 0.0, 0.0], [-40.0, 15.0, 80.0], [5.0, -10.0, 20.0], [90.0, 45.0, -30.0]])


@pytest.fixture(scope='module')
def vol():
    return np.random.RandomState(51).random_sample(SHAPE).astype(np.float32)


def _matrices():
    return vt.utils.box_matrices(POS, ROT, BOX)


def _templates_and_mask():
    rs = np.random.RandomState(53)
    tmpls = rs.uniform(-1, 1, (K,) + BOX).astype(np.float32)
    mask = rs.uniform(0, 1, BOX).astype(np.float32)
    mask[0, 0, 0] = mask[-1, -1, -1] = 0
    return tmpls, mask


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_multi_equals_the_stacked_columns_of_extract_dot(interp, vol):
    ms = _matrices()
    tmpls, mask = _templates_and_mask()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    for m in (mask, None):
        got = sv.extract_dot_multi(ms, tmpls, m)
        assert got.shape == (5, 2 + K) and got.dtype == np.float64 and got.all()
        for j in range(K):
            single = sv.extract_dot(ms, tmpls[j], m)
            assert np.array_equal(got[:, :2], single[:, :2]) and np.array_equal(got[:, 2 + j], single[:, 2]), (interp, j)
    assert np.array_equal(sv.extract_dot_multi(ms, tmpls), sv.extract_dot_multi(ms, tmpls, np.ones(BOX, np.float32)))      # None means ones
    assert np.array_equal(sv.extract_dot_multi(ms, tmpls), sv.extract_dot_multi(ms, tmpls.astype(np.float64), np.ones(BOX, int)))
    out = np.full((5, 2 + K), 7.0)
    assert sv.extract_dot_multi(ms, tmpls, mask, output=out) is out and np.array_equal(out, sv.extract_dot_multi(ms, tmpls, mask))
    one = sv.extract_dot_multi(ms, tmpls[3:4], mask)                     # a stack of one
    assert one.shape == (5, 3) and np.array_equal(one, sv.extract_dot(ms, tmpls[3], mask))


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_correlate_templates_at_equals_correlate_at_per_column(interp, vol):
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    templates = sv.extract_at(POS[:3], ROT[:3], BOX)
    _, mask = _templates_and_mask()
    for m in (None, mask):
        cc = sv.correlate_templates_at(POS, ROT, templates, m)
        assert cc.shape == (5, 3) and cc.dtype == np.float64
        for j in range(3):
            assert np.array_equal(cc[:, j], sv.correlate_at(POS, ROT, templates[j], m)), (interp, j)
        assert np.argmax(cc[:3], axis=1).tolist() == [0, 1, 2] and (np.abs(np.diag(cc[:3]) - 1.0) <= 1e-6).all(), (interp, cc)
    flat = vt.StaticVolume(np.zeros(SHAPE, np.float32), interpolation=interp, device='cpu')
    assert np.array_equal(flat.correlate_templates_at(POS, ROT, templates, mask), np.zeros((5, 3)))      # no variance: 0, not NaN


def test_argument_errors(vol):
    sv = vt.StaticVolume(vol, device='cpu')
    ms = _matrices()
    tmpls, mask = _templates_and_mask()
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls[0])                               # a 3-D template is not a stack
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls[None])                            # 5-D
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls[:0])                              # an empty stack
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, mask[:, :, :-1])                 # mask of another shape
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, np.stack([mask] * K))            # per-template masks are not built
    nan = tmpls.copy()
    nan[4, 1, 2, 3] = np.nan
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, nan, mask)
    inf = mask.copy()
    inf[1, 2, 3] = np.inf
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, inf)
    for bad in (np.zeros((5, 2 + K), np.float32), np.zeros((5, 3), np.float64), np.zeros((4, 2 + K), np.float64)):
        with pytest.raises(ValueError):
            sv.extract_dot_multi(ms, tmpls, mask, output=bad)
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.extract_dot_multi(bad, tmpls)
    with pytest.raises(ValueError):
        sv.correlate_templates_at(POS, ROT, tmpls, np.zeros(BOX, np.float32))       # N = 0
    flat = tmpls.copy()
    flat[2] = 2.0
    with pytest.raises(ValueError):
        sv.correlate_templates_at(POS, ROT, flat, mask)                  # sigma_t = 0 for one template
    with pytest.raises(ValueError):
        sv.correlate_templates_at(POS, ROT, nan, mask)
    with pytest.raises(ValueError):
        sv.correlate_templates_at(POS, ROT, tmpls[0], mask)              # not a stack
    with pytest.raises(ValueError):
        sv.correlate_templates_at(POS, ROT)
    # the single-template calls still refuse a stack
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpls)
    with pytest.raises(ValueError):
        sv.correlate_at(POS, ROT, tmpls, mask)


def test_float64_outputs_are_checked_by_the_shim():
    shape = (5, 2 + K)
    out = np.zeros(shape, np.float64)
    ptr, is_dev, arr = _native.resolve_output(out, shape, 0, dtype=np.float64)
    assert ptr == out.ctypes.data and not is_dev and arr is out
    for bad in (np.zeros(shape, np.float32), np.zeros(shape[::-1], np.float64).T, np.zeros((5, 3), np.float64)):
        with pytest.raises(ValueError):
            _native.resolve_output(bad, shape, 0, dtype=np.float64)

    class Dev:                                                           # what vt.empty arrays expose: float32
        __cuda_array_interface__ = {'shape': shape, 'typestr': '<f4', 'data': (4096, False), 'version': 2, 'strides': None}

    with pytest.raises(ValueError):
        _native.resolve_output(Dev(), shape, 0, dtype=np.float64)
    Dev.__cuda_array_interface__ = dict(Dev.__cuda_array_interface__, typestr='<f8')
    assert _native.resolve_output(Dev(), shape, 0, dtype=np.float64) == (4096, True, None)


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    t = np.ones((2, 4, 4, 4), np.float32)
    out = np.zeros((1, 4), np.float64)
    assert lib.vt_volume_extract_dot_multi(None, 1, m32.ctypes.data, 2, t.ctypes.data, t.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_extract_dot_multi_f64(None, 1, m64.ctypes.data, 2, t.ctypes.data, None, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()
    # k = 0 is refused before the handle is looked at: any non-NULL pointer will do, it is never dereferenced
    fake = out.ctypes.data
    for k in (0, -2):
        assert lib.vt_volume_extract_dot_multi(fake, 1, m32.ctypes.data, k, t.ctypes.data, None, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
        assert b'template count' in lib.vt_last_error()
        assert lib.vt_volume_extract_dot_multi_f64(fake, 1, m64.ctypes.data, k, t.ctypes.data, None, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
        assert b'template count' in lib.vt_last_error()
    assert not out.any()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_extract_dot_multi', 'vt_volume_extract_dot_multi_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 11
    assert '15 per-box scores against k templates' in header             # the last_kernel comment names the new kernel
    assert '14 per-box template scores' in header
