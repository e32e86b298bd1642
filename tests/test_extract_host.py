"""StaticVolume.extract / extract_at / utils.box_matrices without a GPU: the CPU device against scipy's own output_shape
(the reference's CPU call site, transforms.py:136-150), the matrix builder against its formula, argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.ndimage import affine_transform

import voltools_amd as vt
from voltools_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001


def _boxes(shape, box):
    """One box inside, one straddling a corner, one entirely outside (float32 matrices)."""
    centre = (np.asarray(shape, np.float64) - 1) / 2
    ms = vt.utils.box_matrices([centre + (0.3, -0.4, 0.25), (0.5, 1.0, 0.25), np.asarray(shape) + 40.0],
                               [(10, 45, -20), (25, -40, 70), (5, 5, 5)], box)
    return np.ascontiguousarray(ms, dtype=np.float32)


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_cpu_extract_is_scipy_output_shape_per_matrix(interp, golden_volume):
    box = (8, 9, 10)
    ms = _boxes(golden_volume.shape, box)
    sv = vt.StaticVolume(golden_volume, interpolation=interp, device='cpu')
    got = sv.extract(ms, box)
    assert got.shape == (3,) + box and got.dtype == np.float32
    order = 1 if interp == 'linear' else 3
    for i in range(3):
        want = affine_transform(golden_volume, ms[i], output_shape=box, order=order, prefilter=interp.startswith('filt_bspline'))
        assert np.array_equal(got[i], want), (interp, i)
    assert np.abs(got[0]).max() > 0.1 and np.abs(got[1]).max() > 0.1
    assert not got[2].any()                        # entirely outside
    assert (got[1] == 0).any()                     # the corner box hangs over the volume
    out = np.full((3,) + box, 7, np.float32)
    assert sv.extract(ms, box, output=out) is out and np.array_equal(out, got)


@pytest.mark.parametrize('units', ['deg', 'rad'])
@pytest.mark.parametrize('order', ['rzxz', 'sxyz'])
def test_box_matrices_formula(units, order):
    box = (9, 12, 16)
    pos = np.array([[10.25, 20.5, 30.75], [0, 0, 0], [-3.5, 100.0, 7.0]])
    rot = np.array([[10, 45, -20], [0, 0, 90], [123, -45, 6]], dtype=np.float64)
    if units == 'rad':
        rot = np.deg2rad(rot)
    ms = vt.utils.box_matrices(pos, rot, box, rotation_units=units, rotation_order=order)
    assert ms.shape == (3, 4, 4) and ms.dtype == np.float64
    c = np.array([4.0, 5.5, 7.5])
    for i in range(3):
        r3 = vt.utils.rotation_matrix(rot[i], units, order, dtype=np.float64)[:3, :3]
        want = np.zeros((4, 4))
        want[:3, :3] = r3
        for r in range(3):
            want[r, 3] = pos[i, r] - (r3[r, 0] * c[0] + r3[r, 1] * c[1] + r3[r, 2] * c[2])
        want[3, 3] = 1.0
        assert np.abs(ms[i] - want).max() <= 1e-13, (i, ms[i], want)
        # the box centre samples the source at the position
        assert np.abs(ms[i, :3, :3] @ c + ms[i, :3, 3] - pos[i]).max() <= 1e-12


def test_box_matrices_without_rotation_and_plain_crop(golden_volume):
    box = (6, 7, 8)
    c = (np.asarray(box) - 1) / 2
    starts = np.array([[3, 4, 5], [-2, 20, 25], [17, -3, 0]])
    ms = vt.utils.box_matrices(starts + c, None, box)
    for i in range(3):
        assert np.array_equal(ms[i, :3, :3], np.eye(3)) and np.array_equal(ms[i, :3, 3], starts[i].astype(np.float64))
        assert np.array_equal(ms[i, 3], [0, 0, 0, 1])
    sv = vt.StaticVolume(golden_volume, interpolation='linear', device='cpu')
    got = sv.extract_at(starts + c, box_shape=box)
    pad = 8
    padded = np.pad(golden_volume, pad, mode='constant')
    for i in range(3):
        z, y, x = starts[i] + pad
        assert np.array_equal(got[i], padded[z:z + box[0], y:y + box[1], x:x + box[2]]), i


def test_argument_errors(golden_volume):
    sv = vt.StaticVolume(golden_volume, device='cpu')
    eye = np.eye(4, dtype=np.float32)[None]
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.extract(bad, (4, 4, 4))
    for bad_box in ((4, 4), (4, 0, 4), (4, -1, 4), (4.0, 4, 4), 4, None):
        with pytest.raises(ValueError):
            sv.extract(eye, bad_box)
    with pytest.raises(ValueError):
        sv.extract(eye, (4, 4, 4), output=np.zeros((1, 4, 4, 5), np.float32))
    with pytest.raises(ValueError):
        sv.extract_at([[1, 2, 3], [4, 5, 6]], [[0, 0, 0]], (4, 4, 4))
    with pytest.raises(ValueError):
        sv.extract_at([[1, 2, 3]], [[0, 0, 0], [1, 1, 1]], (4, 4, 4))
    with pytest.raises(ValueError):
        vt.utils.box_matrices([1, 2, 3], None, (4, 4, 4))


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    out = np.zeros((4, 4, 4), np.float32)
    assert lib.vt_volume_extract(None, 1, m32.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_extract_f64(None, 1, m64.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    for box in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
        assert lib.vt_volume_extract(None, 1, m32.ctypes.data, *box, out.ctypes.data, 0) == VT_EINVAL
        assert lib.vt_volume_extract_f64(None, 1, m64.ctypes.data, *box, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_extract', 'vt_volume_extract_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 8
    assert 'transforms.py:136-150' in header and '11 batched box extraction' in header
