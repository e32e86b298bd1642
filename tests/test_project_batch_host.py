"""StaticVolume.projection_batch / tilt_series / utils.tilt_matrices without a GPU: the CPU device against the existing
single projection and against scipy's own output_shape summed over axis 0, the matrix builder against its definition,
argument errors, and the C entry points' argument codes."""
import os
import re

import numpy as np
import pytest
from scipy.ndimage import affine_transform

import voltools_amd as vt
from voltools_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
SHAPE = (20, 22, 24)


@pytest.fixture(scope='module')
def vol():
    return np.random.RandomState(41).random_sample(SHAPE).astype(np.float32)


def _matrices():
    """A tilt about axis 1, a tilt about axis 2 and a general rotation with scale and shift (float32)."""
    c = np.divide(np.subtract(SHAPE, 1), 2, dtype=np.float32)
    return np.stack([vt.utils.transform_matrix(rotation=(0, 30, 0), rotation_order='sxyz', center=c),
                     vt.utils.transform_matrix(rotation=(0, 0, -45), rotation_order='sxyz', center=c),
                     vt.utils.transform_matrix(rotation=(20, 35, -50), rotation_order='sxyz', scale=(1.1, 0.9, 1.05),
                                               translation=(1.5, -2, 0.25), center=c)])


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_batch_equals_single_projections(interp, vol):
    ms = _matrices()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.projection_batch(ms)
    assert got.shape == (3,) + SHAPE[1:] and got.dtype == np.float32
    want = np.stack([sv.projection(m) for m in ms])
    assert np.abs(want).max() > 1.0
    assert np.array_equal(got, want), (interp, float(np.abs(got - want).max()))
    out = np.full(got.shape, 7, np.float32)
    assert sv.projection_batch(ms, output=out) is out and np.array_equal(out, got)


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_cpu_batch_with_an_output_shape(interp, vol):
    oshape = (9, 13, 30)
    ms = _matrices()
    sv = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    got = sv.projection_batch(ms, output_shape=oshape)
    assert got.shape == (3, 13, 30) and got.dtype == np.float32
    order = 1 if interp == 'linear' else 3
    for i in range(3):
        full = affine_transform(vol, ms[i], output_shape=oshape, order=order, prefilter=interp.startswith('filt_bspline'))
        want = full.sum(axis=0, dtype=np.float64).astype(np.float32)
        assert np.array_equal(got[i], want), (interp, i, float(np.abs(got[i] - want).max()))
    assert (got[0] == 0).any() and got[0].any()          # a 30-wide image hangs over the 24-wide volume


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_tilt_matrices_definition(axis):
    angles = [-60.0, 0.0, 12.5, 60.0]
    c = np.divide(np.subtract(SHAPE, 1), 2, dtype=np.float32)
    ms = vt.utils.tilt_matrices(angles, axis, SHAPE)
    assert ms.shape == (4, 4, 4)
    for i, a in enumerate(angles):
        r = [0.0, 0.0, 0.0]
        r[axis] = a
        want = vt.utils.transform_matrix(rotation=tuple(r), rotation_order='sxyz', center=c)
        assert np.array_equal(ms[i], want), (axis, a)
    # an explicit centre, and radians against degrees
    c2 = (3.0, 4.5, 6.25)
    deg = vt.utils.tilt_matrices(angles, axis, SHAPE, 'deg', c2)
    rad = vt.utils.tilt_matrices(np.deg2rad(angles), axis, SHAPE, 'rad', c2)
    assert np.array_equal(deg[1], vt.utils.transform_matrix(rotation=(0, 0, 0), rotation_order='sxyz', center=c2))
    assert np.abs(deg.astype(np.float64) - rad).max() <= 4e-6       # float32 sines one ulp apart; the translation column (magnitude < 16, ulp 1e-6) collects a few such roundings
    # the turn leaves the tilt axis alone
    assert np.array_equal(ms[0][axis, :3], np.eye(3)[axis]) and np.array_equal(ms[0][:3, axis], np.eye(3)[axis])


def test_tilt_series_is_projection_batch_of_tilt_matrices_and_project(vol):
    sv = vt.StaticVolume(vol, interpolation='linear', device='cpu')
    angles = [-40.0, 25.0]
    for axis in (1, 2):
        got = sv.tilt_series(angles, axis)
        assert np.array_equal(got, sv.projection_batch(vt.utils.tilt_matrices(angles, axis, SHAPE)))
        for i, a in enumerate(angles):
            r = [0.0, 0.0, 0.0]
            r[axis] = a
            assert np.array_equal(got[i], sv.project(rotation=tuple(r), rotation_order='sxyz')), (axis, a)
    assert sv.tilt_series(angles, output_shape=(9, 13, 30)).shape == (2, 13, 30)


def test_argument_errors(vol):
    sv = vt.StaticVolume(vol, device='cpu')
    eye = np.eye(4, dtype=np.float32)[None]
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.projection_batch(bad)
    for bad_shape in ((4, 4), (4, 0, 4), (4, -1, 4), (4.0, 4, 4), 4):
        with pytest.raises(ValueError):
            sv.projection_batch(eye, output_shape=bad_shape)
    with pytest.raises(ValueError):
        sv.projection_batch(eye, output=np.zeros((1,) + SHAPE[1:] + (1,), np.float32))
    with pytest.raises(ValueError):
        sv.projection_batch(eye, output_shape=(4, 5, 6), output=np.zeros((1,) + SHAPE[1:], np.float32))
    for bad_axis in (-1, 3, 1.0, None):
        with pytest.raises(ValueError):
            vt.utils.tilt_matrices([0.0], bad_axis, SHAPE)
        with pytest.raises(ValueError):
            sv.tilt_series([0.0], bad_axis)
    with pytest.raises(ValueError):
        sv.tilt_series([])


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    out = np.zeros((4, 4), np.float32)
    assert lib.vt_volume_project_batch(None, 1, m32.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_project_batch_f64(None, 1, m64.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_project_batch', 'vt_volume_project_batch_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 8
