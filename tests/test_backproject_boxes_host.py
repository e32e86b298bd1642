"""StaticVolume.backproject_boxes without a GPU: the device='cpu' path box by box against the float64 model of tests/backproject_model.py
and bit for bit against the CPU backproject, utils.backproject_box_matrices against its formula and against crops of the full
back-projection, argument errors, library codes and symbols."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import backproject_model as bm
from test_backproject_host import STACK, INTERPS, OUT_IN, MARGIN, W5, PLANES, interior_matrices, cpu_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
NB = 3


@pytest.fixture(scope='module')
def stack():
    s = np.random.RandomState(11).random_sample(STACK).astype(np.float32)
    s.setflags(write=False)
    return s


def box_batch():
    """(NB, 5, 4, 4) float64: interior_matrices, the same in reverse order and rolled by two, so every box pairs the images with other
    matrices and every footprint keeps its MARGIN."""
    ms = interior_matrices()
    return np.ascontiguousarray(np.stack([ms, ms[::-1], np.roll(ms, 2, axis=0)]))


def box_weights():
    return np.stack([W5, W5[::-1], np.array([1.0, 0.25, -0.5, 2.0, -1.0])])


# ---- the CPU device path -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
def test_cpu_device_path_against_the_model_and_the_cpu_backproject(interp, stack):
    ms, w = box_batch(), box_weights()
    H, W = STACK[1:]
    for m in ms.reshape(-1, 4, 4):
        y, x = bm.coords(m, OUT_IN)
        assert y.min() >= MARGIN and y.max() <= H - 1 - MARGIN and x.min() >= MARGIN and x.max() <= W - 1 - MARGIN
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    for mats in (ms, ms.astype(np.float32)):
        got = sv.backproject_boxes(mats, OUT_IN, w, planes=PLANES)
        assert got.dtype == np.float32 and got.shape == (NB,) + OUT_IN
        for b in range(NB):
            # the tolerance of test_backproject_host.py's CPU-path test, per box
            want = bm.backproject(stack, mats[b], PLANES, w[b], OUT_IN, interp).astype(np.float64)
            err = float(np.abs(got[b].astype(np.float64) - want).max())
            bound = cpu_bound(interp, w[b], stack)
            print(f'{interp} {mats.dtype} box {b}: max|cpu - model| {err:.3e}  bound {bound:.3e}')
            assert err <= bound, (interp, b, err)
            # bit for bit the CPU backproject of that box's matrices
            assert np.array_equal(got[b].view(np.uint32), sv.backproject(mats[b], OUT_IN, w[b], planes=PLANES).view(np.uint32))
    # weights (n,) are used for every box; None = ones; planes=None: image i belongs to entry i
    got = sv.backproject_boxes(ms, OUT_IN, W5, planes=PLANES)
    for b in range(NB):
        assert np.array_equal(got[b], sv.backproject(ms[b], OUT_IN, W5, planes=PLANES))
    got = sv.backproject_boxes(ms, OUT_IN)
    for b in range(NB):
        assert np.array_equal(got[b], sv.backproject(ms[b], OUT_IN))
    # accumulate starts from the output, per box; without it the output's contents do not count
    base = np.random.RandomState(2).standard_normal((NB,) + OUT_IN).astype(np.float32)
    out = base.copy()
    assert sv.backproject_boxes(ms, OUT_IN, w, output=out, planes=PLANES, accumulate=True) is out
    for b in range(NB):
        ref = base[b].copy()
        sv.backproject(ms[b], OUT_IN, w[b], output=ref, planes=PLANES, accumulate=True)
        assert np.array_equal(out[b], ref) and not np.array_equal(out[b], base[b])
    out2 = base.copy()
    sv.backproject_boxes(ms, OUT_IN, w, output=out2, planes=PLANES)
    assert np.array_equal(out2, sv.backproject_boxes(ms, OUT_IN, w, planes=PLANES))
    # one box
    assert np.array_equal(sv.backproject_boxes(ms[1:2], OUT_IN, w[1:2], planes=PLANES)[0], sv.backproject(ms[1], OUT_IN, w[1], planes=PLANES))


# ---- the matrices --------------------------------------------------------------------------------------------------------------
ANGLES5 = (-40.0, -17.5, 3.0, 21.0, 38.0)
VOLUME = (16, 30, 36)
BOX = (6, 8, 10)


@pytest.mark.parametrize('axis', [0, 1, 2])
def test_backproject_box_matrices_shape_and_formula(axis):
    pos = np.array([[7.5, 14.5, 17.5], [3.25, 9.0, 30.125], [12.0, 20.75, 4.5], [0.0, 0.0, 0.0]])
    for image, center in ((None, None), ((40, 52), None), ((5, 40, 52), (3.0, 10.5, 7.25))):
        got = vt.utils.backproject_box_matrices(pos, ANGLES5, axis, VOLUME, BOX, image, 'deg', center)
        assert got.shape == (4, 5, 4, 4) and got.dtype == np.float64
        full = vt.utils.backproject_matrices(ANGLES5, axis, VOLUME, image, 'deg', center)
        c = (np.asarray(BOX, np.float64) - 1.0) / 2.0
        for b in range(4):
            for i in range(5):
                assert np.array_equal(got[b, i, :3, :3], full[i, :3, :3])
                assert np.array_equal(got[b, i, 3], [0.0, 0.0, 0.0, 1.0])
                # a direct float64 evaluation; the two differ by the order of three additions at most
                want = full[i, :3, 3] + sum(full[i, :3, k] * (pos[b, k] - c[k]) for k in range(3))
                assert np.abs(got[b, i, :3, 3] - want).max() <= 8 * np.finfo(np.float64).eps * (np.abs(full[i, :3]).sum() * 40.0)
        # voxel v of box b is voxel v + positions[b] - c of the volume
        v = np.array([2.0, 5.0, 7.0, 1.0])
        for b in range(4):
            u = np.append(v[:3] + pos[b] - c, 1.0)
            assert np.abs(got[b] @ v - full @ u).max() <= 1e-11
    rad = vt.utils.backproject_box_matrices(pos, np.deg2rad(ANGLES5), axis, VOLUME, BOX, None, 'rad')
    assert np.abs(rad - vt.utils.backproject_box_matrices(pos, ANGLES5, axis, VOLUME, BOX)).max() <= 1e-12


def test_backproject_box_matrices_errors():
    pos = np.zeros((2, 3))
    for bad in (np.zeros(3), np.zeros((2, 2)), np.zeros((0, 3)), np.zeros((1, 2, 3))):
        with pytest.raises(ValueError):
            vt.utils.backproject_box_matrices(bad, ANGLES5, 1, VOLUME, BOX)
    for vol, box in ((None, BOX), (VOLUME, None), ((16, 30), BOX), (VOLUME, (6, 0, 10)), (VOLUME, (6, 8, 10.0))):
        with pytest.raises(ValueError):
            vt.utils.backproject_box_matrices(pos, ANGLES5, 1, vol, box)
    with pytest.raises(ValueError):
        vt.utils.backproject_box_matrices(pos, [], 1, VOLUME, BOX)
    with pytest.raises(ValueError):
        vt.utils.backproject_box_matrices(pos, ANGLES5, 3, VOLUME, BOX)
    with pytest.raises(ValueError):
        vt.utils.backproject_box_matrices(pos, ANGLES5, 1, VOLUME, BOX, (40,))


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_cpu_boxes_are_crops_of_the_full_backprojection(interp, stack):
    """positions - c integer: voxel v of box b is voxel v + o_b of the volume in exact arithmetic; in float64 the two coordinates differ
    by a few ulps, which moves a value by far less than the tolerance unless a voxel sits on the skirt, where it would flip between a
    value and 0.  The angles keep every voxel of the volume at least 1e-9 from the skirt (asserted on the model's coordinates)."""
    angles = (-40.0, -17.5, 3.0, 21.0, 38.0)
    volume = (16, 44, 60)                  # larger than the 40 x 52 images: the first and last boxes hold voxels outside the skirt
    ms_full = vt.utils.backproject_matrices(angles, 1, volume, STACK[1:])
    H, W = STACK[1:]
    partly_outside = False
    for m in ms_full:
        y, x = bm.coords(m, volume)
        for s, n in ((y, H), (x, W)):
            assert np.abs(s + 0.5).min() > 1e-9 and np.abs(s - (n - 0.5)).min() > 1e-9
        ins = bm.inside(y, x, H, W)
        partly_outside = partly_outside or (ins.any() and not ins.all())
    assert partly_outside
    offs = np.array([[0, 0, 0], [5, 11, 13], [3, 7, 20], [10, 36, 50]])
    c = (np.asarray(BOX, np.float64) - 1.0) / 2.0
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    w = np.array([1.0, -0.5, 0.75, 2.0, 1.25])
    full = sv.backproject_tilts(angles, output_shape=volume, weights=w)
    got = sv.backproject_boxes_at(offs + c, angles, 1, volume, BOX, weights=w)
    assert got.shape == (4,) + BOX and full.any()
    assert np.array_equal(got, sv.backproject_boxes(vt.utils.backproject_box_matrices(offs + c, angles, 1, volume, BOX, STACK[1:]), BOX, w))
    bound = cpu_bound(interp, w, stack)    # the tolerance of test_backproject_host.py's CPU-path test
    for b, o in enumerate(offs):
        crop = full[o[0]:o[0] + BOX[0], o[1]:o[1] + BOX[1], o[2]:o[2] + BOX[2]]
        assert crop.shape == BOX
        err = float(np.abs(got[b].astype(np.float64) - crop).max())
        print(f'{interp} box {b}: max|box - crop| {err:.3e}  bound {bound:.3e}')
        assert err <= bound, (interp, b, err)
    assert (got[0] == 0).any() and (got[0] != 0).any() and got[1].all()
    with pytest.raises(ValueError):
        sv.backproject_boxes_at(offs + c, angles, 1, None, BOX)
    with pytest.raises(ValueError):
        sv.backproject_boxes_at(offs + c, angles, 1, volume)


# ---- argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors(stack):
    sv = vt.StaticVolume(stack, device='cpu')
    ms, w = box_batch(), box_weights()
    for bad in (np.eye(4), interior_matrices(), np.zeros((0, 5, 4, 4)), np.zeros((2, 0, 4, 4)), np.zeros((2, 5, 3, 4)),
                np.zeros((1, 2, 5, 4, 4))):
        with pytest.raises(ValueError):
            sv.backproject_boxes(bad, OUT_IN)
    for bad in (W5[:4], np.ones((NB, 4)), np.ones((NB + 1, 5)), np.ones((5, NB)), np.ones((NB, 5, 1)), np.ones(NB)):
        with pytest.raises(ValueError):
            sv.backproject_boxes(ms, OUT_IN, bad)
    for bad in (np.nan, np.inf):
        wb = w.copy()
        wb[1, 2] = bad
        with pytest.raises(ValueError):
            sv.backproject_boxes(ms, OUT_IN, wb)
    with pytest.raises(ValueError):
        sv.backproject_boxes(ms[:, :3], OUT_IN)                                                  # planes=None with n != T
    for bad in ([0, 1, 2, 3, 5], [0, 1, 2, 3, -1], [0, 1, 2, 3], [0.0, 1.0, 2.0, 3.0, 4.0], [[0, 1, 2, 3, 4]] * NB):
        with pytest.raises(ValueError):
            sv.backproject_boxes(ms, OUT_IN, planes=bad)
    for bad in (np.zeros(OUT_IN, np.float32), np.zeros((NB, 6, 8, 13), np.float32), np.zeros((NB + 1,) + OUT_IN, np.float32)):
        with pytest.raises(ValueError):
            sv.backproject_boxes(ms, OUT_IN, output=bad)
    for shape in ((6, 0, 12), (6, 8), (6, 8, 12.0), None):
        with pytest.raises(ValueError):
            sv.backproject_boxes(ms, shape)
    with pytest.raises(ValueError):
        sv.backproject_boxes(ms, OUT_IN, w, accumulate=True)                                     # nothing to add into
    with pytest.raises(ValueError):
        sv.backproject_boxes_at(np.zeros((2, 3)), (0.0,) * 5, 1, (8, 8, 8), (4, 4, 4), accumulate=True)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            sv.backproject_boxes(ms, OUT_IN, _max_table_bytes=bad)
    # prefiltered coefficients that mix the images are refused
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, 'filt_bspline', 'cpu').backproject_boxes(ms, OUT_IN)
    assert vt.StaticVolume(stack, 'filt_bspline', 'cpu', stack=True).backproject_boxes(ms, OUT_IN).any()


# ---- the library without a GPU --------------------------------------------------------------------------------------------------
def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.zeros((2, 1, 4, 4), np.float32)
    m64 = np.zeros((2, 1, 4, 4), np.float64)
    w = np.ones(2)
    pl = np.zeros(1, np.int32)
    out = np.zeros((2, 4, 4, 4), np.float32)
    assert lib.vt_volume_backproject_boxes(None, 2, 1, m32.ctypes.data, pl.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_backproject_boxes_f64(None, 2, 1, m64.ctypes.data, pl.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_backproject_boxes_f64(None, 2, 1, m64.ctypes.data, None, None, 4, 4, 4, out.ctypes.data, _native.ACCUMULATE) == VT_EINVAL
    assert lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_backproject_boxes', 'vt_volume_backproject_boxes_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 11
    assert '19 nb boxes of one shape back-projected from one stack' in header      # the last_kernel comment names the new kernel
    assert 'backproject_box_matrices' in dir(vt.utils)
