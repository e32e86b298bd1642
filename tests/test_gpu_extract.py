"""-m gpu: StaticVolume.extract (vt_volume_extract, kernel 11) against the oracle's generalised entry point with
out_shape = box, on EVERY voxel of every box (no mask), tolerances of test_gpu_parity.py."""
import ctypes

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = {'linear': 1e-6, 'bspline': 1e-6, 'bspline_simple': 1e-6, 'filt_bspline': 3e-6, 'filt_bspline_simple': 3e-6}
TOL_EDGE = {'linear': 1e-6, 'bspline': 2e-6, 'filt_bspline': 1e-5}       # tests/test_gpu_edge_scipy.py
ALL_INTERPS = list(TOL)
VT_EINVAL = 10001
BOXES = [(32, 32, 32), (17, 23, 29), (40, 48, 56), (96, 96, 96)]


def routed_to_kernel_11(interp, box):
    """The committed default routing rule (vt_api.hip: extract_routes_tiled)."""
    return True


def rand_vol(shape, seed=0):
    return np.random.RandomState(seed).random_sample(shape).astype(np.float32)


def centred(m3, pos, box):
    """4x4 float64 pull matrix with linear part m3 whose box centre samples the source at pos."""
    c = (np.asarray(box, np.float64) - 1) / 2
    m = np.eye(4)
    m[:3, :3] = m3
    m[:3, 3] = np.asarray(pos, np.float64) - np.asarray(m3, np.float64) @ c
    return m


def rot3(angles, order='sxyz'):
    return vt.utils.rotation_matrix(angles, 'deg', order, dtype=np.float64)[:3, :3]


def batch(shape, box, seed=3):
    """>= 24 float32 matrices: random rotations at fractional positions, a box over each face and one corner, one entirely
    outside, scale 2 and 0.5, a mirror, a shear, identity at an integer position."""
    rs = np.random.RandomState(seed)
    s = np.asarray(shape, np.float64)
    ms = []
    for _ in range(11):
        ms.append(centred(rot3(rs.uniform(0, 360, 3)), rs.uniform(0.15, 0.85, 3) * s, box))
    mid = (s - 1) / 2
    for axis in range(3):
        for end in (0.0, s[axis] - 1):
            pos = mid + rs.uniform(-3, 3, 3)
            pos[axis] = end + rs.uniform(-0.5, 0.5)
            ms.append(centred(rot3(rs.uniform(-30, 30, 3)), pos, box))
    ms.append(centred(rot3((20, 35, -50)), (0.25, -0.5, 0.75), box))                      # corner
    ms.append(centred(rot3((10, 20, 30)), s + 2.0 * np.asarray(box) + 5.0, box))          # entirely outside
    ms.append(centred(2.0 * rot3((15, -25, 40)), mid + 0.3, box))                          # scale 2 (minification)
    ms.append(centred(0.5 * rot3((-35, 10, 60)), mid - 0.7, box))                          # scale 0.5
    ms.append(centred(np.diag([-1.0, 1.0, -1.0]), mid + (0.5, 0.25, -0.25), box))         # mirror
    sh = np.eye(3)
    sh[0, 1], sh[0, 2], sh[1, 2] = 0.2, -0.15, 0.3
    ms.append(centred(sh, mid + 0.4, box))                                                 # shear
    ident = np.eye(4)
    ident[:3, 3] = np.floor(mid / 2)
    ms.append(ident)                                                                       # identity at an integer position
    assert len(ms) >= 24
    return np.ascontiguousarray(np.stack(ms), dtype=np.float32)


def oracle_boxes(vol, ms, interp, box):
    src = oracle.prefilter(vol) if interp.startswith('filt') else vol
    okind = interp[5:] if interp.startswith('filt') else interp
    return np.stack([oracle.affine_ex(src, np.asarray(m, np.float64), okind, box) for m in ms])


def check(got, want, tol, what):
    assert got.shape == want.shape, what
    err = np.abs(got.astype(np.float64) - want).reshape(got.shape[0], -1).max(axis=1)
    print(what, 'max|hip-oracle| per box:', ' '.join(f'{e:.2e}' for e in err))
    assert np.isfinite(got).all(), what
    assert err.max() <= tol, (what, int(err.argmax()), float(err.max()))


@pytest.mark.parametrize('box', BOXES)
@pytest.mark.parametrize('shape', [(150, 170, 190), (96, 100, 104)])
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_parity_every_voxel(interp, shape, box):
    vol = rand_vol(shape, 21)
    ms = batch(shape, box)
    want = oracle_boxes(vol, ms, interp, box)
    assert not want[18].any() and want[0].any() and want[17].any()            # the outside box is empty, the others are not
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    for flags, kernel in ((0, 11 if routed_to_kernel_11(interp, box) else 1), (_native.FORCE_TILED, 11), (_native.FORCE_DIRECT, 1)):
        got = sv.extract(ms, box, _flags=flags)
        info = sv.info()
        assert info.last_kernel == kernel, (interp, shape, box, flags, info.last_kernel)
        if kernel == 11:
            assert info.last_lds_bytes <= 160 * 1024 and info.last_grid >= len(ms) and min(info.last_tile) > 0
        check(got, want, TOL[interp], (interp, shape, box, flags))
    sv.close()


def test_default_routing_includes_96_cube():
    assert routed_to_kernel_11('linear', (96, 96, 96)) and routed_to_kernel_11('filt_bspline', (96, 96, 96))


@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_footprint_that_fits_no_lds_box(interp):
    """scale 0.05 in the pull direction is magnification; the footprint that fits no LDS box is the minifying one (each box voxel
    steps 20 source voxels), as `minify_big` of the parity suite -- both are in the batch, among ordinary rotations, in order."""
    shape, box = (150, 170, 190), (32, 32, 32)
    vol = rand_vol(shape, 22)
    mid = (np.asarray(shape, np.float64) - 1) / 2
    ms = [centred(rot3((10, 20, 30)), mid, box), centred(20.0 * rot3((5, 50, -15)), mid + 0.25, box),
          centred(rot3((-40, 15, 80)), mid - 3.5, box), centred(np.diag([20.0, 20.0, 20.0]), mid, box),
          centred(0.05 * np.eye(3), mid + 0.5, box), centred(rot3((0, 0, 45)), mid + 7.25, box)]
    ms = np.ascontiguousarray(np.stack(ms), dtype=np.float32)
    want = oracle_boxes(vol, ms, interp, box)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    for flags in (0, _native.FORCE_TILED):
        got = sv.extract(ms, box, _flags=flags)
        check(got, want, TOL[interp], (interp, 'minify', flags))
    assert sv.info().last_kernel == 11
    sv.close()


@pytest.mark.parametrize('flags', [0, _native.FORCE_TILED, _native.FORCE_DIRECT])
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline_simple'])
def test_independence_and_determinism(interp, flags):
    shape, box = (96, 100, 104), (40, 48, 56)
    vol = rand_vol(shape, 23)
    ms = batch(shape, box)
    big = centred(20.0 * rot3((5, 50, -15)), (48, 50, 52), box).astype(np.float32)       # an entry on the global-gather route
    ms = np.concatenate([ms, big[None]])
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    whole = sv.extract(ms, box, _flags=flags).copy()
    again = sv.extract(ms, box, _flags=flags)
    assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))
    rev = sv.extract(ms[::-1].copy(), box, _flags=flags)
    assert np.array_equal(whole.view(np.uint32), rev[::-1].view(np.uint32))
    for i in range(len(ms)):
        alone = sv.extract(ms[i:i + 1], box, _flags=flags)
        assert np.array_equal(whole[i].view(np.uint32), alone[0].view(np.uint32)), (interp, flags, i)
    sv.close()


@pytest.mark.parametrize('flags', [0, _native.FORCE_TILED, _native.FORCE_DIRECT])
def test_known_answer_plain_crops(flags):
    shape, box = (50, 60, 70), (20, 24, 28)
    vol = rand_vol(shape, 24)
    starts = np.array([[5, 6, 7], [0, 0, 0], [40, 50, 60], [-8, 30, -10], [30, 36, 42], [45, -20, 66], [-30, -30, -30]])
    c = (np.asarray(box) - 1) / 2
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_at(starts + c, box_shape=box) if flags == 0 else \
        sv.extract(vt.utils.box_matrices(starts + c, None, box), box, _flags=flags)
    pad = 32
    padded = np.pad(vol, pad, mode='constant')
    for i, st in enumerate(starts):
        z, y, x = st + pad
        want = padded[z:z + box[0], y:y + box[1], x:x + box[2]]
        assert np.array_equal(got[i].view(np.uint32), want.view(np.uint32)), (flags, i)
    sv.close()


def test_handle_is_untouched():
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 25)
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(vol, interpolation='bspline', device='gpu:0')
    before = sv.affine(m).copy()
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    sv.extract(batch(shape, box), box)
    info = sv.info()
    assert (info.out_depth, info.out_height, info.out_width) == dims == shape
    after = sv.affine(m)
    assert after.shape == shape and np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert sv.affine_batch(np.stack([m, m])).shape == (2,) + shape and sv.projection(m).shape == shape[1:]
    sv.close()


def test_output_kinds_hold_the_same_bits():
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 26)
    ms = batch(shape, box)
    full = (len(ms),) + box
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fresh = sv.extract(ms, box)
    assert fresh.shape == full and fresh.dtype == np.float32
    host = np.full(full, 5, np.float32)
    assert sv.extract(ms, box, output=host) is None
    dev = vt.empty(full, device='gpu:0')
    assert sv.extract(ms, box, output=dev) is None
    sv.synchronize()
    assert np.array_equal(fresh.view(np.uint32), host.view(np.uint32))
    assert np.array_equal(fresh.view(np.uint32), dev.get().view(np.uint32))
    torch = pytest.importorskip('torch')
    tens = torch.full(full, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.extract(ms, box, output=tens) is None
    sv.synchronize()
    assert np.array_equal(fresh.view(np.uint32), tens.cpu().numpy().view(np.uint32))
    with pytest.raises(ValueError):
        sv.extract(ms, box, output=np.zeros((len(ms),) + (24, 40, 33), np.float32))
    sv.close()


@pytest.mark.parametrize('interp', list(TOL_EDGE))
def test_edge_scipy_handle_equals_cpu_extract(interp):
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 27)
    ms = batch(shape, box)
    want = vt.StaticVolume(vol, interpolation=interp, device='cpu').extract(ms, box)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    for flags in (0, _native.FORCE_TILED, _native.FORCE_DIRECT):
        check(sv.extract(ms, box, _flags=flags), want, TOL_EDGE[interp], (interp, 'edge=scipy', flags))
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_float64_matrices_on_a_long_axis(interp):
    shape, box = (40, 48, 3000), (16, 24, 40)
    vol = rand_vol(shape, 28)
    rs = np.random.RandomState(9)
    ms = np.stack([centred(rot3(rs.uniform(-20, 20, 3)), (20.123456789, 24.987654321, 2900.0 + rs.uniform(0, 60) + 1.0 / 3.0), box)
                   for _ in range(8)])
    assert ms.dtype == np.float64 and not np.array_equal(ms, ms.astype(np.float32).astype(np.float64))
    want = np.stack([oracle.affine_ex(vol, m, interp, box) for m in ms])
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    for flags in (0, _native.FORCE_TILED, _native.FORCE_DIRECT):
        check(sv.extract(ms, box, _flags=flags), want, TOL[interp], (interp, 'f64', flags))
    sv.close()


def test_user_sized_case():
    shape, box, n = (512, 512, 512), (64, 64, 64), 64
    vol = rand_vol(shape, 29)
    rs = np.random.RandomState(10)
    pos = rs.uniform(0, 511, (n, 3))
    rot = rs.uniform(0, 360, (n, 3))
    ms = vt.utils.box_matrices(pos, rot, box, rotation_order='sxyz').astype(np.float32)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    got = sv.extract(ms, box)
    assert sv.info().last_kernel == (11 if routed_to_kernel_11('filt_bspline', box) else 1)
    sv.close()
    check(got, oracle_boxes(vol, ms, 'filt_bspline', box), TOL['filt_bspline'], ('filt_bspline', shape, box))


def test_slab_and_unfinalized_handles_are_refused():
    lib = _native.load()
    vol = rand_vol((20, 24, 28), 30)
    m = np.eye(4, dtype=np.float32)
    out = np.zeros((8, 8, 8), np.float32)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert lib.vt_volume_extract(h, 1, m.ctypes.data, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    assert b'slab' in lib.vt_last_error()
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert lib.vt_volume_extract(h, 1, m.ctypes.data, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    assert b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    _native.check(lib.vt_volume_extract(h, 1, m.ctypes.data, 8, 8, 8, out.ctypes.data, 0), 'extract')
    assert np.array_equal(out, vol[:8, :8, :8])
    lib.vt_volume_destroy(h)
