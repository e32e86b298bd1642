"""-m gpu: StaticVolume.projection_batch / tilt_series (vt_volume_project_batch, kernel 12) against the oracle's generalised
entry point summed over axis 0 in float64, on EVERY pixel of every image.

Tolerance: TOL[interp] * depth, derived rather than measured -- every voxel of the transformed volume is within TOL of the
oracle (the contract of tests/test_gpu_parity.py), the float64 accumulation adds nothing at this scale, and the single final
rounding is <= 2^-24 * depth for inputs in [0, 1).  tests/test_gpu_parity.py::test_projection_matches_oracle uses the same."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle

pytestmark = pytest.mark.gpu

TOL = {'linear': 1e-6, 'bspline': 1e-6, 'bspline_simple': 1e-6, 'filt_bspline': 3e-6, 'filt_bspline_simple': 3e-6}   # tests/test_gpu_parity.py
TOL_EDGE = {'linear': 1e-6, 'bspline': 2e-6, 'filt_bspline': 1e-5}       # tests/test_gpu_edge_scipy.py
ALL_INTERPS = list(TOL)
VT_EINVAL = 10001
SHAPE = (72, 80, 88)
# the source's own shape; ragged in every tile dimension; depth below one tile; many depth tiles per image (several segments);
# and an image of 1024 tiles or more, the size from which an image is one depth segment and kernel 12 stores without the reduce pass
OUT_SHAPES = [SHAPE, (33, 47, 50), (5, 16, 130), (70, 20, 24), (20, 512, 512)]
OUTSIDE = 10        # index of the matrix that maps the whole output outside the volume


def routed_to_kernel_12(interp, oshape):
    """The committed default routing rule (vt_api.hip: project_batch_routes_fused)."""
    if interp == 'linear':
        return max(oshape) <= 256
    if interp in ('bspline', 'filt_bspline'):
        return max(oshape) <= 64
    return False


@functools.lru_cache(maxsize=None)
def rand_vol(shape, seed=0):
    v = np.random.RandomState(seed).random_sample(shape).astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def oracle_source(shape, seed, filtered):
    v = oracle.prefilter(rand_vol(shape, seed)) if filtered else rand_vol(shape, seed)
    v.setflags(write=False)
    return v


def rot3(angles, order='sxyz'):
    return vt.utils.rotation_matrix(angles, 'deg', order, dtype=np.float64)[:3, :3]


def centred(m3, oshape, shape=SHAPE, shift=(0.0, 0.0, 0.0)):
    """4x4 float64 pull matrix with linear part m3 that maps the centre of the output onto the centre of the volume (+ shift)."""
    c = (np.asarray(oshape, np.float64) - 1) / 2
    m = np.eye(4)
    m[:3, :3] = m3
    m[:3, 3] = (np.asarray(shape, np.float64) - 1) / 2 + np.asarray(shift, np.float64) - np.asarray(m3, np.float64) @ c
    return m


def batch(oshape, shape=SHAPE):
    """The eleven float64 matrices of the parity cases, none of them exact in float32."""
    sh = np.eye(3)
    sh[0, 1], sh[0, 2], sh[1, 2] = 0.2, -0.15, 0.3
    ident = np.eye(4)
    ident[:3, 3] = (3.0, -2.0, 5.0)
    third = (1.0 / 3.0, -1.0 / 7.0, 1.0 / 9.0)
    ms = [centred(rot3((0, 0, 0)), oshape, shape, third),                                      # 0: tilt about axis 1 by 0
          centred(rot3((0, 30, 0)), oshape, shape, third),                                     # 1: ... by 30
          centred(rot3((0, -60, 0)), oshape, shape, third),                                    # 2: ... by -60
          centred(rot3((0, 0, 45)), oshape, shape, third),                                     # 3: tilt about axis 2 by 45
          centred(rot3((20, 35, -50)), oshape, shape, third),                                  # 4: general rotation
          centred(2.0 * rot3((20, 35, -50)), oshape, shape, third),                            # 5: ... at scale 2
          centred(20.0 * rot3((5, 50, -15)), oshape, shape, third),                            # 6: minification: the global-gather route
          centred(np.diag([-1.0, 1.0, -1.0]), oshape, shape, (0.5, 0.25, -0.25)),              # 7: mirror
          centred(sh, oshape, shape, third),                                                    # 8: shear
          ident,                                                                                # 9: identity, integer offset
          centred(rot3((10, 20, 30)), oshape, shape, 3.0 * np.asarray(shape) + 2.0 * np.asarray(oshape))]   # 10: entirely outside
    assert len(ms) == 11
    return np.stack(ms)


def oracle_images(shape, seed, ms, interp, oshape):
    src = oracle_source(shape, seed, interp.startswith('filt'))
    okind = interp[5:] if interp.startswith('filt') else interp
    return np.stack([oracle.affine_ex(src, np.asarray(m, np.float64), okind, oshape).sum(axis=0, dtype=np.float64) for m in ms])


def check(got, want, tol, what):
    assert got.shape == want.shape and got.dtype == np.float32, what
    err = np.abs(got.astype(np.float64) - want).reshape(got.shape[0], -1).max(axis=1)
    print(what, 'tol %.2e' % tol, 'max|hip-oracle| per image:', ' '.join(f'{e:.2e}' for e in err))
    assert np.isfinite(got).all(), what
    assert err.max() <= tol, (what, int(err.argmax()), float(err.max()))


def segments_of(sv, oshape):
    """Depth segments kernel 12 used for the single-matrix launch that was just made (last_grid = segments * in-plane tiles)."""
    info = sv.info()
    _, th, tw = info.last_tile
    inplane = -(-oshape[1] // th) * -(-oshape[2] // tw)
    assert info.last_grid % inplane == 0
    return info.last_grid // inplane


@pytest.mark.parametrize('oshape', OUT_SHAPES)
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_parity_every_pixel(interp, oshape):
    vol = rand_vol(SHAPE, 31)
    m64 = batch(oshape)
    m32 = np.ascontiguousarray(m64, dtype=np.float32)
    assert not np.array_equal(m64, m32.astype(np.float64))
    tol = TOL[interp] * oshape[0]
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    for ms in (m32, m64):
        want = oracle_images(SHAPE, 31, ms, interp, oshape)
        assert not want[OUTSIDE].any() and all(want[i].any() for i in range(len(ms)) if i != OUTSIDE)
        for flags in (0, _native.FORCE_TILED, _native.FORCE_DIRECT):
            got = sv.projection_batch(ms, oshape, _flags=flags)
            info = sv.info()
            if flags == _native.FORCE_TILED:
                assert info.last_kernel == 12 and info.last_lds_bytes <= 160 * 1024 and min(info.last_tile) > 0 and info.last_grid >= 1
            elif flags == _native.FORCE_DIRECT:
                assert info.last_kernel != 12
            else:
                assert (info.last_kernel == 12) == routed_to_kernel_12(interp, oshape), (interp, oshape, info.last_kernel)
            check(got, want, tol, (interp, oshape, str(ms.dtype), flags, 'kernel %d' % info.last_kernel))
            assert not got[OUTSIDE].any()
    # the deep, narrow output splits its depth between workgroups; the image of 1024 tiles does not
    sv.projection_batch(m32[4:5], oshape, _flags=_native.FORCE_TILED)
    if oshape == (70, 20, 24):
        assert segments_of(sv, oshape) >= 2
    if oshape == (20, 512, 512):
        assert segments_of(sv, oshape) == 1
    sv.close()


@pytest.mark.parametrize('oshape', [(70, 20, 24), (33, 47, 50), (20, 512, 512)])
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline_simple'])
def test_independence_and_determinism(interp, oshape):
    flags = _native.FORCE_TILED
    ms = np.ascontiguousarray(batch(oshape), dtype=np.float32)
    sv = vt.StaticVolume(rand_vol(SHAPE, 32), interpolation=interp, device='gpu:0')
    whole = sv.projection_batch(ms, oshape, _flags=flags).copy()
    assert sv.info().last_kernel == 12
    again = sv.projection_batch(ms, oshape, _flags=flags)
    assert np.array_equal(whole.view(np.uint32), again.view(np.uint32))
    rev = sv.projection_batch(ms[::-1].copy(), oshape, _flags=flags)
    assert np.array_equal(whole.view(np.uint32), rev[::-1].view(np.uint32))
    for i in range(len(ms)):
        alone = sv.projection_batch(ms[i:i + 1], oshape, _flags=flags)
        assert np.array_equal(whole[i].view(np.uint32), alone[0].view(np.uint32)), (interp, oshape, i)
    dev = vt.empty(whole.shape, device='gpu:0')
    assert sv.projection_batch(ms, oshape, output=dev, _flags=flags) is None
    sv.synchronize()
    assert np.array_equal(whole.view(np.uint32), dev.get().view(np.uint32))
    host = np.full(whole.shape, 5, np.float32)
    assert sv.projection_batch(ms, oshape, output=host, _flags=flags) is None
    assert np.array_equal(whole.view(np.uint32), host.view(np.uint32))
    sv.close()


@pytest.mark.parametrize('interp', list(TOL_EDGE))
def test_edge_scipy_handle_equals_cpu(interp):
    shape, oshape = (40, 44, 48), (36, 50, 40)
    vol = rand_vol(shape, 33)
    ms = np.ascontiguousarray(np.stack([centred(rot3((0, 25, 0)), oshape, shape, (0.3, -0.4, 0.25)),
                                        centred(rot3((20, 35, -50)), oshape, shape, (0.1, 0.2, 0.3)),
                                        centred(rot3((5, -10, 8)), oshape, shape, (12.5, -9.25, 7.75))]), dtype=np.float32)   # a face inside the output
    want = vt.StaticVolume(vol, interpolation=interp, device='cpu').projection_batch(ms, oshape).astype(np.float64)
    assert (want[2] == 0).any() and want[2].any()
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    for flags in (0, _native.FORCE_TILED, _native.FORCE_DIRECT):
        got = sv.projection_batch(ms, oshape, _flags=flags)
        check(got, want, TOL_EDGE[interp] * oshape[0], (interp, 'edge=scipy', flags, 'kernel %d' % sv.info().last_kernel))
    sv.close()


@pytest.mark.parametrize('flags', [0, _native.FORCE_TILED, _native.FORCE_DIRECT])
def test_shared_handle_state(flags):
    """Kernel 12 leaves the handle as it found it: same resident bytes, same output shape, same bits on the second visit.  The loop
    route is the single-matrix path, so it may build that path's lazy copies and helper (resident bytes are then vt_volume_project's
    to account for, and a later visit may run on another kernel family: both visits are within the tolerance of the oracle, so within
    twice that of each other); it sets the handle's output shape for the duration of the call and must have put it back."""
    shape = (70, 66, 72)
    small, large = (33, 47, 50), (64, 96, 100)
    vol = rand_vol(shape, 34)
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    ms_small = np.ascontiguousarray(batch(small, shape), dtype=np.float32)
    ms_large = np.ascontiguousarray(batch(large, shape), dtype=np.float32)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fused = []

    def batch_call(ms, oshape):
        before = sv.info().resident_bytes
        got = sv.projection_batch(ms, oshape, _flags=flags).copy()
        info = sv.info()
        fused.append(info.last_kernel == 12)
        if fused[-1]:
            assert info.resident_bytes == before, (oshape, before, info.resident_bytes)
        assert (info.out_depth, info.out_height, info.out_width) == shape
        assert sv.affine(m).shape == shape
        return got

    first = batch_call(ms_small, small)
    # under FORCE_TILED and on the default route of a class the rule sends to kernel 12, the strict invariants above and below apply
    assert fused[-1] == (flags == _native.FORCE_TILED or (flags == 0 and routed_to_kernel_12('filt_bspline', small)))
    assert routed_to_kernel_12('filt_bspline', small) and not routed_to_kernel_12('filt_bspline', large)
    vol_before = sv.affine(m).copy()
    assert vol_before.shape == shape
    assert sv.projection(m).shape == shape[1:]
    assert sv.extract(ms_small[:5], (16, 16, 16)).shape == (5, 16, 16, 16)
    assert sv.affine_batch(np.stack([m, m])).shape == (2,) + shape
    assert batch_call(ms_large, large).shape == (len(ms_large),) + large[1:]
    last = batch_call(ms_small, small)
    if fused[0] and fused[-1]:
        assert np.array_equal(first.view(np.uint32), last.view(np.uint32))
    else:
        assert np.abs(first.astype(np.float64) - last).max() <= 2 * TOL['filt_bspline'] * small[0]
    after = sv.affine(m)
    assert after.shape == shape and np.array_equal(vol_before.view(np.uint32), after.view(np.uint32))
    sv.close()


def test_c_level_error_codes():
    lib = _native.load()
    vol = rand_vol((20, 24, 28), 35)
    m = np.eye(4, dtype=np.float32)
    out = np.zeros((8, 8), np.float32)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert lib.vt_volume_project_batch(h, 1, m.ctypes.data, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    assert b'slab' in lib.vt_last_error()
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert lib.vt_volume_project_batch(h, 1, m.ctypes.data, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    assert b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    bad = m.copy()
    bad[1, 2] = np.nan
    m64 = np.eye(4)
    for flags in (0, _native.FORCE_TILED, _native.FORCE_DIRECT):
        assert lib.vt_volume_project_batch(h, 1, bad.ctypes.data, 8, 8, 8, out.ctypes.data, flags) == VT_EINVAL
        assert lib.vt_volume_project_batch(h, 0, m.ctypes.data, 8, 8, 8, out.ctypes.data, flags) == VT_EINVAL
        assert lib.vt_volume_project_batch_f64(h, -1, m64.ctypes.data, 8, 8, 8, out.ctypes.data, flags) == VT_EINVAL
        for dims in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (8, -3, 8)):
            assert lib.vt_volume_project_batch(h, 1, m.ctypes.data, *dims, out.ctypes.data, flags) == VT_EINVAL
            assert lib.vt_volume_project_batch_f64(h, 1, m64.ctypes.data, *dims, out.ctypes.data, flags) == VT_EINVAL
        _native.check(lib.vt_volume_project_batch(h, 1, m.ctypes.data, 8, 8, 8, out.ctypes.data, flags), 'project_batch')
        want = vol[:8, :8, :8].sum(axis=0, dtype=np.float64)
        assert np.abs(out - want).max() <= 8 * 2.0 ** -24 * 8, flags       # eight exact samples in [0, 1): the final rounding (and float32 partial sums on the loop path)
    lib.vt_volume_destroy(h)


def test_tilt_series_matches_project_and_fills_a_torch_tensor():
    shape = (48, 52, 56)
    vol = rand_vol(shape, 36)
    angles = [-60.0, -20.0, 0.0, 35.0]
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    tol = TOL['linear'] * shape[0]
    for axis in (1, 2):
        got = sv.tilt_series(angles, axis)
        assert got.shape == (len(angles),) + shape[1:]
        for i, a in enumerate(angles):
            r = [0.0, 0.0, 0.0]
            r[axis] = a
            one = sv.project(rotation=tuple(r), rotation_order='sxyz')
            # both are within tol of the oracle's image of the same matrix
            assert np.abs(got[i].astype(np.float64) - one).max() <= 2 * tol, (axis, a)
    torch = pytest.importorskip('torch')
    tens = torch.full((len(angles),) + shape[1:], 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.tilt_series(angles, 1, output=tens) is None
    sv.synchronize()
    assert np.array_equal(sv.tilt_series(angles, 1).view(np.uint32), tens.cpu().numpy().view(np.uint32))
    sv.close()
