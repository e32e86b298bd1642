"""-m gpu: StaticVolume.extract_sum / average_at (vt_volume_extract_sum, kernel 13) against the float64 weighted sum of the oracle's
boxes on every voxel, against the library's own boxes to one float32 rounding, and bit for bit where the arithmetic is exact."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, TOL_EDGE, ALL_INTERPS, VT_EINVAL, batch, centred, rot3, oracle_boxes, rand_vol

pytestmark = pytest.mark.gpu

SHAPE = (96, 100, 104)
FLAGS = [0, _native.FORCE_TILED, _native.FORCE_DIRECT]


def weights(n):
    w = np.random.RandomState(5).uniform(-1, 2, n)
    if n > 3:
        w[3] = 0
    if n > 7:
        w[7] = -0.75
    return w


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tiles_of(info, box):
    return int(np.prod([-(-b // t) for b, t in zip(box, info.last_tile)]))


@functools.lru_cache(maxsize=None)
def oracle_case(interp, box):
    """(matrices, float64 oracle boxes) of the 25-matrix batch out of the SHAPE source: computed once per (interp, box), never modified."""
    ms = batch(SHAPE, box)
    want = oracle_boxes(rand_vol(SHAPE, 21), ms, interp, box).astype(np.float64)
    want.setflags(write=False)
    ms.setflags(write=False)
    return ms, want


def check_sum(got, boxes, w, tol, what):
    """|got - sum_i w_i box_i| <= sum|w_i| * tol + 2^-23 |want|: every box voxel is within tol of the oracle, one float32 rounding follows."""
    want = np.tensordot(w, boxes, axes=1)
    bound = np.abs(w).sum() * tol + 2.0 ** -23 * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    print(what, f'max|hip-oracle| {err.max():.3e}  min(bound) {bound.min():.3e}  worst ratio {(err / bound).max():.3f}')
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, float((err / bound).max()))


# ---- 1. parity against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize('box', [(17, 23, 29), (40, 48, 56)])
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_parity_against_the_oracle(interp, box):
    ms, boxes = oracle_case(interp, box)
    assert not boxes[18].any() and boxes[0].any() and boxes[17].any()           # the outside box is empty, the others are not
    w = weights(len(ms))
    assert w[18] != 0
    w_other = w.copy()
    w_other[18] = 1000.0
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    for flags in FLAGS:
        got = sv.extract_sum(ms, box, w, _flags=flags)
        info = sv.info()
        assert info.last_kernel == 13, (interp, box, flags, info.last_kernel)
        assert info.last_lds_bytes <= 160 * 1024 and min(info.last_tile) > 0 and info.last_grid >= tiles_of(info, box)
        check_sum(got, boxes, w, TOL[interp], (interp, box, flags))
        # the box that lies entirely outside contributes nothing, whatever its weight
        assert np.array_equal(bits(got), bits(sv.extract_sum(ms, box, w_other, _flags=flags))), (interp, box, flags)
    sv.close()


# ---- 2. against the library's own boxes, 3. n = 1 --------------------------------------------------------------------
def own_batch(box):
    ms = batch(SHAPE, box)
    big = centred(20.0 * rot3((5, 50, -15)), (48, 50, 52), box).astype(np.float32)       # an entry on the global-gather route
    return np.concatenate([ms, big[None]])


@pytest.mark.parametrize('flags', [0, _native.FORCE_TILED])
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline_simple'])
def test_against_the_librarys_own_boxes_and_single_boxes(interp, flags):
    box = (40, 48, 56)
    ms = own_batch(box)
    w = weights(len(ms))
    sv = vt.StaticVolume(rand_vol(SHAPE, 23), interpolation=interp, device='gpu:0')
    own = sv.extract(ms, box, _flags=flags).astype(np.float64)
    assert own[-1].any()
    got = sv.extract_sum(ms, box, w, _flags=flags)
    assert sv.info().last_kernel == 13
    ref = np.tensordot(w, own, axes=1)
    mag = np.tensordot(np.abs(w), np.abs(own), axes=1)
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * mag           # one correct float32 rounding + float64 accumulation error
    print(interp, flags, f'max err {err.max():.3e}, worst err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}')
    assert (err <= bound).all(), (interp, flags, float(err.max()))
    # n = 1, weight 1: the box of extract, bit for bit
    for i in range(len(ms)):
        alone = sv.extract_sum(ms[i:i + 1], box, _flags=flags)
        assert np.array_equal(bits(alone), bits(own[i].astype(np.float32))), (interp, flags, i)
    sv.close()


# ---- 4. segments -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case(interp):
    shape, box, n = (40, 44, 48), (8, 8, 8), 257
    rs = np.random.RandomState(3)
    s = np.asarray(shape, np.float64)
    ms = np.stack([centred(rot3(rs.uniform(0, 360, 3)), rs.uniform(0.15, 0.85, 3) * s, box) for _ in range(n)]).astype(np.float32)
    vol = rand_vol(shape, 31)
    boxes = oracle_boxes(vol, ms, interp, box).astype(np.float64)
    for a in (ms, vol, boxes):
        a.setflags(write=False)
    return shape, box, vol, ms, boxes


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_segments(interp):
    shape, box, vol, ms, boxes = small_case(interp)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    for n in (1, 2, 25, 257):
        w = weights(n)
        got = sv.extract_sum(ms[:n], box, w)
        info = sv.info()
        tiles = tiles_of(info, box)
        assert info.last_kernel == 13 and info.last_grid % tiles == 0
        segments = info.last_grid // tiles
        assert 1 <= segments <= n
        if n == 1:
            assert segments == 1
        if n == 257:
            assert segments > 1
        check_sum(got, boxes[:n], w, TOL[interp], (interp, 'segments', n, segments))
    sv.close()


def test_several_matrices_in_one_segment():
    box = (128, 128, 128)
    vol = rand_vol(SHAPE, 21)
    s = np.asarray(SHAPE, np.float64)
    ms = np.stack([centred(rot3((10, 20, 30)), (s - 1) / 2, box), centred(rot3((-40, 15, 80)), (s - 1) / 2 + 0.3, box),
                   centred(0.5 * rot3((5, 50, -15)), (s - 1) / 2 - 0.7, box)]).astype(np.float32)
    w = weights(3)
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_sum(ms, box, w)
    info = sv.info()
    assert info.last_kernel == 13 and info.last_grid == tiles_of(info, box) >= 1024
    sv.close()
    check_sum(got, oracle_boxes(vol, ms, 'linear', box).astype(np.float64), w, TOL['linear'], ('one segment', box))


# ---- 5. known answer -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_known_answer_weighted_crops(flags):
    shape, box = (50, 60, 70), (20, 24, 28)
    vol = rand_vol(shape, 24)
    starts = np.array([[5, 6, 7], [0, 0, 0], [40, 50, 60], [-8, 30, -10], [30, 36, 42], [45, -20, 66], [-30, -30, -30]])
    w = np.array([1, 2, 0.5, -1, 4, 0.25, 1], np.float64)
    c = (np.asarray(box) - 1) / 2
    pad = 32
    padded = np.pad(vol, pad, mode='constant')
    want = np.zeros(box, np.float64)
    for wi, st in zip(w, starts):
        z, y, x = st + pad
        want += wi * padded[z:z + box[0], y:y + box[1], x:x + box[2]].astype(np.float64)      # exact: float32 times a few bits, short sums
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_sum(vt.utils.box_matrices(starts + c, None, box), box, w, _flags=flags)
    assert sv.info().last_kernel == 13
    sv.close()
    assert np.array_equal(bits(got), bits(want.astype(np.float32))), flags


# ---- 6. determinism and outputs, 7. handle untouched ---------------------------------------------------------------------
def test_determinism_and_output_kinds():
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 26)
    ms = batch(shape, box)
    w = weights(len(ms))
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fresh = sv.extract_sum(ms, box, w).copy()
    assert fresh.shape == box and fresh.dtype == np.float32 and fresh.any()
    assert np.array_equal(bits(fresh), bits(sv.extract_sum(ms, box, w)))
    sv.affine(m)
    sv.extract(ms, box)
    sv.projection_batch(np.stack([m, m]), _flags=_native.FORCE_TILED)
    assert np.array_equal(bits(fresh), bits(sv.extract_sum(ms, box, w)))
    fresh_sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    assert np.array_equal(bits(fresh), bits(fresh_sv.extract_sum(ms, box, w)))
    fresh_sv.close()
    host = np.full(box, 5, np.float32)
    assert sv.extract_sum(ms, box, w, output=host) is None
    dev = vt.empty(box, device='gpu:0')
    assert sv.extract_sum(ms, box, w, output=dev) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(host)) and np.array_equal(bits(fresh), bits(dev.get()))
    torch = pytest.importorskip('torch')
    tens = torch.full(box, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.extract_sum(ms, box, w, output=tens) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    with pytest.raises(ValueError):
        sv.extract_sum(ms, box, w, output=np.zeros((24, 40, 33), np.float32))
    with pytest.raises(ValueError):
        sv.extract_sum(ms, box, w[:-1])
    sv.close()


def test_handle_is_untouched():
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 25)
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(vol, interpolation='bspline', device='gpu:0')
    before = sv.affine(m).copy()
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    ms = batch(shape, box)
    assert sv.extract_sum(ms, box, weights(len(ms))).shape == box
    info = sv.info()
    assert (info.out_depth, info.out_height, info.out_width) == dims == shape
    after = sv.affine(m)
    assert after.shape == shape and np.array_equal(bits(before), bits(after))
    assert sv.affine_batch(np.stack([m, m])).shape == (2,) + shape and sv.projection(m).shape == shape[1:]
    sv.close()


# ---- 8. edge='scipy' --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', list(TOL_EDGE))
def test_edge_scipy_handle_equals_cpu_extract_sum(interp):
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 27)
    ms = batch(shape, box)
    w = weights(len(ms))
    want = vt.StaticVolume(vol, interpolation=interp, device='cpu').extract_sum(ms, box, w)
    sv =vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    for flags in FLAGS:
        got = sv.extract_sum(ms, box, w, _flags=flags)
        ref = want.astype(np.float64)
        bound = np.abs(w).sum() * TOL_EDGE[interp] + 2.0 ** -23 * np.abs(ref)
        err = np.abs(got.astype(np.float64) - ref)
        print(interp, 'edge=scipy', flags, f'max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}')
        assert (err <= bound).all(), (interp, flags, float(err.max()))
    sv.close()


# ---- 9. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    vol = rand_vol((20, 24, 28), 30)
    m = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    one = np.ones(1)
    out = np.zeros((8, 8, 8), np.float32)

    def call(h, n=1, mat=m, w=one, box=(8, 8, 8)):
        return lib.vt_volume_extract_sum(h, n, mat.ctypes.data, None if w is None else w.ctypes.data, *box, out.ctypes.data, 0)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    assert lib.vt_volume_extract_sum_f64(h, 1, m64.ctypes.data, None, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    assert call(h, n=0) == VT_EINVAL
    bad = m.copy()
    bad[1, 2] = np.nan
    assert call(h, mat=bad) == VT_EINVAL and b'finite' in lib.vt_last_error()
    assert call(h, w=np.array([np.inf])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    assert call(h, box=(0, 8, 8)) == VT_EINVAL
    _native.check(call(h, w=np.array([2.0])), 'extract_sum')
    assert np.array_equal(out, 2.0 * vol[:8, :8, :8])
    _native.check(call(h, w=None), 'extract_sum without weights')
    assert np.array_equal(out, vol[:8, :8, :8])
    _native.check(lib.vt_volume_extract_sum_f64(h, 1, m64.ctypes.data, one.ctypes.data, 8, 8, 8, out.ctypes.data, 0), 'extract_sum_f64')
    assert np.array_equal(out, vol[:8, :8, :8])
    lib.vt_volume_destroy(h)


# ---- 10. user-sized ---------------------------------------------------------------------------------------------------
def test_user_sized_case():
    shape, box, n = (512, 512, 512), (64, 64, 64), 64
    vol = rand_vol(shape, 29)
    rs = np.random.RandomState(10)
    pos = rs.uniform(0, 511, (n, 3))
    rot = rs.uniform(0, 360, (n, 3))
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    got = sv.average_at(pos, rot, box, rotation_order='sxyz')
    assert sv.info().last_kernel == 13
    sv.close()
    ms = vt.utils.box_matrices(pos, rot, box, rotation_order='sxyz')
    check_sum(got, oracle_boxes(vol, ms, 'filt_bspline', box).astype(np.float64), np.full(n, 1.0 / n), TOL['filt_bspline'],
              ('filt_bspline', shape, box))
