"""-m gpu: StaticVolume.extract_sum_multi / class_averages_at (vt_volume_extract_sum_multi, kernel 16).  The defining property is that box j
holds the bits extract_sum (kernel 13) gives for column j of the weights alone; the oracle, exact crops and the refusals are checked
besides."""
import ctypes

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, batch, rand_vol
from test_gpu_extract_sum import SHAPE, FLAGS, bits, check_sum, oracle_case, own_batch, small_case, tiles_of

pytestmark = pytest.mark.gpu

G = 9                                                        # a ragged last chunk for 2, 4 and 8 columns per workgroup
CHUNK = {(16, 16, 16): 2, (8, 16, 16): 4, (8, 8, 16): 8}     # columns per workgroup for each tile (include/voltools_hip.h)


def weight_matrix(n, g=G, seed=7):
    """n x g in (-1, 2) with, where they exist: row 3 all zero, row 5 zero in columns 0..7 (the whole first chunk, whatever its width, and
    every whole chunk of 2 or 4), row 9 zero in columns 0 and 1 only, and column 6 all zero."""
    w = np.random.RandomState(seed).uniform(-1, 2, (n, g))
    if n > 3:
        w[3] = 0
    if n > 5:
        w[5, :8] = 0
    if n > 9:
        w[9, :2] = 0
    if g > 6:
        w[:, 6] = 0
    return w


def chunks_of(info, g):
    return -(-g // CHUNK[tuple(info.last_tile)])


def columns_by_kernel_13(sv, ms, box, w, flags=0):
    want = np.stack([sv.extract_sum(ms, box, np.ascontiguousarray(w[:, j]), _flags=flags) for j in range(w.shape[1])])
    assert sv.info().last_kernel == 13
    return want


# ---- 1. bit identity with kernel 13 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp,box', [(i, (17, 23, 29)) for i in ALL_INTERPS] + [('linear', (40, 48, 56)), ('filt_bspline', (40, 48, 56))])
def test_bit_identity_with_kernel_13(interp, box):
    ms = own_batch(box)                                       # the 25-matrix batch and an entry on the global-gather route
    w = weight_matrix(len(ms))
    assert not w[3].any() and not w[5, :8].any() and w[5, 8] != 0 and not w[:, 6].any() and not w[9, :2].any() and w[9, 2] != 0
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    for flags in FLAGS:
        got = sv.extract_sum_multi(ms, box, w, _flags=flags)
        info = sv.info()
        assert info.last_kernel == 16, (interp, box, flags, info.last_kernel)
        assert got.shape == (G,) + box and got.dtype == np.float32 and np.isfinite(got).all()
        # (the larger box's partials pass 64 MiB: several launches, last_grid is the last one's)
        assert info.last_lds_bytes <= 160 * 1024 and min(info.last_tile) > 0 and info.last_grid % tiles_of(info, box) == 0
        want = columns_by_kernel_13(sv, ms, box, w, flags)
        for j in range(G):
            assert np.array_equal(bits(got[j]), bits(want[j])), (interp, box, flags, j)
        assert got[0].any() and got[8].any() and not got[6].any()
    sv.close()


# ---- 2. segments -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_segments(interp):
    shape, box, vol, ms, _ = small_case(interp)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    for n in (1, 2, 25, 257):
        for g in (1, 5):
            w = weight_matrix(n, g, seed=11)
            got = sv.extract_sum_multi(ms[:n], box, w)
            info = sv.info()
            per_segment = tiles_of(info, box) * chunks_of(info, g)
            assert info.last_kernel == 16 and info.last_grid % per_segment == 0, (n, g, info.last_grid)
            segments = info.last_grid // per_segment
            assert 1 <= segments <= n
            if n == 1:
                assert segments == 1
            if n == 257:
                assert segments > 1
            want = columns_by_kernel_13(sv, ms[:n], box, w)
            assert sv.info().last_grid == segments * tiles_of(sv.info(), box)           # kernel 13 made the same segments
            for j in range(g):
                assert np.array_equal(bits(got[j]), bits(want[j])), (interp, n, g, j)
    sv.close()


# ---- 3. parity against the oracle, independent of kernel 13 -----------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_parity_against_the_oracle(interp):
    box = (17, 23, 29)
    ms, boxes = oracle_case(interp, box)
    w = weight_matrix(len(ms), 3, seed=13)
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    got = sv.extract_sum_multi(ms, box, w)
    assert sv.info().last_kernel == 16
    sv.close()
    for j in range(3):
        check_sum(got[j], boxes, w[:, j], TOL[interp], (interp, box, 'column', j))


# ---- 4. split of the partials ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_partials_beyond_the_cap_split_the_call(interp, monkeypatch):
    """VT_DOT_PART_CAP (read when the handle is created) is lowered to one column chunk's partials, to eight bytes less than that (still
    one chunk per launch) and to two chunks' worth and a little: the columns are independent, so the bits are those of the unsplit call
    on a handle with the default cap."""
    shape, box, vol, ms, _ = small_case(interp)
    w = weight_matrix(len(ms), G, seed=17)
    plain = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    want = plain.extract_sum_multi(ms, box, w).copy()
    info = plain.info()
    tiles, gc = tiles_of(info, box), CHUNK[tuple(info.last_tile)]
    chunks = -(-G // gc)
    assert info.last_grid % (tiles * chunks) == 0                 # one launch
    segments = info.last_grid // (tiles * chunks)
    assert segments > 1
    plain.close()
    part_chunk = gc * segments * int(np.prod(box)) * 8
    for cap, chunks_per in ((part_chunk, 1), (part_chunk - 8, 1), (2 * part_chunk + 8, 2)):
        monkeypatch.setenv('VT_DOT_PART_CAP', str(cap))
        sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
        monkeypatch.delenv('VT_DOT_PART_CAP')
        got = sv.extract_sum_multi(ms, box, w)
        info = sv.info()
        last_cols = G - (-(-G // (chunks_per * gc)) - 1) * chunks_per * gc
        assert info.last_kernel == 16 and info.last_grid == tiles * segments * -(-last_cols // gc), (cap, info.last_grid, tiles, segments)
        if chunks_per == 1:
            assert chunks > 1                                       # several launches
        assert np.array_equal(bits(got), bits(want)), (interp, cap)
        sv.close()


# ---- 5. independence of the stack ---------------------------------------------------------------------------------------------
def test_independence_of_the_stack():
    box = (17, 23, 29)
    ms = own_batch(box)
    w = weight_matrix(len(ms))
    sv = vt.StaticVolume(rand_vol(SHAPE, 23), interpolation='filt_bspline', device='gpu:0')
    full = sv.extract_sum_multi(ms, box, w).copy()
    assert np.array_equal(bits(sv.extract_sum_multi(ms, box, w[:, [4, 0]])), bits(full[[4, 0]]))
    assert np.array_equal(bits(sv.extract_sum_multi(ms, box, w[:, :1])), bits(full[:1]))
    order = list(range(G))
    order[1], order[7] = order[7], order[1]
    assert np.array_equal(bits(sv.extract_sum_multi(ms, box, w[:, order])), bits(full[order]))
    sv.close()


# ---- 6. known answer, exact -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_known_answer_weighted_crops(flags):
    shape, box = (50, 60, 70), (20, 24, 28)
    vol = rand_vol(shape, 24)
    starts = np.array([[5, 6, 7], [0, 0, 0], [40, 50, 60], [-8, 30, -10], [30, 36, 42], [45, -20, 66], [-30, -30, -30]])
    w = np.array([[1, 0.5, 0], [2, -1, 0], [0.5, 4, 0.25], [-1, 0.25, 0], [4, 1, 0], [0.25, 2, 0], [1, -0.5, 8]], np.float64)
    c = (np.asarray(box) - 1) / 2
    pad = 32
    padded = np.pad(vol, pad, mode='constant')
    want = np.zeros((3,) + box, np.float64)
    for wi, st in zip(w, starts):
        z, y, x = st + pad
        crop = padded[z:z + box[0], y:y + box[1], x:x + box[2]].astype(np.float64)
        for j in range(3):
            want[j] += wi[j] * crop                            # exact: float32 times a few bits, short sums
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_sum_multi(vt.utils.box_matrices(starts + c, None, box), box, w, _flags=flags)
    assert sv.info().last_kernel == 16
    sv.close()
    assert want[2].any()
    assert np.array_equal(bits(got), bits(want.astype(np.float32))), flags


# ---- 7. determinism, outputs, handle untouched ----------------------------------------------------------------------------------
def test_determinism_output_kinds_and_handle_untouched():
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 26)
    ms = batch(shape, box)
    w = weight_matrix(len(ms), 5, seed=19)
    out_shape = (5,) + box
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    before = sv.affine(m).copy()
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    fresh = sv.extract_sum_multi(ms, box, w).copy()
    assert fresh.shape == out_shape and fresh.dtype == np.float32 and fresh.any()
    info = sv.info()
    assert (info.out_depth, info.out_height, info.out_width) == dims == shape
    assert np.array_equal(bits(fresh), bits(sv.extract_sum_multi(ms, box, w)))
    after = sv.affine(m)
    assert after.shape == shape and np.array_equal(bits(before), bits(after))
    sv.extract(ms, box)
    sv.extract_sum(ms, box, w[:, 0])
    assert np.array_equal(bits(fresh), bits(sv.extract_sum_multi(ms, box, w)))
    fresh_sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    assert np.array_equal(bits(fresh), bits(fresh_sv.extract_sum_multi(ms, box, w)))
    fresh_sv.close()
    host = np.full(out_shape, 5, np.float32)
    assert sv.extract_sum_multi(ms, box, w, output=host) is None
    dev = vt.empty(out_shape, device='gpu:0')
    assert sv.extract_sum_multi(ms, box, w, output=dev) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(host)) and np.array_equal(bits(fresh), bits(dev.get()))
    torch = pytest.importorskip('torch')
    tens = torch.full(out_shape, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.extract_sum_multi(ms, box, w, output=tens) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    with pytest.raises(ValueError):
        sv.extract_sum_multi(ms, box, w, output=np.zeros(box, np.float32))
    with pytest.raises(ValueError):
        sv.extract_sum_multi(ms, box, w[:-1])
    sv.close()


# ---- 8. edge='scipy' ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_edge_scipy_handle_holds_kernel_13s_bits(interp):
    shape, box = (70, 66, 72), (24, 40, 32)
    ms = batch(shape, box)
    w = weight_matrix(len(ms), 5, seed=23)
    sv = vt.StaticVolume(rand_vol(shape, 27), interpolation=interp, device='gpu:0', edge='scipy')
    for flags in FLAGS:
        got = sv.extract_sum_multi(ms, box, w, _flags=flags)
        assert sv.info().last_kernel == 16 and got.any()
        want = columns_by_kernel_13(sv, ms, box, w, flags)
        assert np.array_equal(bits(got), bits(want)), (interp, flags)
    sv.close()


# ---- 9. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    vol = rand_vol((20, 24, 28), 30)
    m = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    two = np.array([[2.0, 0.5]])
    out = np.zeros((2, 8, 8, 8), np.float32)

    def call(h, n=1, mat=m, g=2, w=two, box=(8, 8, 8)):
        return lib.vt_volume_extract_sum_multi(h, n, mat.ctypes.data, g, None if w is None else w.ctypes.data, *box, out.ctypes.data, 0)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    assert lib.vt_volume_extract_sum_multi_f64(h, 1, m64.ctypes.data, 2, two.ctypes.data, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    assert call(h, n=0) == VT_EINVAL
    assert call(h, g=0) == VT_EINVAL
    assert call(h, w=None) == VT_EINVAL
    bad = m.copy()
    bad[1, 2] = np.nan
    assert call(h, mat=bad) == VT_EINVAL and b'finite' in lib.vt_last_error()
    assert call(h, w=np.array([[1.0, np.inf]])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    assert call(h, box=(0, 8, 8)) == VT_EINVAL
    assert not out.any()
    _native.check(call(h), 'extract_sum_multi')
    info = _native.VolumeInfo()
    _native.check(lib.vt_volume_info(h, ctypes.byref(info)), 'info')
    assert info.last_kernel == 16
    assert np.array_equal(out[0], 2.0 * vol[:8, :8, :8]) and np.array_equal(out[1], 0.5 * vol[:8, :8, :8])
    out[:] = 0
    _native.check(lib.vt_volume_extract_sum_multi_f64(h, 1, m64.ctypes.data, 2, two.ctypes.data, 8, 8, 8, out.ctypes.data, 0), 'extract_sum_multi_f64')
    assert np.array_equal(out[0], 2.0 * vol[:8, :8, :8]) and np.array_equal(out[1], 0.5 * vol[:8, :8, :8])
    lib.vt_volume_destroy(h)


# ---- 10. class_averages_at -----------------------------------------------------------------------------------------------------
def test_class_averages_at():
    box, n, classes = (17, 23, 29), 40, 3
    rs = np.random.RandomState(29)
    pos = rs.uniform(0.2, 0.8, (n, 3)) * np.asarray(SHAPE)
    rot = rs.uniform(0, 360, (n, 3))
    labels = rs.randint(0, classes, n)
    assert set(labels) == set(range(classes))
    sv = vt.StaticVolume(rand_vol(SHAPE, 23), interpolation='filt_bspline', device='gpu:0')
    got = sv.class_averages_at(pos, rot, box, labels=labels, n_classes=classes + 1)
    assert sv.info().last_kernel == 16 and got.shape == (classes + 1,) + box and not got[classes].any()
    own = sv.extract_at(pos, rot, box).astype(np.float64)
    for c in range(classes):
        sel = labels == c
        sub = sv.average_at(pos[sel], rot[sel], box)
        assert sv.info().last_kernel == 13
        # both are one float32 rounding of a float64 sum of the library's own boxes times 1 / n_c, split into different segments: the
        # bound of test_against_the_librarys_own_boxes_and_single_boxes holds for each, hence twice that between them
        ref = own[sel].sum(axis=0) / sel.sum()
        mag = np.abs(own[sel]).sum(axis=0) / sel.sum()
        bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * mag
        for what, a in (('class_averages_at', got[c]), ('average_at', sub)):
            err = np.abs(a.astype(np.float64) - ref)
            print(c, what, f'max err {err.max():.3e}, worst err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}')
            assert (err <= bound).all(), (c, what, float(err.max()))
        assert (np.abs(got[c].astype(np.float64) - sub.astype(np.float64)) <= 2 * bound).all(), c
    # one class that holds every box: average_at's bits
    same = sv.class_averages_at(pos, rot, box, labels=np.zeros(n, int), n_classes=1)
    assert np.array_equal(bits(same), bits(sv.average_at(pos, rot, box)[None]))
    sv.close()
