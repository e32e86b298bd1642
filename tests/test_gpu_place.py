"""-m gpu: StaticVolume.place / place_at (vt_volume_place, kernel 17) against the float64 weighted sum of the oracle's volumes on every
voxel, bit for bit against kernel 13 (extract_sum with the output as the box, one segment), bit for bit between the sparse lists and the
diagnostic dense ones, against the library's own boxes to one float32 rounding, and the accumulate mode down to the untouched bits."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, batch, centred, rot3, oracle_boxes, rand_vol

pytestmark = pytest.mark.gpu

TSHAPE = (20, 24, 28)                  # the small map the handle holds
OUT = (48, 56, 72)
DENSE = _native.PLACE_DENSE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tiles_of(info, shape):
    return int(np.prod([-(-b // t) for b, t in zip(shape, info.last_tile)]))


def placed(m3, out_pos, tshape=TSHAPE):
    """4x4 float64 pull matrix (output index -> map coordinate) with linear part m3 under which output position out_pos samples
    the centre of the map."""
    c = (np.asarray(tshape, np.float64) - 1) / 2
    m = np.eye(4)
    m[:3, :3] = m3
    m[:3, 3] = c - np.asarray(m3, np.float64) @ np.asarray(out_pos, np.float64)
    return m


def place_batch(out=OUT, tshape=TSHAPE, seed=4):
    """14 float32 matrices: five random rotations at fractional positions (the first two overlap), a copy over each of two faces and one
    corner, one entirely outside (index 8), scale 2 and 0.5, a mirror, a shear, the identity at an integer offset (index 13)."""
    rs = np.random.RandomState(seed)
    o = np.asarray(out, np.float64)
    mid = (o - 1) / 2
    ms = [placed(rot3(rs.uniform(0, 360, 3)), mid + (-6.3, 4.25, -9.5), tshape),
          placed(rot3(rs.uniform(0, 360, 3)), mid + (-1.75, 7.5, -4.2), tshape)]
    for _ in range(3):
        ms.append(placed(rot3(rs.uniform(0, 360, 3)), rs.uniform(0.2, 0.8, 3) * o, tshape))
    ms.append(placed(rot3(rs.uniform(-30, 30, 3)), (0.3, mid[1] + 2.2, mid[2] - 1.4), tshape))                 # over the d = 0 face
    ms.append(placed(rot3(rs.uniform(-30, 30, 3)), (mid[0] - 1.1, mid[1] + 0.6, o[2] - 1 + 0.2), tshape))       # over the w = end face
    ms.append(placed(rot3((20, 35, -50)), o - 1 + (0.25, -0.5, 0.75), tshape))                                  # corner
    ms.append(placed(rot3((10, 20, 30)), o + 2.0 * np.asarray(tshape) + 5.0, tshape))                           # entirely outside
    ms.append(placed(2.0 * rot3((15, -25, 40)), mid + (10.3, -12.6, 20.4), tshape))                             # scale 2: a half-size copy
    ms.append(placed(0.5 * rot3((-35, 10, 60)), mid - 0.7, tshape))                                             # scale 0.5: double size
    ms.append(placed(np.diag([-1.0, 1.0, -1.0]), mid + (0.5, 0.25, -0.25), tshape))                            # mirror
    sh = np.eye(3)
    sh[0, 1], sh[0, 2], sh[1, 2] = 0.2, -0.15, 0.3
    ms.append(placed(sh, mid + 0.4, tshape))                                                                    # shear
    ident = np.eye(4)
    ident[:3, 3] = -np.asarray(IDENT_START, np.float64)
    ms.append(ident)                                                                                            # identity at an integer offset
    return np.ascontiguousarray(np.stack(ms), dtype=np.float32)


IDENT_START = (5, 30, 40)
OUTSIDE, IDENT = 8, 13
WEIGHTS = np.array([0.75, -1.5, 2.0, 0.0, 1.25, -0.5, 1.0, 0.6, 1.5, -2.0, 0.35, 1.0, -0.8, 1.0])       # mixed signs, one exact 0


@functools.lru_cache(maxsize=None)
def oracle_case(interp):
    """(matrices, float64 oracle volumes) of place_batch: computed once per interpolation, never modified."""
    ms = place_batch()
    want = oracle_boxes(rand_vol(TSHAPE, 21), ms, interp, OUT).astype(np.float64)
    want.setflags(write=False)
    ms.setflags(write=False)
    return ms, want


def check_sum(got, vols, w, tol, what):
    """|got - sum_i w_i A_i| <= sum|w_i| * tol + 2^-23 |want| (check_sum of test_gpu_extract_sum.py)."""
    want = np.tensordot(w, vols, axes=1)
    bound = np.abs(w).sum() * tol + 2.0 ** -23 * np.abs(want)
    err = np.abs(got.astype(np.float64) - want)
    print(what, f'max|hip-oracle| {err.max():.3e}  min(bound) {bound.min():.3e}  worst ratio {(err / bound).max():.3f}')
    assert got.shape == want.shape and got.dtype == np.float32 and np.isfinite(got).all(), what
    assert (err <= bound).all(), (what, float((err / bound).max()))


def own_reference(sv, ms, w, shape, base=None, chunk=50):
    """(float64 sum_i w_i A_i [+ base], sum_i |w_i| |A_i| [+ |base|], voxels some copy reaches) from the library's own extract volumes."""
    ref = np.zeros(shape, np.float64) if base is None else base.astype(np.float64)
    mag = np.abs(ref)
    reached = np.zeros(shape, bool)
    for a in range(0, len(ms), chunk):
        own = sv.extract(ms[a:a + chunk], shape)
        for k in range(own.shape[0]):
            one = own[k].astype(np.float64)
            ref += w[a + k] * one
            mag += abs(w[a + k]) * np.abs(one)
            reached |= one != 0
    return ref, mag, reached


def check_own(got, ref, mag, what):
    """One correct float32 rounding + float64 accumulation error: the "own boxes" bound of test_gpu_extract_sum.py."""
    err = np.abs(got.astype(np.float64) - ref)
    bound = 2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * mag
    print(what, f'max err {err.max():.3e}, worst err/bound {(err / np.maximum(bound, 1e-300)).max():.3f}')
    assert (err <= bound).all(), (what, float(err.max()))


# ---- 1. parity against the oracle on every voxel -----------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_parity_against_the_oracle(interp):
    ms, vols = oracle_case(interp)
    assert len(ms) == 14 and not vols[OUTSIDE].any() and all(vols[i].any() for i in range(14) if i != OUTSIDE)
    assert ((vols[0] != 0) & (vols[1] != 0)).any()                              # two copies overlap
    w = WEIGHTS
    w_other = w.copy()
    w_other[OUTSIDE] = 1000.0
    sv = vt.StaticVolume(rand_vol(TSHAPE, 21), interpolation=interp, device='gpu:0')
    for flags in (0, _native.FORCE_DIRECT, DENSE):
        got = sv.place(ms, OUT, w, _flags=flags)
        info = sv.info()
        assert info.last_kernel == 17, (interp, flags, info.last_kernel)
        assert info.last_lds_bytes <= 160 * 1024 and min(info.last_tile) > 0 and 0 < info.last_grid <= tiles_of(info, OUT)
        if flags == DENSE:
            assert info.last_grid == tiles_of(info, OUT)
        check_sum(got, vols, w, TOL[interp], (interp, flags))
        # the copy that lies entirely outside contributes nothing, whatever its weight
        assert np.array_equal(bits(got), bits(sv.place(ms, OUT, w_other, _flags=flags))), (interp, flags)
    sv.close()


@pytest.mark.parametrize('flags', [0, _native.FORCE_DIRECT, DENSE])
def test_integer_offset_identity_reproduces_the_map(flags):
    vol = rand_vol(TSHAPE, 21)
    ms = place_batch()
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.place(ms[IDENT:IDENT + 1], OUT, [1.0], _flags=flags)
    assert sv.info().last_kernel == 17
    sv.close()
    want = np.zeros(OUT, np.float32)
    z, y, x = IDENT_START
    crop = vol[:OUT[0] - z, :OUT[1] - y, :OUT[2] - x]
    want[z:z + crop.shape[0], y:y + crop.shape[1], x:x + crop.shape[2]] = crop
    assert crop.shape[0] == TSHAPE[0] and crop.shape[1] > 0 and crop.shape[2] > 0
    assert np.array_equal(bits(got), bits(want)), flags


# ---- 2. bit identity with kernel 13 ----------------------------------------------------------------------------------------
BIG_T, BIG_OUT = (40, 44, 48), (160, 160, 176)


def kernel13_batch():
    """25 matrices: the batch of the extraction tests with the output as the box, plus one on the global-gather route (own_batch)."""
    ms = batch(BIG_T, BIG_OUT)[:24]
    big = centred(20.0 * rot3((5, 50, -15)), (18, 20, 22), BIG_OUT).astype(np.float32)
    return np.concatenate([ms, big[None]])


@pytest.mark.parametrize('interp,edge', [('linear', 'texture'), ('bspline', 'texture'), ('filt_bspline_simple', 'texture'),
                                         ('bspline', 'scipy')])
def test_bit_identity_with_extract_sum_in_one_segment(interp, edge):
    ms = kernel13_batch()
    assert len(ms) == 25
    w = np.random.RandomState(5).uniform(-1, 2, 25)
    w[3] = 0
    sv = vt.StaticVolume(rand_vol(BIG_T, 23), interpolation=interp, device='gpu:0', edge=edge)
    want = sv.extract_sum(ms, BIG_OUT, w)
    info = sv.info()
    assert info.last_kernel == 13 and info.last_grid == tiles_of(info, BIG_OUT) >= 1024          # one segment
    tile13 = tuple(info.last_tile)
    alone = sv.extract_sum(ms[24:], BIG_OUT)
    assert alone.any()                                                                           # the global-gather entry lands
    for flags in (0, DENSE, _native.FORCE_TILED):
        got = sv.place(ms, BIG_OUT, w, _flags=flags)
        info = sv.info()
        assert info.last_kernel == 17 and tuple(info.last_tile) == tile13
        assert np.array_equal(bits(got + 0.0), bits(want + 0.0)), (interp, edge, flags)
    want_direct = sv.extract_sum(ms, BIG_OUT, w, _flags=_native.FORCE_DIRECT)
    got = sv.place(ms, BIG_OUT, w, _flags=_native.FORCE_DIRECT)
    assert np.array_equal(bits(got + 0.0), bits(want_direct + 0.0)), (interp, edge, 'direct')
    sv.close()


# ---- 3. the lists never drop a contributor ---------------------------------------------------------------------------------
def odd_batch(out, tshape):
    """A rotated copy, a matrix with a zero row (singular) and a 1e-7-scaled one (every output voxel samples next to the map's centre)."""
    o = np.asarray(out, np.float64)
    sing = placed(rot3((25, -40, 10)), (o - 1) / 2 + 0.3, tshape)
    sing[1, :3] = 0.0
    sing[1, 3] = 7.25
    return np.stack([placed(rot3((12, 33, -47)), (o - 1) / 2 - 0.6, tshape), sing,
                     placed(1e-7 * rot3((40, 5, -70)), (o - 1) / 2, tshape)]).astype(np.float32)


LIST_CASES = {
    'batch of 1': (TSHAPE, (64, 72, 80), lambda: place_batch((64, 72, 80))[2:3]),
    'smaller than one tile': (TSHAPE, (5, 7, 9), lambda: place_batch((5, 7, 9))[[0, 1, 9, 10, 12]]),
    'no multiple of the tile': (TSHAPE, (33, 47, 70), lambda: place_batch((33, 47, 70))),
    'map larger than the output': ((40, 44, 48), (17, 23, 29), lambda: place_batch((17, 23, 29), (40, 44, 48))[:13]),
    'singular and tiny': (TSHAPE, (33, 47, 70), lambda: odd_batch((33, 47, 70), TSHAPE)),
}


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
@pytest.mark.parametrize('case', list(LIST_CASES))
def test_sparse_lists_equal_dense_lists(case, interp):
    tshape, out, make = LIST_CASES[case]
    ms = make()
    w = np.random.RandomState(6).uniform(-1, 2, len(ms))
    sv = vt.StaticVolume(rand_vol(tshape, 24), interpolation=interp, device='gpu:0')
    for flags in (0, _native.FORCE_DIRECT):
        sparse = sv.place(ms, out, w, _flags=flags)
        info = sv.info()
        grid, total = info.last_grid, tiles_of(info, out)
        assert info.last_kernel == 17 and 0 < grid <= total
        if case == 'batch of 1':
            assert grid < total, (grid, total)
        dense = sv.place(ms, out, w, _flags=flags | DENSE)
        assert sv.info().last_grid == total
        assert sparse.any() and np.array_equal(bits(sparse), bits(dense)), (case, interp, flags)
        for i in range(len(ms)):                                         # ... and for every entry on its own
            one = sv.place(ms[i:i + 1], out, w[i:i + 1], _flags=flags)
            g = sv.info().last_grid
            assert np.array_equal(bits(one), bits(sv.place(ms[i:i + 1], out, w[i:i + 1], _flags=flags | DENSE))), (case, interp, flags, i)
            assert g > 0 or not one.any(), (case, i)
    sv.close()


# ---- 4. long lists ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_long_lists_against_the_librarys_own_boxes(interp):
    tshape, out, n = (8, 8, 8), (64, 64, 64), 300
    rs = np.random.RandomState(8)
    pos = rs.uniform(-2, 66, (n, 3))
    rot = rs.uniform(0, 360, (n, 3))
    w = rs.uniform(-1, 2, n)
    ms = vt.utils.place_matrices(pos, rot, tshape, rotation_order='sxyz')
    sv = vt.StaticVolume(rand_vol(tshape, 25), interpolation=interp, device='gpu:0')
    got = sv.place_at(pos, rot, out, w, rotation_order='sxyz')
    info = sv.info()
    assert info.last_kernel == 17 and 0 < info.last_grid <= tiles_of(info, out)
    assert np.array_equal(bits(got), bits(sv.place(ms, out, w)))
    ref, mag, reached = own_reference(sv, ms, w, out)
    assert reached.mean() > 0.2
    check_own(got, ref, mag, (interp, 'n = 300'))
    assert np.array_equal(bits(got), bits(sv.place(ms, out, w, _flags=DENSE)))
    sv.close()


# ---- 5. accumulate -----------------------------------------------------------------------------------------------------------
def accumulate_case():
    out = (64, 72, 80)
    ms = np.stack([placed(rot3((10, 20, 30)), (14.3, 15.6, 18.2)), placed(rot3((-40, 15, 80)), (20.5, 22.25, 25.0)),
                   placed(rot3((5, 50, -15)), (-3.0, 14.0, 30.5))]).astype(np.float32)             # all near the low corner
    w = np.array([1.5, -0.75, 2.0])
    base = np.random.RandomState(9).standard_normal(out).astype(np.float32)
    base[60, 70, 77], base[50, 60, 70], base[63, 71, 79], base[40, 10, 75] = np.nan, np.inf, -0.0, -np.inf
    return out, ms, w, base


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_accumulate(interp):
    out, ms, w, base = accumulate_case()
    sv = vt.StaticVolume(rand_vol(TSHAPE, 26), interpolation=interp, device='gpu:0')
    ref, mag, reached = own_reference(sv, ms, w, out, base=base)
    assert reached.any() and not reached[44:].any() and not reached[:, :, 56:].any()
    host = base.copy()
    assert sv.place(ms, out, w, output=host, accumulate=True) is None
    info = sv.info()
    assert info.last_kernel == 17 and 0 < info.last_grid < tiles_of(info, out)
    # no copy reaches: every bit as found (NaN, Inf and -0 included); elsewhere double(base) + the sum, rounded once
    assert np.array_equal(bits(host)[~reached], bits(base)[~reached])
    assert np.isnan(host[60, 70, 77]) and bits(host)[63, 71, 79] == 0x80000000
    err = np.abs(host[reached].astype(np.float64) - ref[reached])
    bound = (2.0 ** -24 * np.abs(ref) + 2.0 ** -40 * mag)[reached]
    print(interp, f'accumulate: max err {err.max():.3e}, worst err/bound {(err / bound).max():.3f}')
    assert (err <= bound).all() and not np.array_equal(bits(host)[reached], bits(base)[reached])
    # device output, dense lists: the same bits
    dev = vt.empty(out, device='gpu:0')
    dev.set(base)
    assert sv.place(ms, out, w, output=dev, accumulate=True) is None
    sv.synchronize()
    assert np.array_equal(bits(dev.get()), bits(host))
    dense = base.copy()
    sv.place(ms, out, w, output=dense, accumulate=True, _flags=DENSE)
    assert np.array_equal(bits(dense), bits(host))
    # every copy outside: nothing is launched, nothing changes
    far = np.stack([placed(rot3((10, 20, 30)), (200.0, 300.0, -150.0)), placed(np.eye(3), (-40.0, 30.0, 30.0))]).astype(np.float32)
    for target in (base.copy(), None):
        if target is None:
            dev.set(base)
        sv.place(far, out, [1.0, -2.0], output=dev if target is None else target, accumulate=True)
        sv.synchronize()
        assert sv.info().last_kernel == 17 and sv.info().last_grid == 0
        assert np.array_equal(bits(dev.get() if target is None else target), bits(base))
    with pytest.raises(ValueError):
        sv.place(ms, out, w, accumulate=True)
    sv.close()


# ---- 6. nothing to do ----------------------------------------------------------------------------------------------------------
def test_nothing_to_do_then_an_ordinary_call():
    out = (33, 47, 70)
    sv = vt.StaticVolume(rand_vol(TSHAPE, 27), interpolation='bspline', device='gpu:0')
    far = np.stack([placed(rot3((10, 20, 30)), (200.0, 300.0, -150.0)), placed(np.eye(3), (-40.0, 30.0, 30.0))]).astype(np.float32)
    host = np.full(out, 5, np.float32)
    assert sv.place(far, out, output=host) is None
    assert sv.info().last_kernel == 17 and sv.info().last_grid == 0
    assert not bits(host).any()                                          # all +0
    dev = vt.empty(out, device='gpu:0')
    dev.set(np.full(out, 5, np.float32))
    sv.place(far, out, output=dev)
    sv.synchronize()
    assert sv.info().last_grid == 0 and not bits(dev.get()).any()
    got = sv.place(far, out)
    assert got.shape == out and not bits(got).any()
    ms = place_batch(out)
    got = sv.place(ms, out, WEIGHTS)
    assert sv.info().last_grid > 0 and got.any()
    ref, mag, _ = own_reference(sv, ms, WEIGHTS, out)
    check_own(got, ref, mag, 'after an empty call')
    sv.close()


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------
def test_determinism_and_output_kinds():
    ms, w = place_batch(), WEIGHTS
    c = np.divide(np.subtract(TSHAPE, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(rand_vol(TSHAPE, 28), interpolation='filt_bspline', device='gpu:0')
    fresh = sv.place(ms, OUT, w).copy()
    assert fresh.shape == OUT and fresh.dtype == np.float32 and fresh.any()
    assert np.array_equal(bits(fresh), bits(sv.place(ms, OUT, w)))
    sv.affine(m)
    sv.extract(ms[:3], (9, 10, 11))
    assert np.array_equal(bits(fresh), bits(sv.place(ms, OUT, w)))
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    assert dims == TSHAPE                                                # the handle's own output shape is untouched
    fresh_sv = vt.StaticVolume(rand_vol(TSHAPE, 28), interpolation='filt_bspline', device='gpu:0')
    assert np.array_equal(bits(fresh), bits(fresh_sv.place(ms, OUT, w)))
    fresh_sv.close()
    host = np.full(OUT, 5, np.float32)
    assert sv.place(ms, OUT, w, output=host) is None
    dev = vt.empty(OUT, device='gpu:0')
    dev.set(np.full(OUT, 5, np.float32))
    assert sv.place(ms, OUT, w, output=dev) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(host)) and np.array_equal(bits(fresh), bits(dev.get()))
    assert np.array_equal(bits(fresh), bits(sv.place(ms.astype(np.float64), OUT, w)))          # the float64 entry point, same values
    torch = pytest.importorskip('torch')
    tens = torch.full(OUT, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.place(ms, OUT, w, output=tens) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    with pytest.raises(ValueError):
        sv.place(ms, OUT, w, output=np.zeros((48, 56, 73), np.float32))
    with pytest.raises(ValueError):
        sv.place(ms, OUT, w[:-1])
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_disjoint_copies_in_any_order(interp):
    out = (96, 96, 96)
    rs = np.random.RandomState(11)
    pos = np.array([[24 + 48 * a, 24 + 48 * b, 24 + 48 * c] for a in range(2) for b in range(2) for c in range(2)], np.float64)
    pos += rs.uniform(-1, 1, pos.shape)
    rot = rs.uniform(0, 360, pos.shape)        # the map's half diagonal is 20.9 voxels: footprints 48 apart are disjoint
    w = rs.uniform(-1, 2, len(pos))
    sv = vt.StaticVolume(rand_vol(TSHAPE, 29), interpolation=interp, device='gpu:0')
    first = sv.place_at(pos, rot, out, w).copy()
    assert first.any()
    for seed in range(3):
        perm = np.random.RandomState(seed).permutation(len(pos))
        assert np.array_equal(bits(first), bits(sv.place_at(pos[perm], rot[perm], out, w[perm]))), (interp, seed)
    sv.close()


# ---- 8. refusals through the C ABI ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    vol = rand_vol((20, 24, 28), 30)
    m = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    one = np.ones(1)
    out = np.zeros((8, 8, 8), np.float32)

    def call(h, n=1, mat=m, w=one, shape=(8, 8, 8), flags=0):
        return lib.vt_volume_place(h, n, mat.ctypes.data, None if w is None else w.ctypes.data, *shape, out.ctypes.data, flags)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    assert lib.vt_volume_place_f64(h, 1, m64.ctypes.data, None, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    assert call(h, n=0) == VT_EINVAL
    assert call(h, n=-3) == VT_EINVAL
    bad = m.copy()
    bad[1, 2] = np.nan
    assert call(h, mat=bad) == VT_EINVAL and b'finite' in lib.vt_last_error()
    assert call(h, w=np.array([np.inf])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    assert call(h, shape=(0, 8, 8)) == VT_EINVAL
    assert call(h, shape=(8, -1, 8)) == VT_EINVAL
    _native.check(call(h, w=np.array([2.0])), 'place')
    assert np.array_equal(out, 2.0 * vol[:8, :8, :8])
    _native.check(call(h, w=None, flags=_native.ACCUMULATE), 'place, accumulating, without weights')
    assert np.array_equal(out, 3.0 * vol[:8, :8, :8])
    _native.check(lib.vt_volume_place_f64(h, 1, m64.ctypes.data, one.ctypes.data, 8, 8, 8, out.ctypes.data, _native.KEEP_OUTSIDE), 'place_f64')
    assert np.array_equal(out, vol[:8, :8, :8])
    lib.vt_volume_destroy(h)
