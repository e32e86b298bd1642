"""-m gpu: StaticVolume.extract_dot / correlate_at (vt_volume_extract_dot, kernel 14) against float64 sums over the oracle's boxes with bounds
derived from the per-voxel tolerance, against sums over the library's own boxes to float64 accumulation error, and bit for bit where the
arithmetic is exact or the contract says so (independence of the batch, determinism, output kinds, split launches)."""
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
ACC = 2.0 ** -40                 # float64 accumulation of up to 1e5 terms, relative to the sum of their magnitudes


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def tiles_of(info, box):
    return int(np.prod([-(-b // t) for b, t in zip(box, info.last_tile)]))


@functools.lru_cache(maxsize=None)
def template_and_mask(box):
    """Template uniform(-1, 1); mask a soft sphere (1 inside 0.7 of the half-diagonal of the inscribed ellipsoid, 0 from 1.0 on: the corners)."""
    tmpl = np.random.RandomState(41).uniform(-1, 1, box).astype(np.float32)
    g = np.meshgrid(*[np.linspace(-1, 1, b) for b in box], indexing='ij')
    r = np.sqrt(sum(x * x for x in g))
    mask = np.clip((1.0 - r) / 0.3, 0, 1).astype(np.float32)
    assert mask[0, 0, 0] == 0 and mask[-1, -1, -1] == 0 and mask.max() == 1 and ((mask > 0) & (mask < 1)).any()
    tmpl.setflags(write=False)
    mask.setflags(write=False)
    return tmpl, mask


def sums_and_bounds(boxes, tmpl, mask, tol):
    """want (n, 3) in float64 from reference boxes, and the bound on |got - want| that follows from |sample - box voxel| <= tol:
    S0: tol sum|mask|;  S1: tol sum|mask| (2|b| + tol);  S2: tol sum|tmpl|;  plus ACC sum|terms| each for the float64 accumulation."""
    b = boxes.astype(np.float64)
    m = np.ones(b.shape[1:]) if mask is None else mask.astype(np.float64)
    t = tmpl.astype(np.float64)
    ax = (1, 2, 3)
    want = np.stack([(m * b).sum(ax), (m * b * b).sum(ax), (t * b).sum(ax)], axis=1)
    mag = np.stack([np.abs(m * b).sum(ax), np.abs(m * b * b).sum(ax), np.abs(t * b).sum(ax)], axis=1)
    bound = np.stack([tol * np.abs(m).sum() * np.ones(len(b)), tol * (np.abs(m) * (2 * np.abs(b) + tol)).sum(ax),
                      tol * np.abs(t).sum() * np.ones(len(b))], axis=1) + ACC * mag
    return want, bound, mag


def check_dot(got, want, bound, what):
    assert got.shape == want.shape and got.dtype == np.float64 and np.isfinite(got).all(), what
    err = np.abs(got - want)
    ratio = err / np.maximum(bound, 1e-300)
    print(what, 'max err per sum', ' '.join(f'{e:.2e}' for e in err.max(0)), ' worst err/bound', ' '.join(f'{r:.3f}' for r in ratio.max(0)))
    assert (err <= bound).all(), (what, float(ratio.max()))


@functools.lru_cache(maxsize=None)
def oracle_case(interp, box):
    """(matrices, oracle boxes) of the batch of test_gpu_extract (24 matrices) out of the SHAPE source: computed once per (interp, box), never modified."""
    ms = batch(SHAPE, box)
    want = oracle_boxes(rand_vol(SHAPE, 21), ms, interp, box)
    want.setflags(write=False)
    ms.setflags(write=False)
    return ms, want


# ---- 1. parity against the oracle ------------------------------------------------------------------------------------
@pytest.mark.parametrize('box', [(17, 23, 29), (40, 48, 56)])
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_parity_against_the_oracle(interp, box):
    ms, boxes = oracle_case(interp, box)
    assert len(ms) >= 24 and not boxes[18].any() and boxes[0].any() and boxes[17].any()    # the outside box is empty, the others are not
    tmpl, mask = template_and_mask(box)
    want, bound, _ = sums_and_bounds(boxes, tmpl, mask, TOL[interp])
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    for flags in FLAGS:
        got = sv.extract_dot(ms, tmpl, mask, _flags=flags)
        info = sv.info()
        assert info.last_kernel == 14, (interp, box, flags, info.last_kernel)
        assert 0 < info.last_lds_bytes <= 160 * 1024 and min(info.last_tile) > 0 and info.last_grid == tiles_of(info, box) * len(ms)
        check_dot(got, want, bound, (interp, box, flags))
        assert np.array_equal(got[18], np.zeros(3)), (interp, box, flags, got[18])      # wholly outside: exactly (0, 0, 0)
    sv.close()


# ---- 2. against the library's own boxes ------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [0, _native.FORCE_TILED])
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline_simple'])
def test_against_the_librarys_own_boxes(interp, flags):
    box = (40, 48, 56)
    big = centred(20.0 * rot3((5, 50, -15)), (48, 50, 52), box).astype(np.float32)       # an entry on the global-gather route
    ms = np.concatenate([batch(SHAPE, box), big[None]])
    tmpl, mask = template_and_mask(box)
    sv = vt.StaticVolume(rand_vol(SHAPE, 23), interpolation=interp, device='gpu:0')
    own = sv.extract(ms, box, _flags=flags)
    assert own[-1].any()
    for m in (mask, None):
        got = sv.extract_dot(ms, tmpl, m, _flags=flags)
        assert sv.info().last_kernel == 14
        want, _, mag = sums_and_bounds(own, tmpl, m, 0.0)
        check_dot(got, want, ACC * mag, (interp, flags, 'own boxes', m is not None))     # the samples are kernel 11's: accumulation error only
        # the 20x-scaled entry fits no LDS box: alone, its launch stages nothing (no LDS dims, the 96 bytes of the reduction only),
        # and its row in the batch holds the same bits -- it took the global gather inside the tiled launch
        alone = sv.extract_dot(ms[-1:], tmpl, m, _flags=flags)
        info = sv.info()
        assert tuple(info.last_lds_dims) == (0, 0, 0) and info.last_lds_bytes == 96, (tuple(info.last_lds_dims), info.last_lds_bytes)
        assert np.array_equal(bits(alone[0]), bits(got[-1]))
        sv.extract_dot(ms[:1], tmpl, m, _flags=flags)
        assert min(sv.info().last_lds_dims) > 0                          # an ordinary rotation stages its box
    sv.close()


# ---- 3. independence and determinism ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_case():
    shape, box, n = (40, 44, 48), (8, 8, 8), 257
    rs = np.random.RandomState(3)
    s = np.asarray(shape, np.float64)
    ms = np.stack([centred(rot3(rs.uniform(0, 360, 3)), rs.uniform(0.15, 0.85, 3) * s, box) for _ in range(n)]).astype(np.float32)
    vol = rand_vol(shape, 31)
    tmpl = rs.uniform(-1, 1, box).astype(np.float32)
    mask = rs.uniform(0, 1, box).astype(np.float32)
    for a in (ms, vol, tmpl, mask):
        a.setflags(write=False)
    return shape, box, vol, ms, tmpl, mask


@pytest.mark.parametrize('flags', [0, _native.FORCE_DIRECT])
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_independence_of_the_batch(interp, flags):
    shape, box, vol, ms, tmpl, mask = small_case()
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    whole = sv.extract_dot(ms, tmpl, mask, _flags=flags).copy()
    assert whole.shape == (257, 3) and (whole[:, 1] > 0).all()
    for n in (1, 2, 25, 257):
        assert np.array_equal(bits(whole[:n]), bits(sv.extract_dot(ms[:n], tmpl, mask, _flags=flags))), (interp, flags, n)
    perm = np.random.RandomState(4).permutation(257)
    assert np.array_equal(bits(whole[perm]), bits(sv.extract_dot(ms[perm], tmpl, mask, _flags=flags)))
    for i in range(0, 257, 16):
        assert np.array_equal(bits(whole[i]), bits(sv.extract_dot(ms[i:i + 1], tmpl, mask, _flags=flags)[0])), (interp, flags, i)
    sv.close()


def test_determinism_and_output_kinds():
    shape, box, vol, ms, tmpl, mask = small_case()
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fresh = sv.extract_dot(ms, tmpl, mask).copy()
    assert np.array_equal(bits(fresh), bits(sv.extract_dot(ms, tmpl, mask)))
    sv.affine(m)
    sv.extract(ms, box)
    sv.extract_sum(ms, box)
    sv.projection_batch(np.stack([m, m]), _flags=_native.FORCE_TILED)
    assert np.array_equal(bits(fresh), bits(sv.extract_dot(ms, tmpl, mask)))
    other = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    assert np.array_equal(bits(fresh), bits(other.extract_dot(ms, tmpl, mask)))
    other.close()
    host = np.full((257, 3), 5.0)
    assert sv.extract_dot(ms, tmpl, mask, output=host) is None
    assert np.array_equal(bits(fresh), bits(host))
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=np.zeros((257, 3), np.float32))
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=np.zeros((256, 3), np.float64))
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=vt.empty((257, 3), device='gpu:0'))      # vt.empty arrays are float32
    sv.close()


def test_torch_float64_device_output_holds_the_same_bits():
    import torch                                                         # the project's plumbing: its absence is a failure, not a skip
    shape, box, vol, ms, tmpl, mask = small_case()
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fresh = sv.extract_dot(ms, tmpl, mask)
    tens = torch.full((257, 3), 5.0, dtype=torch.float64, device='cuda:0')
    assert sv.extract_dot(ms, tmpl, mask, output=tens) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    with pytest.raises(ValueError):
        sv.extract_dot(ms, tmpl, mask, output=torch.zeros((257, 3), dtype=torch.float32, device='cuda:0'))
    sv.close()


# ---- 4. the partial buffer is split ----------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_partials_beyond_the_cap_split_the_call(interp, monkeypatch):
    """The cap on one launch's partials is 64 MiB; VT_DOT_PART_CAP (read when the handle is created) lowers it so that 257 matrices of
    8^3 split into launches of 10 -- the arithmetic per matrix is the same, so the bits are those of the unsplit call and of small batches."""
    shape, box, vol, ms, tmpl, mask = small_case()
    plain = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    want = plain.extract_dot(ms, tmpl, mask).copy()
    info = plain.info()
    tiles = tiles_of(info, box)
    assert info.last_grid == tiles * 257                      # one launch
    small = np.concatenate([plain.extract_dot(ms[i:i + 7], tmpl, mask) for i in range(0, 257, 7)])
    plain.close()
    monkeypatch.setenv('VT_DOT_PART_CAP', str(10 * tiles * 24 + 8))
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    monkeypatch.delenv('VT_DOT_PART_CAP')
    got = sv.extract_dot(ms, tmpl, mask)
    info = sv.info()
    assert info.last_kernel == 14 and info.last_grid == tiles * 7, (info.last_grid, tiles)      # 25 launches of 10 and one of 7
    assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got), bits(small))
    tens_free = sv.extract_dot(ms[:10], tmpl, mask)
    assert sv.info().last_grid == tiles * 10 and np.array_equal(bits(tens_free), bits(want[:10]))
    sv.close()


# ---- 5. known answer, exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_known_answer_integer_crops(flags):
    shape, box = (50, 60, 70), (20, 24, 28)
    rs = np.random.RandomState(24)
    vol = rs.randint(0, 16, shape).astype(np.float32)
    mask = rs.randint(0, 3, box).astype(np.float32)
    tmpl = rs.randint(-3, 4, box).astype(np.float32)
    starts = np.array([[5, 6, 7], [0, 0, 0], [40, 50, 60], [-8, 30, -10], [30, 36, 42], [45, -20, 66], [-30, -30, -30]])
    c = (np.asarray(box) - 1) / 2
    pad = 32
    padded = np.pad(vol, pad, mode='constant').astype(np.float64)
    want = np.zeros((len(starts), 3))
    for i, st in enumerate(starts):
        z, y, x = st + pad
        b = padded[z:z + box[0], y:y + box[1], x:x + box[2]]
        want[i] = (mask * b).sum(), (mask * b * b).sum(), (tmpl * b).sum()      # small integers: exact in any order
    assert not want[6].any() and want[:6, 0].all()
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_dot(vt.utils.box_matrices(starts + c, None, box), tmpl, mask, _flags=flags)
    assert sv.info().last_kernel == 14
    sv.close()
    assert np.array_equal(got, want), (flags, got, want)


@pytest.mark.parametrize('flags', FLAGS)
def test_s1_rounds_the_product_before_the_addition(flags):
    """Two voxels, values chosen so that round(round(m0 b0 b0) + round(m1 b1 b1)) -- the documented expression, what numpy float64 evaluates --
    differs in the last bit from round(round(m0 b0 b0) + m1 b1 b1), what a fused multiply-add would give.  Both voxels belong to one thread
    (planes 0 and 1 of one (h, w) position), every other term of the reduction is 0, so the result is that expression exactly."""
    from fractions import Fraction as F
    b = np.array([float.fromhex('0x1.203ebcp+0'), float.fromhex('0x1.568972p+0')], np.float32)
    m = np.array([float.fromhex('0x1.23f066p-1'), float.fromhex('0x1.32b6c8p-1')], np.float32)
    t = np.array([3.0, -2.0], np.float32)
    b64, m64, t64 = b.astype(np.float64), m.astype(np.float64), t.astype(np.float64)
    mb = m64 * b64                                                       # exact
    r = mb * b64                                                         # rounded once each
    want = np.array([[mb[0] + mb[1], r[0] + r[1], t64[0] * b64[0] + t64[1] * b64[1]]])
    fused = float(F(float(r[0])) + F(float(mb[1])) * F(float(b64[1])))
    assert want[0, 1] != fused                                           # the case tells the two apart
    vol = np.zeros((8, 8, 8), np.float32)
    vol[0, 0, 0], vol[1, 0, 0] = b
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_dot(np.eye(4, dtype=np.float32)[None], t.reshape(2, 1, 1), m.reshape(2, 1, 1), _flags=flags)
    assert sv.info().last_kernel == 14
    sv.close()
    assert np.array_equal(bits(got), bits(want)), (flags, [x.hex() for x in got[0]], [x.hex() for x in want[0]], fused.hex())


# ---- 6. edge='scipy' -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', list(TOL_EDGE))
def test_edge_scipy_handle_equals_cpu_extract_dot(interp):
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 27)
    ms = batch(shape, box)
    tmpl, mask = template_and_mask(box)
    cpu = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    ref_boxes = cpu.extract(ms, box)
    _, bound, _ = sums_and_bounds(ref_boxes, tmpl, mask, TOL_EDGE[interp])
    want = cpu.extract_dot(ms, tmpl, mask)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    for flags in FLAGS:
        check_dot(sv.extract_dot(ms, tmpl, mask, _flags=flags), want, bound, (interp, 'edge=scipy', flags))
    sv.close()


# ---- 7. correlate_at -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_correlate_at_finds_the_true_pose(interp):
    shape, box = (64, 72, 80), (16, 16, 16)
    vol = rand_vol(shape, 33).copy()
    vol[:24, :24, :24] = 0                                               # a constant region (the last pose's box samples [4, 19]^3)
    _, mask = template_and_mask(box)
    rs = np.random.RandomState(34)
    p, r = np.array([40.3, 41.7, 50.2]), np.array([25.0, 40.0, -70.0])
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    template = sv.extract_at(p[None], r[None], box)[0]
    pos = np.concatenate([p[None], p + rs.uniform(-1.5, 1.5, (5, 3)), np.repeat(p[None], 5, 0), rs.uniform(30, 56, (5, 3)), [[11.5, 11.5, 11.5]]])
    rot = np.concatenate([r[None], np.repeat(r[None], 5, 0), r + rs.uniform(-40, 40, (5, 3)), rs.uniform(0, 360, (5, 3)), [[0.0, 0.0, 0.0]]])
    assert len(pos) == 17                                                # the true pose, 15 decoys, the constant region
    for m in (mask, None):
        cc = sv.correlate_at(pos, rot, template, m)
        assert sv.info().last_kernel == 14
        print(interp, m is not None, 'cc', ' '.join(f'{x:.4f}' for x in cc))
        assert cc.shape == (17,) and cc.dtype == np.float64 and np.isfinite(cc).all()
        assert int(np.argmax(cc)) == 0 and cc[0] >= 1 - 1e-5 and cc[0] <= 1 + 1e-5 and (cc[1:16] < cc[0]).all()
        assert cc[16] == 0.0 or interp.startswith('filt')                # a box of zeros has no variance: exactly 0, not NaN
    sv.close()
    # the prefilter of filt_bspline is recursive (its coefficients near the constant region's border are tiny, not zero): for the cubic
    # kernels the same statement is made on a volume that is zero everywhere
    flat = vt.StaticVolume(np.zeros(shape, np.float32), interpolation=interp, device='gpu:0')
    for m in (mask, None):
        assert np.array_equal(flat.correlate_at(pos, rot, template, m), np.zeros(17))
    flat.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    rs = np.random.RandomState(30)
    vol = rs.randint(0, 16, (20, 24, 28)).astype(np.float32)
    tmpl = rs.randint(-3, 4, (8, 8, 8)).astype(np.float32)
    ones = np.ones((8, 8, 8), np.float32)
    m = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    out = np.full((1, 3), 7.0)

    def call(h, n=1, mat=m, t=tmpl, k=ones, box=(8, 8, 8)):
        return lib.vt_volume_extract_dot(h, n, mat.ctypes.data, None if t is None else t.ctypes.data, None if k is None else k.ctypes.data,
                                         *box, out.ctypes.data, 0)

    def refused(rc, word=None):
        msg = lib.vt_last_error()
        return rc == VT_EINVAL and msg and (word is None or word in msg)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert refused(call(h), b'slab')
    assert refused(lib.vt_volume_extract_dot_f64(h, 1, m64.ctypes.data, tmpl.ctypes.data, None, 8, 8, 8, out.ctypes.data, 0), b'slab')
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert refused(call(h), b'finalize')
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    assert refused(call(h, n=0))
    bad = m.copy()
    bad[1, 2] = np.nan
    assert refused(call(h, mat=bad), b'finite')
    inf = tmpl.copy()
    inf[3, 4, 5] = np.inf
    assert refused(call(h, t=inf), b'template')
    nan = ones.copy()
    nan[7, 7, 7] = np.nan
    assert refused(call(h, k=nan), b'mask')
    assert refused(call(h, box=(8, 0, 8)))
    assert refused(call(h, t=None))
    assert np.array_equal(out, np.full((1, 3), 7.0))                     # no refusal wrote anything
    b = vol[:8, :8, :8].astype(np.float64)
    want = np.array([[b.sum(), (b * b).sum(), (tmpl * b).sum()]])
    _native.check(call(h), 'extract_dot')
    assert np.array_equal(out, want)
    out[...] = 7.0
    _native.check(call(h, k=None), 'extract_dot without a mask')
    assert np.array_equal(out, want)
    out[...] = 7.0
    _native.check(lib.vt_volume_extract_dot_f64(h, 1, m64.ctypes.data, tmpl.ctypes.data, ones.ctypes.data, 8, 8, 8, out.ctypes.data, 0), 'extract_dot_f64')
    assert np.array_equal(out, want)
    lib.vt_volume_destroy(h)


# ---- 9. handle untouched ---------------------------------------------------------------------------------------------
def test_handle_is_untouched():
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 25)
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    tmpl, mask = template_and_mask(box)
    sv = vt.StaticVolume(vol, interpolation='bspline', device='gpu:0')
    before = sv.affine(m).copy()
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    ms = batch(shape, box)
    assert sv.extract_dot(ms, tmpl, mask).shape == (len(ms), 3)
    info = sv.info()
    assert (info.out_depth, info.out_height, info.out_width) == dims == shape
    after = sv.affine(m)
    assert after.shape == shape and np.array_equal(before.view(np.uint32), after.view(np.uint32))
    assert sv.affine_batch(np.stack([m, m])).shape == (2,) + shape and sv.projection(m).shape == shape[1:]
    sv.close()
