"""-m gpu: StaticVolume.extract_dot_multi / correlate_templates_at (vt_volume_extract_dot_multi, kernel 15): bit for bit the columns of
extract_dot (kernel 14) per template on every route, against float64 sums over the oracle's boxes, independent of the batch and of the
stack of templates, deterministic across output kinds and handles, split launches, exact known answers, refusals, edge='scipy'."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, TOL_EDGE, ALL_INTERPS, VT_EINVAL, batch, centred, rot3, oracle_boxes, rand_vol
from test_gpu_extract_dot import FLAGS, bits, check_dot, small_case, sums_and_bounds, template_and_mask, tiles_of

pytestmark = pytest.mark.gpu

SHAPE = (96, 100, 104)
K = 9                            # no multiple of 2, 4 or 8, and 2 + K = 11 columns are no multiple of 3 (the kernel serves three columns per pass): a ragged last group


@functools.lru_cache(maxsize=None)
def templates_of(box, seed=43, k=K):
    t = np.random.RandomState(seed).uniform(-1, 1, (k,) + tuple(box)).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def bit_case(box):
    """batch() plus the 20x-scaled entry of test_against_the_librarys_own_boxes (the global gather inside a tiled launch)."""
    big = centred(20.0 * rot3((5, 50, -15)), (48, 50, 52), box).astype(np.float32)
    ms = np.concatenate([batch(SHAPE, box), big[None]])
    ms.setflags(write=False)
    return ms


def launch_facts(info):
    return info.last_grid, tuple(info.last_tile), tuple(info.last_lds_dims), info.last_lds_bytes


def assert_columns_are_kernel_14s(sv, ms, tmpls, mask, flags, what):
    """Every template column, and both mask columns, hold extract_dot's bits; the launch is reported as extract_dot's, kernel apart."""
    singles = []
    for j in range(len(tmpls)):
        singles.append(sv.extract_dot(ms, tmpls[j], mask, _flags=flags))
        assert sv.info().last_kernel == 14
    facts = launch_facts(sv.info())
    multi = sv.extract_dot_multi(ms, tmpls, mask, _flags=flags)
    info = sv.info()
    assert info.last_kernel == 15, (what, info.last_kernel)
    assert launch_facts(info) == facts, (what, launch_facts(info), facts)
    assert multi.shape == (len(ms), 2 + len(tmpls)) and multi.dtype == np.float64
    for j, single in enumerate(singles):
        assert np.array_equal(bits(multi[:, :2]), bits(single[:, :2])), (what, j, 'mask sums')
        assert np.array_equal(bits(multi[:, 2 + j]), bits(single[:, 2])), (what, j, 'template sum')
    return multi


# ---- 1. bit identity with kernel 14 ----------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_bit_identity_with_kernel_14(interp, flags):
    box = (17, 23, 29)                                                   # cut tiles on all three axes for both tile shapes
    ms = bit_case(box)
    tmpls = templates_of(box)
    _, mask = template_and_mask(box)
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    for m in (mask, None):
        multi = assert_columns_are_kernel_14s(sv, ms, tmpls, m, flags, (interp, flags, m is not None))
        assert bits(multi[18]).tolist() == [0] * (2 + K), multi[18]     # wholly outside: a row of exact +0
        assert multi[-1].all() and multi[0].all()                        # the global-gather entry and an ordinary one are scored
    sv.close()


@pytest.mark.parametrize('flags', FLAGS)
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_bit_identity_with_kernel_14_whole_tiles(interp, flags):
    box = (40, 48, 56)                                                   # several whole tiles
    ms = bit_case(box)
    tmpls = templates_of(box)
    _, mask = template_and_mask(box)
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    for m in (mask, None):
        multi = assert_columns_are_kernel_14s(sv, ms, tmpls, m, flags, (interp, flags, m is not None))
        assert bits(multi[18]).tolist() == [0] * (2 + K), multi[18]
    sv.close()


# ---- 2. parity against the oracle (independent of kernel 14) ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def oracle_case(interp, box):
    ms = batch(SHAPE, box)
    want = oracle_boxes(rand_vol(SHAPE, 21), ms, interp, box)
    want.setflags(write=False)
    ms.setflags(write=False)
    return ms, want


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_parity_against_the_oracle(interp):
    box = (17, 23, 29)
    ms, boxes = oracle_case(interp, box)
    assert not boxes[18].any() and boxes[0].any() and boxes[17].any()
    tmpls = templates_of(box)
    _, mask = template_and_mask(box)
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation=interp, device='gpu:0')
    for flags in FLAGS:
        got = sv.extract_dot_multi(ms, tmpls, mask, _flags=flags)
        assert sv.info().last_kernel == 15 and got.shape == (len(ms), 2 + K)
        for j in range(K):
            want, bound, _ = sums_and_bounds(boxes, tmpls[j], mask, TOL[interp])
            check_dot(got[:, [0, 1, 2 + j]], want, bound, (interp, flags, 'template', j))
    sv.close()


# ---- 3. independence of the batch and of the stack -------------------------------------------------------------------
@pytest.mark.parametrize('flags', [0, _native.FORCE_DIRECT])
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_independence_of_the_batch_and_of_the_stack(interp, flags):
    shape, box, vol, ms, _, mask = small_case()
    tmpls = templates_of(box, 44)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    whole = sv.extract_dot_multi(ms, tmpls, mask, _flags=flags).copy()
    assert whole.shape == (257, 2 + K) and (whole[:, 1] > 0).all() and whole[:, 2:].all()
    for n in (1, 2, 25, 257):
        assert np.array_equal(bits(whole[:n]), bits(sv.extract_dot_multi(ms[:n], tmpls, mask, _flags=flags))), (interp, flags, n)
    perm = np.random.RandomState(4).permutation(257)
    assert np.array_equal(bits(whole[perm]), bits(sv.extract_dot_multi(ms[perm], tmpls, mask, _flags=flags)))
    for i in range(0, 257, 16):
        assert np.array_equal(bits(whole[i]), bits(sv.extract_dot_multi(ms[i:i + 1], tmpls, mask, _flags=flags)[0])), (interp, flags, i)
    swapped = np.arange(K)
    swapped[[1, 7]] = 7, 1
    for sel in ([4, 0], [0], swapped.tolist()):
        got = sv.extract_dot_multi(ms, tmpls[sel], mask, _flags=flags)
        assert got.shape == (257, 2 + len(sel))
        assert np.array_equal(bits(got[:, :2]), bits(whole[:, :2])), (interp, flags, sel)
        assert np.array_equal(bits(got[:, 2:]), bits(whole[:, [2 + j for j in sel]])), (interp, flags, sel)
    sv.close()


# ---- 4. determinism and output kinds ---------------------------------------------------------------------------------
def test_determinism_and_output_kinds():
    shape, box, vol, ms, tmpl, mask = small_case()
    tmpls = templates_of(box, 44)
    c = np.divide(np.subtract(shape, 1), 2, dtype=np.float32)
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), translation=(1.5, -2, 0.25), center=c)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fresh = sv.extract_dot_multi(ms, tmpls, mask).copy()
    assert np.array_equal(bits(fresh), bits(sv.extract_dot_multi(ms, tmpls, mask)))
    host = np.full((257, 2 + K), 5.0)
    assert sv.extract_dot_multi(ms, tmpls, mask, output=host) is None
    assert np.array_equal(bits(fresh), bits(host))
    sv.affine(m)
    sv.extract(ms, box)
    sv.extract_sum(ms, box)
    sv.extract_dot(ms, tmpl, mask)
    sv.projection_batch(np.stack([m, m]), _flags=_native.FORCE_TILED)
    assert np.array_equal(bits(fresh), bits(sv.extract_dot_multi(ms, tmpls, mask)))
    other = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    assert np.array_equal(bits(fresh), bits(other.extract_dot_multi(ms, tmpls, mask)))
    other.close()
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, mask, output=np.zeros((257, 2 + K), np.float32))
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, mask, output=np.zeros((257, 3), np.float64))
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, mask, output=vt.empty((257, 2 + K), device='gpu:0'))      # vt.empty arrays are float32
    sv.close()


def test_torch_float64_device_output_holds_the_same_bits():
    import torch                                                         # the project's plumbing: its absence is a failure, not a skip
    shape, box, vol, ms, _, mask = small_case()
    tmpls = templates_of(box, 44)
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    fresh = sv.extract_dot_multi(ms, tmpls, mask)
    tens = torch.full((257, 2 + K), 5.0, dtype=torch.float64, device='cuda:0')
    assert sv.extract_dot_multi(ms, tmpls, mask, output=tens) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    assert np.array_equal(bits(fresh), bits(sv.extract_dot_multi(ms, tmpls, mask)))
    with pytest.raises(ValueError):
        sv.extract_dot_multi(ms, tmpls, mask, output=torch.zeros((257, 2 + K), dtype=torch.float32, device='cuda:0'))
    sv.close()


# ---- 5. the partial buffer is split ----------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_partials_beyond_the_cap_split_the_call(interp, monkeypatch):
    """VT_DOT_PART_CAP (read when the handle is created) is lowered to one matrix's partials of 2 + K columns (25 launches for n = 25), to
    eight bytes less than that (still one matrix per launch) and to seven matrices' worth (three launches of 7 and one of 4): the
    arithmetic per matrix is the same, so the bits are those of the unsplit call on a handle with the default cap."""
    shape, box, vol, ms, _, mask = small_case()
    ms = ms[:25]
    tmpls = templates_of(box, 44)
    plain = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    want = plain.extract_dot_multi(ms, tmpls, mask).copy()
    info = plain.info()
    tiles = tiles_of(info, box)
    assert info.last_grid == tiles * 25                       # one launch
    plain.close()
    part_one = tiles * (2 + K) * 8
    for cap, last in ((part_one, 1), (part_one - 8, 1), (7 * part_one + 8, 4)):
        monkeypatch.setenv('VT_DOT_PART_CAP', str(cap))
        sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
        monkeypatch.delenv('VT_DOT_PART_CAP')
        got = sv.extract_dot_multi(ms, tmpls, mask)
        info = sv.info()
        assert info.last_kernel == 15 and info.last_grid == tiles * last, (cap, info.last_grid, tiles)
        assert np.array_equal(bits(got), bits(want)), (interp, cap)
        sv.close()


# ---- 6. known answer, exact ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_known_answer_one_hot_templates(flags):
    shape, box = (50, 60, 70), (20, 24, 28)
    rs = np.random.RandomState(24)
    vol = rs.randint(0, 16, shape).astype(np.float32)
    hot = np.array([[0, 0, 0], [19, 23, 27], [7, 15, 16], [8, 16, 15], [16, 8, 3], [3, 0, 27], [19, 0, 0], [10, 12, 14], [15, 23, 1]])
    assert len(hot) == K and len({tuple(x) for x in hot}) == K
    tmpls = np.zeros((K,) + box, np.float32)
    for j, (z, y, x) in enumerate(hot):
        tmpls[j, z, y, x] = 1
    starts = np.array([[5, 6, 7], [0, 0, 0], [30, 36, 42], [-8, 30, -10], [40, 50, 60], [45, -20, 66], [-30, -30, -30]])
    c = (np.asarray(box) - 1) / 2
    pad = 32
    padded = np.pad(vol, pad, mode='constant').astype(np.float64)
    want = np.zeros((len(starts), 2 + K))
    for i, st in enumerate(starts):
        z, y, x = st + pad
        b = padded[z:z + box[0], y:y + box[1], x:x + box[2]]
        want[i, 0], want[i, 1] = b.sum(), (b * b).sum()                  # small integers: exact in any order
        want[i, 2:] = [b[tuple(h)] for h in hot]
    assert not want[6].any() and want[:6, 0].all() and want[:3, 2:].any(axis=1).all()
    sv = vt.StaticVolume(vol, interpolation='linear', device='gpu:0')
    got = sv.extract_dot_multi(vt.utils.box_matrices(starts + c, None, box), tmpls, None, _flags=flags)
    assert sv.info().last_kernel == 15
    sv.close()
    assert np.array_equal(got, want), (flags, got, want)


# ---- 7. correlate_templates_at ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_correlate_templates_at_classifies_the_poses(interp):
    from scipy.ndimage import gaussian_filter
    shape, box = (64, 72, 80), (16, 16, 16)
    vol = gaussian_filter(rand_vol(shape, 33).astype(np.float64), 1.0).astype(np.float32)      # a smooth random source
    _, mask = template_and_mask(box)
    rs = np.random.RandomState(35)
    poses = np.array([[40.3, 41.7, 50.2], [20.6, 30.1, 25.4], [45.2, 22.8, 60.5], [25.9, 50.3, 33.3]])
    rots = np.array([[25.0, 40.0, -70.0], [-60.0, 10.0, 130.0], [0.0, 0.0, 0.0], [200.0, 75.0, 15.0]])
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    templates = sv.extract_at(poses, rots, box)
    assert templates.shape == (4,) + box
    pos = np.concatenate([poses, rs.uniform(20, 44, (5, 3))])
    rot = np.concatenate([rots, rs.uniform(0, 360, (5, 3))])
    for m in (mask, None):
        cc = sv.correlate_templates_at(pos, rot, templates, m)
        assert sv.info().last_kernel == 15
        print(interp, m is not None, 'cc diagonal', ' '.join(f'{cc[i, i]:.5f}' for i in range(4)), ' decoys max', f'{cc[4:].max():.4f}')
        assert cc.shape == (9, 4) and cc.dtype == np.float64 and np.isfinite(cc).all()
        assert np.argmax(cc[:4], axis=1).tolist() == [0, 1, 2, 3]
        assert (np.diag(cc[:4]) > 0.99).all(), np.diag(cc[:4])
        assert (cc[4:] < 0.99).all()
        for j in range(4):
            assert np.array_equal(bits(cc[:, j]), bits(sv.correlate_at(pos, rot, templates[j], m))), (interp, j)
    sv.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    rs = np.random.RandomState(30)
    vol = rs.randint(0, 16, (20, 24, 28)).astype(np.float32)
    tmpls = rs.randint(-3, 4, (K, 8, 8, 8)).astype(np.float32)
    ones = np.ones((8, 8, 8), np.float32)
    m = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    out = np.full((1, 2 + K), 7.0)
    b = vol[:8, :8, :8].astype(np.float64)
    want = np.array([[b.sum(), (b * b).sum()] + [(tmpls[j] * b).sum() for j in range(K)]])      # small integers: exact

    def call(h, n=1, mat=m, k=K, t=tmpls, mk=ones, box=(8, 8, 8), o=out):
        return lib.vt_volume_extract_dot_multi(h, n, mat.ctypes.data, k, None if t is None else t.ctypes.data,
                                               None if mk is None else mk.ctypes.data, *box, None if o is None else o.ctypes.data, 0)

    def refused(rc, word=None):
        msg = lib.vt_last_error()
        return rc == VT_EINVAL and msg and (word is None or word in msg)

    def shape_of(h):
        info = _native.VolumeInfo()
        _native.check(lib.vt_volume_info(h, ctypes.byref(info)), 'info')
        return info.out_depth, info.out_height, info.out_width

    def still_usable(h):
        assert np.array_equal(out, np.full((1, 2 + K), 7.0))            # the refusal wrote nothing
        _native.check(call(h), 'extract_dot_multi after a refusal')
        assert np.array_equal(bits(out), bits(want))
        out[...] = 7.0

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert refused(call(h), b'slab')
    assert refused(lib.vt_volume_extract_dot_multi_f64(h, 1, m64.ctypes.data, K, tmpls.ctypes.data, None, 8, 8, 8, out.ctypes.data, 0), b'slab')
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert refused(call(h), b'finalize')
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    dims = shape_of(h)
    still_usable(h)
    nan = tmpls.copy()
    nan[7, 3, 4, 5] = np.nan
    inf = ones.copy()
    inf[7, 7, 7] = np.inf
    bad = m.copy()
    bad[1, 2] = np.nan
    for kwargs, word in ((dict(k=0), b'template count'), (dict(k=-3), b'template count'), (dict(t=None), None), (dict(o=None), None),
                         (dict(n=0), None), (dict(t=nan), b'template 7'), (dict(mk=inf), b'mask'), (dict(mat=bad), b'finite'),
                         (dict(box=(8, 0, 8)), None)):
        assert refused(call(h, **kwargs), word), (kwargs, lib.vt_last_error())
        still_usable(h)
        assert shape_of(h) == dims
    _native.check(call(h, mk=None), 'extract_dot_multi without a mask')
    assert np.array_equal(out, want)
    out[...] = 7.0
    _native.check(lib.vt_volume_extract_dot_multi_f64(h, 1, m64.ctypes.data, K, tmpls.ctypes.data, ones.ctypes.data, 8, 8, 8, out.ctypes.data, 0),
                  'extract_dot_multi_f64')
    assert np.array_equal(out, want) and shape_of(h) == dims
    lib.vt_volume_destroy(h)


def test_refusals_are_followed_by_the_bits_of_the_bit_identity_test():
    """Through the Python class (whose argument checks stand in front of the library's) a refused library call is provoked with
    _native directly on the handle; the next valid call gives the bits extract_dot gives."""
    box = (17, 23, 29)
    ms = bit_case(box)
    tmpls = templates_of(box)
    _, mask = template_and_mask(box)
    sv = vt.StaticVolume(rand_vol(SHAPE, 21), interpolation='filt_bspline', device='gpu:0')
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    want = assert_columns_are_kernel_14s(sv, ms, tmpls, mask, 0, 'before').copy()
    out = np.zeros((len(ms), 2 + K))
    nan = tmpls.copy()
    nan[7, 1, 2, 3] = np.nan
    for k, t in ((0, tmpls), (-1, tmpls), (K, nan)):
        rc = sv._lib.vt_volume_extract_dot_multi(sv._handle, len(ms), ms.ctypes.data, k, t.ctypes.data, mask.ctypes.data, *box, out.ctypes.data, 0)
        assert rc == VT_EINVAL and not out.any()
        assert np.array_equal(bits(sv.extract_dot_multi(ms, tmpls, mask)), bits(want))
        info = sv.info()
        assert (info.out_depth, info.out_height, info.out_width) == dims == SHAPE
    sv.close()


# ---- 9. edge='scipy' -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', list(TOL_EDGE))
def test_edge_scipy_handle(interp):
    shape, box = (70, 66, 72), (24, 40, 32)
    vol = rand_vol(shape, 27)
    ms = batch(shape, box)
    tmpls = templates_of(box, 45, 4)
    _, mask = template_and_mask(box)
    cpu = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    ref_boxes = cpu.extract(ms, box)
    want = cpu.extract_dot_multi(ms, tmpls, mask)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    for flags in FLAGS:
        got = assert_columns_are_kernel_14s(sv, ms, tmpls, mask, flags, (interp, 'edge=scipy', flags))
        for j in range(len(tmpls)):
            _, bound, _ = sums_and_bounds(ref_boxes, tmpls[j], mask, TOL_EDGE[interp])
            check_dot(got[:, [0, 1, 2 + j]], want[:, [0, 1, 2 + j]], bound, (interp, 'edge=scipy', flags, j))
    sv.close()
