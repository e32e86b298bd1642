"""-m gpu: StaticVolume.backproject_boxes (vt_volume_backproject_boxes, kernel 19): nb boxes of one shape from one resident stack in one
launch.  The contract is bit identity: box b holds what the library's own backproject (kernel 18) writes for that box's matrices, weights
and planes -- compared under np.array_equal AND as uint32, so the sign of a zero counts.  Besides: every box against the float64 model of
tests/backproject_model.py at test_gpu_backproject.py's TOL, a mixed batch (an all-outside box, entries untiled by size first / last /
twice in a row, a box partly over the images, tiles reached by one entry only, staged patches of different sizes), independence of a box
from its neighbours, accumulate over NaN / Inf / -0, the lattice, face and tile-margin entries of tests/backproject_cases.py, the Python
cut along the box axis, determinism and output kinds, handle state and the refusals.

Box shapes (10, 18, 18) and (10, 26, 18): linear tiles (8, 8, 16) and (8, 16, 16), cubic (8, 8, 16) both; cut tiles in every dimension.
No output shape selects the (16, 16, 16) configuration (tests/test_backproject_cases_host.py), so none is here."""
import ctypes
import functools

import numpy as np
import pytest

import backproject_cases as bc
import backproject_model as bm
import voltools_amd as vt
from voltools_amd import _native
from test_gpu_backproject import STACK, in_plane, tile_classes
from test_gpu_box_lattice import positive
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, rand_vol
from test_gpu_place import bits, check_sum

pytestmark = pytest.mark.gpu

VT_EUNSUPPORTED = 10004
BOXES = ((10, 18, 18), (10, 26, 18))
FLAGS = (0, _native.FORCE_DIRECT)
N = 6                                               # entries per box = images in STACK
PLANES = np.array([3, 0, 5, 2, 2, 1])
T = STACK[0]


def rows(r1, r2):
    """4x4 float64 matrix with rows 1 and 2 as given; row 0 is junk on purpose: it is ignored."""
    m = np.eye(4)
    m[0] = (0.3, -0.7, 0.2, 11.0)
    m[1], m[2] = r1, r2
    return m


def tilts(box, angles, axis=1, at=None):
    ms = vt.utils.backproject_matrices(angles, axis, box, STACK)
    if at is not None:                                                 # move the centre of the box to image point `at`
        ms[:, 1, 3] += at[0] - (STACK[1] - 1) / 2
        ms[:, 2, 3] += at[1] - (STACK[2] - 1) / 2
    return list(ms)


@functools.lru_cache(maxsize=None)
def mixed_batch(box):
    """(names, (7, N, 4, 4) float64 matrices): one box per situation the kernel's walk can meet, all in one call."""
    huge = in_plane([[0.25, 40.0, 0], [0, 0, 40.5]], box, (27.5, 17.0))           # in-plane scale 40: its patch fits no LDS buffer
    huge2 = in_plane([[0.3, 45.0, 0], [0.1, 0.5, 38.0]], box, (25.0, 30.0))
    large = rows((0.1, 2.5, 0.0, -20.3), (0.05, 0.3, 1.2, -3.7))                   # a patch of about 21 x 28 floats
    small = rows((0.005, 0.1, 0.0, -1.35), (0.0, 0.02, 0.1, 20.3))                 # in-plane scale 0.1: a patch row of one or two vectors
    outside = in_plane([[0, 1.0, 0], [0, 0, 1.0]], box, (1000.0, -700.0))
    t = tilts(box, [-60.0, -30.5, 0.0, 20.0, 45.0, 58.0])
    boxes = [
        ('tilts', t),
        ('outside', [outside] * N),
        ('untiled_first_and_twice', [huge, t[0], t[4], huge, huge2, t[2]]),
        ('untiled_last', [t[1], small, large, t[3], t[5], huge2]),
        # the box hangs over the image corner: only h >= 7 and w >= 16 or 17 are over the images, so the tiles of w < 16 are reached by
        # no entry under every tiling, and the others are cut
        ('partial', tilts(box, [-10.0, -5.0, 0.0, 4.0, 7.5, 10.0], 1, (1.25, -8.4))),
        # five entries reach h >= 16 only, one reaches h <= 9 only: the first tile row is that entry's alone
        ('single_reach', [rows((0.0, 1.0, 0.0, -16.0), (0.02 * k, 0.0, 1.0, 10.5 + k)) for k in range(3)] +
                         [rows((0.0, 1.0, 0.0, 30.25), (0.0, 0.0, 1.0, 5.5))] +
                         [rows((0.01, 1.0, 0.0, -16.0), (0.0, 0.05 * k, 1.0, 20.25)) for k in range(2)]),
        ('patch_sizes', [large, small, large, small, t[2], small]),
    ]
    names = tuple(k for k, _ in boxes)
    ms = np.ascontiguousarray(np.stack([np.stack(v) for _, v in boxes]), dtype=np.float64)
    assert ms.shape == (7, N, 4, 4)
    ms.setflags(write=False)
    return names, ms


def mixed_weights(nb):
    w = ((np.arange(nb * N) * 7) % 11 - 5) * 0.25 + 0.125              # mixed signs, no zero
    return w.reshape(nb, N)


@functools.lru_cache(maxsize=None)
def data(seed=41):
    s = rand_vol(STACK, seed)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def model_case(interp, box, f32):
    """(per-entry float64 model volumes (nb, N) + box, inside masks) of mixed_batch: computed once, never modified."""
    _, ms = mixed_batch(box)
    ms = ms.astype(np.float32).astype(np.float64) if f32 else ms
    out = [bm.per_entry(data(), ms[b], PLANES, box, interp) for b in range(len(ms))]
    vols, masks = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    vols.setflags(write=False)
    masks.setflags(write=False)
    return vols, masks


def handle(interp, stack=None):
    return vt.StaticVolume(data() if stack is None else stack, interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))


def same_bits(a, b):
    """np.array_equal on the values and on the uint32 views: a sign-of-zero difference fails."""
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True) and np.array_equal(bits(a), bits(b))


def own(sv, ms, w, box, flags=0, planes=PLANES):
    """The library's own backproject of every box's matrices, weights and planes (kernel 18)."""
    res = np.stack([sv.backproject(ms[b], box, w[b], planes=planes, _flags=flags) for b in range(len(ms))])
    assert sv.info().last_kernel == 18
    return res


def tiles_in(box, tile):
    return int(np.prod([-(-s // t) for s, t in zip(box, tile)]))


# ---- 1. identity with backproject, the model, the mixed batch -----------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('box', BOXES, ids=['x'.join(map(str, b)) for b in BOXES])
def test_identity_with_backproject_and_the_model(box, interp):
    names, ms64 = mixed_batch(box)
    nb = len(ms64)
    w = mixed_weights(nb)
    tile = bc.tile_of(bc.icls(interp), box)
    sv = handle(interp)
    try:
        for f32 in (False, True):
            ms = ms64.astype(np.float32) if f32 else ms64
            vols, masks = model_case(interp, box, f32)
            for flags in FLAGS:
                got = sv.backproject_boxes(ms, box, w, planes=PLANES, _flags=flags)
                info = sv.info()
                assert got.shape == (nb,) + box and got.dtype == np.float32
                assert info.last_kernel == 19 and tuple(info.last_tile) == tile and info.last_grid == nb * tiles_in(box, tile)
                dims = tuple(info.last_lds_dims)
                if flags == 0:
                    assert dims[0] == 2 and dims[1] > 0 and dims[2] % 4 == 0 and info.last_lds_bytes == 2 * 4 * dims[1] * dims[2], dims
                else:
                    assert dims == (2, 0, 0)
                ref = own(sv, ms, w, box, flags)
                for b in range(nb):
                    assert same_bits(got[b], ref[b]), (interp, box, f32, flags, names[b], int((bits(got[b]) != bits(ref[b])).sum()))
                    check_sum(got[b], vols[b], w[b], TOL[interp], (interp, box, f32, flags, names[b]))
        # ---- what the mixed batch holds, from the model's masks and from info() of the single-box calls ----
        vols, masks = model_case(interp, box, False)
        b_out = names.index('outside')
        assert not masks[b_out].any() and same_bits(got[b_out], np.zeros(box, np.float32))                  # exact +0
        part = masks[names.index('partial')]
        assert all(0 < m.sum() < m.size for m in part)
        cls = np.stack([tile_classes(m, tile) for m in masks[names.index('single_reach')]])
        assert ((cls != 0).sum(axis=0) == 1).any()                                                          # a tile one entry alone reaches
        assert (cls == 1).any()
        staged = {}
        for b, name in enumerate(names):
            for i in range(N):
                sv.backproject(ms64[b, i:i + 1], box, planes=PLANES[i:i + 1])
                staged[(name, i)] = tuple(sv.info().last_lds_dims)[1:]
        first = [staged[('untiled_first_and_twice', i)] == (0, 0) for i in range(N)]
        assert first == [True, False, False, True, True, False]                                             # first, and twice in a row
        assert [staged[('untiled_last', i)] == (0, 0) for i in range(N)] == [False] * 5 + [True]
        sizes = [staged[('patch_sizes', i)][0] * staged[('patch_sizes', i)][1] for i in range(N)]
        assert min(sizes) > 0 and sizes[0] > 4 * sizes[1] and sizes[2] > 4 * sizes[3]                        # the buffers alternate sizes
        assert len({v for v in staged.values() if v != (0, 0)}) >= 3                                        # ... and across boxes
    finally:
        sv.close()


# ---- 2. independence ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_a_box_does_not_depend_on_its_neighbours(interp):
    box = BOXES[1]
    names, ms = mixed_batch(box)
    nb = len(ms)
    w = mixed_weights(nb)
    sv = handle(interp)
    try:
        for flags in FLAGS:
            full = sv.backproject_boxes(ms, box, w, planes=PLANES, _flags=flags).copy()
            assert full.any()
            perm = np.array([4, 0, 6, 2, 5, 1, 3])
            got = sv.backproject_boxes(ms[perm], box, w[perm], planes=PLANES, _flags=flags)
            assert same_bits(got, full[perm])
            for sub in ([2], [0, 3], [6, 5, 1], [1, 2, 3, 4, 5]):
                got = sv.backproject_boxes(ms[sub], box, w[sub], planes=PLANES, _flags=flags)
                assert same_bits(got, full[sub]), (interp, flags, sub)
            for b in range(nb):                                                                             # nb = 1
                got = sv.backproject_boxes(ms[b:b + 1], box, w[b:b + 1], planes=PLANES, _flags=flags)
                assert sv.info().last_grid == tiles_in(box, tuple(sv.info().last_tile))
                assert same_bits(got[0], full[b]), (interp, flags, names[b])
            # another box's matrices replaced: by a strongly minified entry (fits no buffer), by large patches, by an outside one
            for victim, repl in ((0, ms[2, 0]), (3, ms[6, 0]), (6, ms[1, 0]), (1, ms[0, 0])):
                other = np.array(ms)
                other[victim, :] = repl
                got = sv.backproject_boxes(other, box, w, planes=PLANES, _flags=flags)
                keep = [b for b in range(nb) if b != victim]
                assert same_bits(got[keep], full[keep]), (interp, flags, victim)
                assert not np.array_equal(got[victim], full[victim])
    finally:
        sv.close()


# ---- 3. accumulate ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
@pytest.mark.parametrize('box', BOXES, ids=['x'.join(map(str, b)) for b in BOXES])
def test_accumulate(box, interp):
    names, ms = mixed_batch(box)
    nb = len(ms)
    w = mixed_weights(nb)
    tile = bc.tile_of(bc.icls(interp), box)
    _, masks = model_case(interp, box, False)
    rs = np.random.RandomState(8)
    base = rs.standard_normal((nb,) + box).astype(np.float32)
    kind = rs.randint(0, 12, base.shape)
    base[kind == 0] = np.nan
    base[kind == 1] = np.inf
    base[kind == 2] = -0.0
    base[kind == 3] = -np.inf
    sv = handle(interp)
    try:
        for flags in FLAGS:
            for device_out in (False, True):
                if device_out:
                    out = vt.empty((nb,) + box, device='gpu:0')
                    out.set(base)
                    assert sv.backproject_boxes(ms, box, w, output=out, planes=PLANES, accumulate=True, _flags=flags) is None
                    sv.synchronize()
                    got = out.get()
                else:
                    got = base.copy()
                    assert sv.backproject_boxes(ms, box, w, output=got, planes=PLANES, accumulate=True, _flags=flags) is None
                assert sv.info().last_kernel == 19
                untouched = 0
                for b in range(nb):
                    ref = base[b].copy()
                    sv.backproject(ms[b], box, w[b], output=ref, planes=PLANES, accumulate=True, _flags=flags)
                    assert same_bits(got[b], ref), (interp, box, flags, device_out, names[b])
                    # tiles no entry of this box reaches keep their bits
                    reached = np.stack([tile_classes(m, tile) for m in masks[b]]).any(axis=0)
                    for a, c, e in zip(*np.nonzero(~reached)):
                        sl = (b, slice(a * tile[0], (a + 1) * tile[0]), slice(c * tile[1], (c + 1) * tile[1]),
                              slice(e * tile[2], (e + 1) * tile[2]))
                        assert np.array_equal(bits(got[sl]), bits(base[sl])), (names[b], a, c, e)
                        untouched += 1
                    if reached.any():
                        assert not np.array_equal(bits(got[b]), bits(base[b]))
                assert untouched > tiles_in(box, tile)                      # the outside box, and tiles of others
                assert np.array_equal(bits(got[names.index('outside')]), bits(base[names.index('outside')]))
    finally:
        sv.close()


# ---- 4. lattice, face and tile-margin entries ---------------------------------------------------------------------------------------
POSITIVE = ('linear', 'bspline', 'bspline_simple')  # non-negative weights on the data itself: zeros are the outside
EDGE_N = 6
EDGE_NB = 7


@functools.lru_cache(maxsize=None)
def edge_stack():
    s = positive(rand_vol(bc.STACK, 401))           # values in [1, 2)
    s.setflags(write=False)
    return s


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('oi', range(len(bc.OUTS)), ids=['x'.join(map(str, o)) for o in bc.OUTS])
def test_lattice_face_and_margin_entries_in_boxes(oi, interp):
    """The cases of tests/backproject_cases.py, every second one of each group plus all tile-margin cases, as the entries of boxes:
    EDGE_N consecutive cases per box, EDGE_NB boxes per call (the last box is filled up from the start of the list).  The float64
    cases go through the float64 entry point, the float32 twins through the float32 one.  Weights all 1 and data in [1, 2): under the
    non-negative interpolations `got != 0` is the union of the entries' inside masks, voxel for voxel."""
    out = bc.OUTS[oi]
    assert out == BOXES[oi]
    ii = ALL_INTERPS.index(interp)
    tile = bc.tile_of(bc.icls(interp), out)
    cases = bc.selected(out, oi, ii, 2) + bc.whole_margin_cases(out, tile)
    planes = bc.planes_of(EDGE_N).astype(np.int32)
    sv = handle(interp, edge_stack())
    groups = set()
    try:
        for f32 in (False, True):
            mine = [c for c in cases if c[2]['f32'] == f32]
            if not mine:
                continue
            groups |= {'margin' if c[2].get('margin') else c[2]['group'] for c in mine}
            mats = [m for _, m, _ in mine]
            mats += mats[:(-len(mats)) % EDGE_N]
            ms = np.ascontiguousarray(np.stack(mats).reshape(-1, EDGE_N, 4, 4), dtype=np.float32 if f32 else np.float64)
            for b0 in range(0, len(ms), EDGE_NB):
                part = ms[b0:b0 + EDGE_NB]
                nb = len(part)
                for flags in FLAGS:
                    got = sv.backproject_boxes(part, out, planes=planes, _flags=flags)
                    info = sv.info()
                    assert info.last_kernel == 19 and tuple(info.last_tile) == tile and info.last_grid == nb * tiles_in(out, tile)
                    assert (info.last_lds_dims[1] > 0) == (flags == 0)
                    ref = own(sv, part, np.ones((nb, EDGE_N)), out, flags, planes)
                    for b in range(nb):
                        assert same_bits(got[b], ref[b]), (interp, out, f32, flags, b0 + b)
                    if interp in POSITIVE and flags == 0:
                        for b in range(nb):
                            union = np.zeros(out, bool)
                            for m in part[b].astype(np.float64):
                                union |= bc.mask_of(m, out)[0]
                            differs = int(((got[b] != 0) != union).sum())
                            assert differs == 0, (interp, out, f32, b0 + b, differs)
    finally:
        sv.close()
    assert groups >= {'lattice', 'f32twin', 'face_exact', 'face_chain', 'margin'}, groups


# ---- 5. the Python cut, determinism, output kinds, handle state -----------------------------------------------------------------------
def test_python_cut_determinism_and_output_kinds():
    box = BOXES[0]
    names, ms = mixed_batch(box)
    nb = len(ms)
    w = mixed_weights(nb)
    sv = handle('filt_bspline')
    tile = bc.tile_of('cubic', box)
    tiles = tiles_in(box, tile)
    fresh = sv.backproject_boxes(ms, box, w, planes=PLANES).copy()
    assert fresh.any() and sv.info().last_grid == nb * tiles
    # the cut: 200 bytes of tables per (box, entry)
    got = sv.backproject_boxes(ms, box, w, planes=PLANES, _max_table_bytes=200 * N * 4)       # 4 + 3 boxes: two library calls
    assert sv.info().last_grid == 3 * tiles and same_bits(got, fresh)
    got = sv.backproject_boxes(ms, box, w, planes=PLANES, _max_table_bytes=200 * N * 4 + 199)
    assert sv.info().last_grid == 3 * tiles and same_bits(got, fresh)
    for small in (200 * N, 1):                                                                 # one box per call: nb library calls
        got = sv.backproject_boxes(ms, box, w, planes=PLANES, _max_table_bytes=small)
        assert sv.info().last_grid == tiles and same_bits(got, fresh)
    dev = vt.empty((nb,) + box, device='gpu:0')
    dev.set(np.full((nb,) + box, 5, np.float32))
    assert sv.backproject_boxes(ms, box, w, output=dev, planes=PLANES, _max_table_bytes=200 * N * 2) is None
    sv.synchronize()
    assert sv.info().last_grid == tiles and same_bits(dev.get(), fresh)
    # repeated calls, another call in between, a fresh handle
    assert same_bits(sv.backproject_boxes(ms, box, w, planes=PLANES), fresh)
    sv.backproject_boxes(ms[:2, :3], (9, 10, 11), planes=PLANES[:3])
    sv.backproject(ms[0], BOXES[1])
    assert same_bits(sv.backproject_boxes(ms, box, w, planes=PLANES), fresh)
    assert (sv.info().out_depth, sv.info().out_height, sv.info().out_width) == STACK              # the handle's own output shape is untouched
    other = handle('filt_bspline')
    assert same_bits(other.backproject_boxes(ms, box, w, planes=PLANES), fresh)
    other.close()
    # output kinds
    host = np.full((nb,) + box, 5, np.float32)
    assert sv.backproject_boxes(ms, box, w, output=host, planes=PLANES) is None
    dev.set(np.full((nb,) + box, 5, np.float32))
    assert sv.backproject_boxes(ms, box, w, output=dev, planes=PLANES) is None
    sv.synchronize()
    assert same_bits(host, fresh) and same_bits(dev.get(), fresh)
    # weights (n,) serve every box; None = ones; planes=None: image i belongs to entry i
    got = sv.backproject_boxes(ms, box, w[0], planes=PLANES)
    assert same_bits(got, sv.backproject_boxes(ms, box, np.tile(w[0], (nb, 1)), planes=PLANES))
    assert same_bits(sv.backproject_boxes(ms, box), sv.backproject_boxes(ms, box, np.ones((nb, N)), planes=np.arange(N)))
    torch = pytest.importorskip('torch')
    tens = torch.full((nb,) + box, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.backproject_boxes(ms, box, w, output=tens, planes=PLANES) is None
    sv.synchronize()
    assert same_bits(tens.cpu().numpy(), fresh)
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_handle_state(interp):
    for box in BOXES:
        names, ms = mixed_batch(box)
        nb = len(ms)
        w = mixed_weights(nb)
        sv = handle(interp)
        fresh = handle(interp)
        want = fresh.backproject(ms[3], box, w[3], planes=PLANES)
        want_info = fresh.info()
        sv.backproject_boxes(ms, box, w, planes=PLANES)
        info = sv.info()
        tile = tuple(info.last_tile)
        assert info.last_kernel == 19 and tile == tuple(want_info.last_tile) == bc.tile_of(bc.icls(interp), box)
        assert info.last_grid == nb * tiles_in(box, tile) == nb * want_info.last_grid
        assert tuple(info.last_lds_dims)[0] == 2 and info.last_lds_bytes == 8 * info.last_lds_dims[1] * info.last_lds_dims[2]
        # the batch-wide largest patch sizes the allocation: at least any single box's
        assert info.last_lds_bytes >= want_info.last_lds_bytes
        got = sv.backproject(ms[3], box, w[3], planes=PLANES)
        after = sv.info()
        assert same_bits(got, want) and after.last_kernel == 18 and after.last_grid == want_info.last_grid
        assert after.last_lds_bytes == want_info.last_lds_bytes and tuple(after.last_lds_dims) == tuple(want_info.last_lds_dims)
        sv.close()
        fresh.close()


def test_boxes_at_are_crops_of_backproject_tilts():
    """backproject_boxes_at against crops of backproject_tilts at integer offsets, at TOL (the two coordinate chains differ by ulps)."""
    angles = np.linspace(-50.0, 50.0, T)
    volume, box = (16, 44, 60), BOXES[0]
    offs = np.array([[0, 0, 0], [3, 12, 21], [6, 26, 42], [2, 20, 5]])
    c = (np.asarray(box, np.float64) - 1.0) / 2.0
    w = np.array([1.0, -0.5, 0.75, 2.0, 1.25, 0.5])
    for interp in ('linear', 'filt_bspline'):
        sv = handle(interp)
        full = sv.backproject_tilts(angles, output_shape=volume, weights=w)
        got = sv.backproject_boxes_at(offs + c, angles, 1, volume, box, weights=w)
        assert sv.info().last_kernel == 19 and got.shape == (4,) + box
        ms = vt.utils.backproject_box_matrices(offs + c, angles, 1, volume, box, STACK[1:])
        assert same_bits(got, sv.backproject_boxes(ms, box, w))
        for b, o in enumerate(offs):
            crop = full[o[0]:o[0] + box[0], o[1]:o[1] + box[1], o[2]:o[2] + box[2]]
            err = float(np.abs(got[b].astype(np.float64) - crop).max())
            print(f'{interp} box {b}: max|box - crop| {err:.3e}')
            assert err <= 2 * np.abs(w).sum() * TOL[interp], (interp, b, err)
        sv.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _native.load()
    box = BOXES[0]
    _, ms64 = mixed_batch(box)
    m2 = np.ascontiguousarray(ms64[:2, :1], dtype=np.float32)                 # two boxes, one entry each
    ones = np.ones(2)
    p0 = np.zeros(1, np.int32)
    out = np.zeros((2,) + box, np.float32)

    def call(h, nb=2, n=1, mat=m2, planes=p0, w=ones, shape=box, flags=0, f64=False):
        fn = lib.vt_volume_backproject_boxes_f64 if f64 else lib.vt_volume_backproject_boxes
        mat = np.ascontiguousarray(mat, dtype=np.float64 if f64 else np.float32)
        return fn(h, nb, n, mat.ctypes.data, None if planes is None else planes.ctypes.data, None if w is None else w.ctypes.data,
                  *shape, out.ctypes.data, flags)

    vol = data()
    # a slab window, an unfinalised handle
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, *STACK, 0, vol.ctypes.data, 0, 2, 12, 2, 6, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    assert call(h, f64=True) == VT_EINVAL
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, *STACK, 0, None, _native.SRC_DEFERRED, 0, T, 0, T, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, T, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    _native.check(call(h), 'backproject_boxes after finalize')
    lib.vt_volume_destroy(h)
    # filt_* without VT_STACK, in Python and by the library; VT_EDGE_SCIPY
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    with pytest.raises(ValueError):
        sv.backproject_boxes(ms64, box, planes=PLANES)
    assert call(sv._handle) == VT_EUNSUPPORTED and b'VT_STACK' in lib.vt_last_error()
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK              # ... and the handle does everything else
    sv.close()
    sv = vt.StaticVolume(vol, device='gpu:0', edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    with pytest.raises(RuntimeError, match=f'code {VT_EUNSUPPORTED}'):
        sv.backproject_boxes(ms64, box, planes=PLANES)
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()

    sv = handle('bspline')
    hd = sv._handle
    want = sv.backproject_boxes(m2, box, planes=[0]).copy()
    assert want.any()
    # non-finite matrices or weights
    for where in ((0, 0, 1, 2), (1, 0, 2, 3)):
        bad = m2.copy()
        bad[where] = np.nan
        assert call(hd, mat=bad) == VT_EINVAL and b'finite' in lib.vt_last_error()
        assert call(hd, mat=bad, f64=True) == VT_EINVAL
        with pytest.raises(RuntimeError, match='finite'):
            sv.backproject_boxes(bad, box, planes=[0])
    assert call(hd, w=np.array([1.0, np.inf])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    with pytest.raises(ValueError):
        sv.backproject_boxes(m2, box, [[1.0], [np.inf]], planes=[0])
    # planes
    for bad in ([T], [-1]):
        assert call(hd, planes=np.array(bad, np.int32)) == VT_EINVAL and b'plane' in lib.vt_last_error()
        with pytest.raises(ValueError):
            sv.backproject_boxes(m2, box, planes=bad)
    assert call(hd, planes=None) == VT_EINVAL and b'plane' in lib.vt_last_error()           # n = 1 != T
    with pytest.raises(ValueError):
        sv.backproject_boxes(m2, box)
    # dims, n, nb
    for shape in ((0,) + box[1:], (box[0], -1, box[2]), box[:2] + (0,)):
        assert call(hd, shape=shape) == VT_EINVAL
    assert call(hd, n=0) == VT_EINVAL and call(hd, n=-2) == VT_EINVAL
    assert call(hd, nb=0) == VT_EINVAL and call(hd, nb=-1) == VT_EINVAL and b'boxes' in lib.vt_last_error()
    assert call(hd, nb=0, f64=True) == VT_EINVAL
    # bounds: nb x n and nb x tiles below 2^31 (refused before anything is read)
    assert call(hd, nb=1 << 16, n=1 << 15) == VT_EUNSUPPORTED and call(hd, nb=1 << 16, n=1 << 15, f64=True) == VT_EUNSUPPORTED
    assert b'pairs' in lib.vt_last_error()
    assert call(hd, nb=1 << 30) == VT_EUNSUPPORTED and b'grid' in lib.vt_last_error()       # 2^30 boxes x 12 tiles
    assert call(hd, nb=(1 << 31) // 12 + 1, f64=True) == VT_EUNSUPPORTED and b'grid' in lib.vt_last_error()
    with pytest.raises(ValueError):
        sv.backproject_boxes(m2, box, planes=[0], accumulate=True)            # accumulate without output
    # the handle is still usable; NULL weights are ones; flags other than the four are ignored
    _native.check(call(hd, w=None, flags=_native.KEEP_OUTSIDE | _native.PLACE_DENSE), 'backproject_boxes')
    assert same_bits(out, want)
    _native.check(call(hd, w=None, f64=True), 'backproject_boxes_f64')
    assert same_bits(out, want)
    sv.close()
