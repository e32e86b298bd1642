"""-m gpu: the two-buffer schedule, stage_patch, the staged / gathered switch and the image shapes of StaticVolume.backproject
(kernel 18), against the float64 model of tests/backproject_model.py and against the library's own per-entry results.

tests/test_gpu_backproject.py has one entry order: its untiled entry at position 8, its outside entry at position 7.  Here the batches
are orders of a few building blocks -- staged entries with patches of clearly different sizes, entries untiled by size, one entirely
outside, one that reaches part of the tiles, one that alone reaches a tile row -- so that the prologue's next_staged, the rotation of the
two buffers and the entries that pass the rotation by are met in every position.  Every classification comes from info() and from the
model's masks, never from a re-implementation of the host planner.

  * every order: check_sum against the model; check_own against the float64 sum, in entry order, of the library's own batch-of-one
    results on the same flags (an entry's patch geometry does not depend on its batch, so that bound is one rounding wide and any stale
    or mis-rotated buffer breaks it);
  * the alternating batch and the 61-entry batch again with accumulate=True over a base that holds NaN, Inf and -0 where no entry reaches;
  * stage_patch: patch rows of more than 256 vectors (Lx > 1024, step_y == 0) from an anisotropic entry on a (2, 8, 1200) stack,
    rows of one or two vectors (Lx of 4 or 8);
  * an in-plane scale sweep across 2 * Ly * Lx * 4 <= lds_limit, the switch found from info();
  * image widths 4k + 1, 4k + 2, 4k + 3, images smaller than the cubic stencil, a one-image stack, each on a fresh handle and on one
    whose resident buffer is the recycled allocation of a handle that held values of magnitude 1e3 (stack=True filt_* included), with
    matrices that sample up to and over the right and bottom faces: bit for bit the same.
No output shape selects backproject_entry_point's (16, 16, 16) configuration (tests/test_backproject_cases_host.py), so none is here.
"""
import collections
import functools
import time

import numpy as np
import pytest

import backproject_model as bm
import voltools_amd as vt
from voltools_amd import _native
from handle_sequences import resident_pitch
from test_gpu_backproject import STACK, in_plane, tile_classes
from test_gpu_extract import TOL, ALL_INTERPS, rand_vol
from test_gpu_place import bits, check_sum, check_own

pytestmark = pytest.mark.gpu

INTERPS = ('linear', 'bspline', 'filt_bspline')
FLAGS = (0, _native.FORCE_DIRECT)
OUT = (12, 24, 40)                                  # several tiles in every direction
T = STACK[0]


def make(data, interp):
    return vt.StaticVolume(data, interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))


def rows(r1, r2):
    """4x4 float64 matrix with rows 1 and 2 as given (4 numbers each); row 0 is junk on purpose: it is ignored."""
    m = np.eye(4)
    m[0] = (0.3, -0.7, 0.2, 11.0)
    m[1], m[2] = r1, r2
    return m


def blocks():
    """The building blocks on OUT and a 40 x 52 image.  All but `top` leave the rows h < 8 unreached; `top` reaches h <= 9 alone."""
    b = collections.OrderedDict()
    tilt = vt.utils.backproject_matrices([-30.5], 1, OUT, STACK)[0].astype(np.float64)
    tilt[1] = (0.0, 1.0, 0.0, -8.25)
    b['tilt'] = tilt                                                                        # a plain tilt about axis 1
    b['large'] = rows((0.1, 2.5, 0.0, -20.3), (0.05, 0.3, 1.2, -3.7))                       # a patch of about 21 x 28
    b['small'] = rows((0.005, 0.1, 0.0, -1.35), (0.0, 0.02, 0.1, 20.3))                     # in-plane scale 0.1: a patch row of one or two vectors
    b['huge'] = in_plane([[0.25, 40.0, 0], [0, 0, 40.5]], OUT, (27.5, 17.0))                # bp_batch's scale-40 entry: fits no buffer
    b['huge2'] = in_plane([[0.3, 45.0, 0], [0.1, 0.5, 38.0]], OUT, (25.0, 30.0))
    b['outside'] = in_plane([[0, 1.0, 0], [0, 0, 1.0]], OUT, (1000.0, -700.0))
    b['partial'] = rows((0.0, 1.0, 0.0, -12.0), (0.0, 0.0, 1.0, -19.5))                     # reaches h >= 12, w >= 19 only
    b['top'] = rows((0.0, 1.0, 0.0, 30.25), (0.0, 0.0, 1.0, 5.5))                           # reaches h <= 9 only
    return b


BLOCKS = blocks()
STAGED = ('tilt', 'large', 'small', 'partial', 'top')
UNTILED = ('huge', 'huge2')
CYCLE = ('tilt', 'small', 'huge', 'large', 'outside', 'partial', 'huge2', 'large', 'small')
ORDERS = collections.OrderedDict([
    ('untiled_first', ('huge', 'tilt', 'small', 'large')),
    ('outside_first', ('outside', 'tilt', 'large', 'small')),
    ('untiled_last', ('tilt', 'small', 'huge')),
    ('outside_last', ('large', 'small', 'outside')),
    ('two_untiled_adjacent', ('tilt', 'huge', 'huge2', 'small')),
    ('all_untiled', ('huge', 'huge2', 'huge')),
    ('alternating', ('large', 'small') * 4),
    ('last_only', ('partial', 'tilt', 'outside', 'top')),
    ('n1_staged', ('tilt',)), ('n1_untiled', ('huge',)), ('n1_outside', ('outside',)),
    ('n2_small_large', ('small', 'large')), ('n2_untiled_staged', ('huge2', 'tilt')), ('n2_outside_staged', ('outside', 'small')),
    ('n3', ('partial', 'outside', 'large')), ('n3_untiled_middle', ('small', 'huge', 'large')),
    ('cycle61', tuple(CYCLE[i % len(CYCLE)] for i in range(61))),
])
ACCUMULATED = ('alternating', 'cycle61')


def weights_of(n):
    return ((np.arange(n) * 7) % 11 - 5) * 0.25 + 0.125                                     # mixed signs, no zero


@functools.lru_cache(maxsize=None)
def data(shape=STACK, seed=51):
    s = rand_vol(shape, seed)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def model_entry(interp, name, plane):
    """(B float64, inside mask) of one block on one image: computed once, never modified."""
    vols, masks = bm.per_entry(data(), BLOCKS[name][None], [plane], OUT, interp)
    vols[0].setflags(write=False)
    masks[0].setflags(write=False)
    return vols[0], masks[0]


class Own:
    """The library's own batch-of-one results with weight 1, per (block, image, flags), float64."""
    def __init__(self, sv):
        self.sv, self.cache = sv, {}

    def __call__(self, name, plane, flags):
        key = (name, plane, flags)
        if key not in self.cache:
            got = self.sv.backproject(BLOCKS[name][None], OUT, [1.0], planes=[plane], _flags=flags)
            self.cache[key] = (got.astype(np.float64), tuple(self.sv.info().last_lds_dims), tuple(self.sv.info().last_tile))
        return self.cache[key]


def run_order(sv, own, interp, key, flags, base=None):
    names = ORDERS[key]
    n = len(names)
    planes = np.arange(n) % T
    ms = np.stack([BLOCKS[k] for k in names])
    w = weights_of(n)
    vols = np.stack([model_entry(interp, k, int(p))[0] for k, p in zip(names, planes)])
    reached = np.zeros(OUT, bool)
    for k, p in zip(names, planes):
        reached |= model_entry(interp, k, int(p))[1]
    ref = np.zeros(OUT) if base is None else base.astype(np.float64)
    mag = np.abs(ref)
    for i, (k, p) in enumerate(zip(names, planes)):
        one = own(k, int(p), flags)[0]
        ref = ref + w[i] * one
        mag = mag + abs(w[i]) * np.abs(one)
    what = (interp, key, flags, 'accumulate' if base is not None else '')
    if base is None:
        got = sv.backproject(ms, OUT, w, planes=planes, _flags=flags)
    else:
        got = base.copy()
        assert sv.backproject(ms, OUT, w, output=got, planes=planes, accumulate=True, _flags=flags) is None
    info = sv.info()
    assert info.last_kernel == 18, what
    if base is None:
        check_sum(got, vols, w, TOL[interp], what)
        check_own(got, ref, mag, what)
    else:
        assert np.array_equal(bits(got)[~reached], bits(base)[~reached]), what        # NaN, Inf and -0 included
        finite = reached & np.isfinite(base)
        assert finite.sum() == reached.sum()
        check_own(got[reached], ref[reached], mag[reached], what)
        want = base.astype(np.float64) + np.tensordot(w, vols, axes=1)
        bound = np.abs(w).sum() * TOL[interp] + 2.0 ** -23 * np.abs(want)
        assert (np.abs(got.astype(np.float64)[reached] - want[reached]) <= bound[reached]).all(), what
        assert reached.any() and not np.array_equal(bits(got)[reached], bits(base)[reached]), what
    return info, reached


# ---- 1. the building blocks, each as a batch of one --------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
def test_building_blocks_are_what_their_names_say(interp):
    sv = make(data(), interp)
    own = Own(sv)
    try:
        sizes = {}
        for name in BLOCKS:
            vol, mask = model_entry(interp, name, 1)
            got, dims, tile = own(name, 1, 0)
            check_sum(got.astype(np.float32), vol[None], np.ones(1), TOL[interp], (interp, name))
            direct, ddims, _ = own(name, 1, _native.FORCE_DIRECT)
            check_sum(direct.astype(np.float32), vol[None], np.ones(1), TOL[interp], (interp, name, 'direct'))
            assert ddims == (2, 0, 0)
            classes = tile_classes(mask, tile)
            if name in STAGED:
                assert dims[0] == 2 and dims[1] > 0 and dims[2] % 4 == 0 and mask.any(), (name, dims)
                sizes[name] = dims[1] * dims[2]
            elif name in UNTILED:
                assert dims == (2, 0, 0) and mask.any(), (name, dims)                       # untiled by size, not by flag
            else:
                assert name == 'outside' and not mask.any() and not bits(got.astype(np.float32)).any()
            if name != 'top':
                assert not mask[:, :8, :].any(), name
            if name in ('partial', 'top', 'huge', 'huge2'):
                assert (classes == 0).any() and (classes != 0).any(), name                  # reaches some tiles, misses others
        assert own('small', 1, 0)[1][2] in ((4, 8) if interp == 'linear' else (8, 12))      # (the cubic halo adds two columns)
        assert sizes['large'] >= 4 * sizes['small'] and sizes['large'] >= 2 * sizes['tilt'] >= 4 * sizes['small'], sizes
        # a tile that `top` alone reaches
        others = np.zeros(OUT, bool)
        for name in BLOCKS:
            if name != 'top':
                others |= model_entry(interp, name, 1)[1]
        tile = own('top', 1, 0)[2]
        assert ((tile_classes(model_entry(interp, 'top', 1)[1], tile) != 0) & (tile_classes(others, tile) == 0)).any()
        print(f'patch dims (2, Ly, Lx) {interp}:', {k: own(k, 1, 0)[1] for k in BLOCKS})
    finally:
        sv.close()


# ---- 2. orders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
def test_orders_against_the_model_and_the_librarys_own_entries(interp):
    t0 = time.time()
    sv = make(data(), interp)
    own = Own(sv)
    try:
        for key, names in ORDERS.items():
            for flags in FLAGS:
                info, reached = run_order(sv, own, interp, key, flags)
                dims = tuple(info.last_lds_dims)
                if flags == 0:
                    assert (dims[1] > 0) == any(k not in UNTILED for k in names), (key, dims)       # (`outside` would fit; it stages nothing)
            if key == 'last_only':
                # some tile is reached by the last entry and by no other
                tile = tuple(info.last_tile)
                planes = np.arange(len(names)) % T
                cls = [tile_classes(model_entry(interp, k, int(p))[1], tile) for k, p in zip(names, planes)]
                assert ((cls[-1] != 0) & np.all([c == 0 for c in cls[:-1]], axis=0)).any()
        assert len(ORDERS['cycle61']) == 61 and {len(v) for v in ORDERS.values()} >= {1, 2, 3, 61}
    finally:
        sv.close()
    print(f'orders {interp} wall s:', round(time.time() - t0, 2))


@pytest.mark.parametrize('interp', INTERPS)
def test_accumulate_keeps_unreached_bits_under_alternating_and_long_batches(interp):
    base = np.random.RandomState(19).standard_normal(OUT).astype(np.float32)
    base[3, 2, 5], base[10, 5, 30], base[7, 0, 39], base[0, 7, 17] = np.nan, -0.0, np.inf, -np.inf
    base[5, 20, 30] = -0.0
    sv = make(data(), interp)
    own = Own(sv)
    try:
        for key in ACCUMULATED:
            for flags in FLAGS:
                info, reached = run_order(sv, own, interp, key, flags, base=base)
                tile = tuple(info.last_tile)
                assert (tile_classes(reached, tile) == 0).any()                             # whole tiles stay unreached ...
                assert not reached[3, 2, 5] and not reached[10, 5, 30] and not reached[7, 0, 39] and not reached[0, 7, 17]
                assert reached[5, 20, 30]
    finally:
        sv.close()


# ---- 3. stage_patch: rows of more than 256 vectors ------------------------------------------------------------------------------
WIDE = (2, 8, 1200)
ONE_TILE = (8, 8, 16)


def wide_blocks():
    at = ((WIDE[1] - 1) / 2, (WIDE[2] - 1) / 2)
    c = (np.asarray(ONE_TILE, np.float64) - 1) / 2

    def centred(r):
        m = rows((*r[0], 0.0), (*r[1], 0.0))
        m[1:3, 3] = np.asarray(at) - np.asarray(r, np.float64) @ c
        return m
    b = collections.OrderedDict()
    b['aniso'] = centred([[0.02, 0.05, 0.0], [0.3, 0.0, 70.25]])                            # row 2 scaled by about 70, row 1 by 0.05
    b['aniso_neg'] = centred([[0.0, -0.05, 0.0], [0.0, 0.1, -69.5]])
    b['narrow'] = centred([[0.0, 0.1, 0.0], [0.0, 0.0, 0.1]])
    b['plain'] = centred([[0.05, 0.9, 0.1], [0.0, -0.1, 1.1]])
    return b


WIDE_ORDERS = (('aniso',), ('aniso', 'narrow'), ('narrow', 'aniso', 'plain'), ('aniso', 'narrow', 'aniso_neg', 'plain', 'aniso', 'narrow', 'aniso'))


@pytest.mark.parametrize('interp', INTERPS)
def test_patch_rows_longer_than_256_vectors(interp):
    stack = data(WIDE, 53)
    wb = wide_blocks()
    sv = make(stack, interp)
    try:
        alone = {}
        for name, m in wb.items():
            got = sv.backproject(m[None], ONE_TILE, [1.0], planes=[1])
            dims = tuple(sv.info().last_lds_dims)
            assert sv.info().last_kernel == 18 and sv.info().last_grid == 1 and dims[1] > 0, (name, dims)       # one tile, staged
            if name.startswith('aniso'):
                assert dims[2] > 1024 and 2 * dims[1] * dims[2] * 4 <= sv.info().last_lds_bytes <= 160 * 1024, (name, dims)
            if name == 'narrow':
                assert dims[2] in ((4, 8) if interp == 'linear' else (8, 12)), dims
            vol, mask = bm.per_entry(stack, m[None], [1], ONE_TILE, interp)
            assert mask.all() or name != 'aniso'
            check_sum(got, vol, np.ones(1), TOL[interp], (interp, 'wide', name))
            alone[name] = (got.astype(np.float64), vol[0])
            print(f'wide {interp} {name} dims:', dims)
        for names in WIDE_ORDERS:
            ms = np.stack([wb[k] for k in names])
            w = weights_of(len(names))
            got = sv.backproject(ms, ONE_TILE, w, planes=np.ones(len(names), int))
            check_sum(got, np.stack([alone[k][1] for k in names]), w, TOL[interp], (interp, 'wide', names))
            ref, mag = np.zeros(ONE_TILE), np.zeros(ONE_TILE)
            for i, k in enumerate(names):
                ref = ref + w[i] * alone[k][0]
                mag = mag + abs(w[i]) * np.abs(alone[k][0])
            check_own(got, ref, mag, (interp, 'wide', names))
    finally:
        sv.close()


# ---- 4. the switch between staged and gathered -------------------------------------------------------------------------------------
SWEEP_STACK = (2, 150, 260)
SWEEP_OUT = (8, 12, 20)
SCALES = np.round(np.arange(6.0, 15.0001, 0.05), 2)            # wide enough for every tile the planner may give SWEEP_OUT


@pytest.mark.parametrize('interp', INTERPS)
def test_scale_sweep_across_the_staged_gathered_switch(interp):
    stack = data(SWEEP_STACK, 57)
    at = ((SWEEP_STACK[1] - 1) / 2, (SWEEP_STACK[2] - 1) / 2)
    sv = make(stack, interp)
    staged = []
    try:
        ms = np.stack([in_plane([[0.01, s, 0.0], [0.0, 0.02, s]], SWEEP_OUT, at) for s in SCALES])
        vols, masks = bm.per_entry(stack, ms, np.arange(len(ms)) % 2, SWEEP_OUT, interp)
        worst = 0.0
        for i, s in enumerate(SCALES):
            got = sv.backproject(ms[i:i + 1], SWEEP_OUT, [1.0], planes=[i % 2])
            info = sv.info()
            dims = tuple(info.last_lds_dims)
            assert info.last_kernel == 18 and masks[i].any()
            staged.append(dims[1] > 0)
            if staged[-1]:
                assert 2 * dims[1] * dims[2] * 4 <= info.last_lds_bytes <= 160 * 1024, (s, dims)
            else:
                assert dims == (2, 0, 0), (s, dims)
            err = float(np.abs(got.astype(np.float64) - vols[i]).max())
            worst = max(worst, err)
            assert err <= TOL[interp], (interp, s, dims, err)
        # the whole sweep as one batch: staged and gathered entries side by side
        w = weights_of(len(ms))
        got = sv.backproject(ms, SWEEP_OUT, w, planes=np.arange(len(ms)) % 2)
        check_sum(got, vols, w, TOL[interp], (interp, 'sweep batch'))
    finally:
        sv.close()
    staged = np.array(staged)
    flips = np.nonzero(staged[:-1] != staged[1:])[0]
    print(f'{interp}: staged at scales {SCALES[staged]}, gathered at {SCALES[~staged]}; worst err {worst:.3e}'.replace('\n', ' '))
    assert staged.any() and (~staged).any(), staged                          # both sides occur ...
    assert len(flips) == 1 and staged[flips[0]] and not staged[flips[0] + 1]        # ... and two adjacent points straddle the one switch
    print(f'switch {interp}: staged up to {SCALES[flips[0]]}, gathered from {SCALES[flips[0] + 1]}')
    print(f'sweep worst err / TOL {interp}: {worst / TOL[interp]:.3f}')


# ---- 5. image shapes, fresh and recycled handles ---------------------------------------------------------------------------------
SHAPES = ((2, 3, 49), (2, 5, 50), (2, 5, 51), (3, 3, 51), (1, 1, 1), (1, 2, 3), (4, 40, 52))


def edge_matrices(shape):
    """Entries that sample up to and over the right and bottom faces (and the left and top ones): the taps of the last inside voxels read
    the pad columns and the row past the last."""
    _, H, W = shape
    oh, ow = min(H, 40) + 8, min(W, 52) + 10                                                # the output of the test
    return np.stack([rows((0.0, 1.0, 0.0, -2.0), (0.0, 0.0, 1.0, -3.0)),                    # integer lattice
                     rows((0.01, 1.0, 0.0, -2.75), (0.02, 0.0, 1.0, -3.75)),                # y up to H - 0.68, x up to W - 0.61: taps in the row
                                                                                            # past the last and in the first pad column
                     rows((0.0, 0.5, 0.0, H - 0.3 - 0.5 * (oh - 1)), (0.0, 0.0, 0.5, W - 0.3 - 0.5 * (ow - 1))),    # scale 0.5 into the far corner
                     rows((0.0, 1.0, 0.0, -2.5), (0.0, 0.0, 1.0, -3.5)),                    # lines exactly on all four faces
                     rows((0.0, 0.9, 0.3, -4.0), (0.0, -0.3, 0.9, 0.5))])                   # rotated: the corners


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_image_shapes_on_fresh_and_recycled_handles(shape, interp):
    lib = _native.load()
    out = (8, min(shape[1], 40) + 8, min(shape[2], 52) + 10)
    stack = data(shape, 61)
    ms = edge_matrices(shape)
    planes = np.arange(len(ms)) % shape[0]
    w = weights_of(len(ms))
    vols, masks = bm.per_entry(stack, ms, planes, out, interp)
    assert all(mk.any() and not mk.all() for mk in masks)
    beyond = [False, False]                                                                 # taps beyond the last row / the last column
    for m, mk in zip(ms, masks):
        y, x = bm.coords(m, out)
        beyond = [beyond[0] or bool((y[mk] > shape[1] - 1).any()), beyond[1] or bool((x[mk] > shape[2] - 1).any())]
    assert all(beyond)
    wide = (shape[0], shape[1], resident_pitch(shape[2]) - 4)
    assert resident_pitch(wide[2]) == resident_pitch(shape[2]) and wide[2] > shape[2]
    dirty_data = (1.0e3 * (1.0 + rand_vol(wide, 63))).astype(np.float32)

    def run(sv):
        res = []
        for flags in FLAGS:
            got = sv.backproject(ms, out, w, planes=planes, _flags=flags)
            assert sv.info().last_kernel == 18
            check_sum(got, vols, w, TOL[interp], (interp, shape, flags))
            res.append(got)
            for i in range(len(ms)):
                one = sv.backproject(ms[i:i + 1], out, [1.0], planes=planes[i:i + 1], _flags=flags)
                check_sum(one, vols[i:i + 1], np.ones(1), TOL[interp], (interp, shape, flags, i))
                res.append(one)
        return res

    _native.check(lib.vt_device_trim(0), 'vt_device_trim')
    sv = make(stack, interp)
    try:
        fresh = run(sv)
    finally:
        sv.close()
    _native.check(lib.vt_device_trim(0), 'vt_device_trim')        # the recycler holds nothing else: the next handle's buffers are the dirty one's
    dirty = make(dirty_data, interp)
    try:
        dirty_bytes = int(dirty.info().resident_bytes)
        junk = dirty.backproject(ms, out, planes=planes)           # ... and so is the staging of the host output
        assert np.abs(junk).max() > 100.0
    finally:
        dirty.close()
    sv = make(stack, interp)
    try:
        assert int(sv.info().resident_bytes) == dirty_bytes > 0     # the same resident size: the recycler's first match
        recycled = run(sv)
    finally:
        sv.close()
    for a, b in zip(fresh, recycled):
        assert np.array_equal(bits(a), bits(b)), (interp, shape)
