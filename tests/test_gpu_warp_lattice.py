"""-m gpu: warp (kernel 20) and place (kernel 17) on integer-lattice, skirt-face and margin coordinates.

Kernel 20 against the float64 model of tests/warp_model.py on the cases of tests/warp_lattice_cases.py.  Both summands of s = a + u are
exact there, so NO voxel is left out of any comparison (tests/test_gpu_warp.py leaves out what comes within 1e-9 of a face).  Per case,
for flags 0 and FORCE_DIRECT: last_kernel 20 and the launch record equal to the model's plan; |got - model| <= TOL[interp] of
tests/test_gpu_extract.py on every voxel; outside voxels +0 by bits; for the non-negative interpolations (the source lies in [1, 2))
`got != 0` equal to the model's inside mask voxel for voxel; for linear the two routes bit for bit; with the zero grid and the constant
field also the oracle of `extract` on the combined matrix.  Every node appends the cases aimed at kTileMargin (the mask equality is
their point), the cases beyond the hull grant, the one with a single huge node (both routes in one launch) and the one whose tile
extent is 4096 or more.  Outputs with axes of length 1 and 2 and the faces of edge='scipy' have tests of their own.

Kernel 17 on lattice_cases.box_cases with the output as "the box", only by what vt_kernels_place.hip documents: one copy with weight 1
holds the bits `extract` writes for that matrix (kernel 11; under FORCE_DIRECT the direct kernel's), the weighted batch is held against
the oracle's boxes by check_sum, sparse lists give the dense lists' bits (batch and every entry alone), the zeros of a single
non-negative copy are the oracle's, and an accumulating pass leaves NaN, Inf and -0 in a tile no listed copy reaches as they were.

Which check would catch which wrong kernel is argued on the CPU in tests/test_warp_lattice_host.py.  The ledger at the end counts
(kernel, class, tile, group, sign of eps, field kind, route) and asserts the coverage; it skips itself on a partial run."""
import collections
import functools
import time

import numpy as np
import pytest

import box_index_model as bm
import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle

import warp_cases as wc
import warp_lattice_cases as wl
import warp_model as wm
from test_gpu_extract import TOL
from test_gpu_edge_scipy import TOL as TOL_EDGE
from test_gpu_extract_sum import check_sum, weights
from test_gpu_warp import bits, same_bits_up_to_zero_sign
from test_gpu_box_lattice import BOXES, POSITIVE, SHAPE, TEXTURE_GROUPS, TILE_OF, Failures, batches, selected
from test_gpu_box_lattice import source as box_source

pytestmark = pytest.mark.gpu

N = _native
SRC = wl.SRC
LEDGER = collections.Counter()      # (kernel, class, tile, group, sign of eps, field kind | None, route | 'whole' | 'cut') -> cases
CASES = collections.Counter()       # (class, tile, group, sign of eps) -> kernel-20 cases (a case has one ledger row per route)
WORST = {}                          # (kernel, interp) -> largest |got - model| (17: of the weighted sum against the oracle's)
WALL = {}
COUNTS = {}                         # node -> (exact, margin zero-grid, margin constant-field, hull) cases run
VOXELS = collections.Counter()      # 'compared', 'left out'
NODES_RUN, NODES_ALL = set(), set()


def _icls(interp):
    return 'linear' if interp == 'linear' else 'cubic'


@functools.lru_cache(maxsize=None)
def oracle_source(filtered):
    vol = wl.source_volume()
    return oracle.prefilter(vol) if filtered else vol


@functools.lru_cache(maxsize=None)
def _oracle_result(key, sampling):
    c = wl.BY_KEY[key]
    kind = 'linear' if sampling == 'linear' else 'bspline'
    return oracle.affine_ex(oracle_source(sampling == 'filt'), c.affine, kind, c.out_shape).astype(np.float64)


def oracle_result(case, interp):
    return _oracle_result(wl.key_of(case), wl.SAMPLING[interp])


def run(sv, case, flags=0):
    got = sv.warp(case.grid, wl.matrix_of(case), case.out_shape, _flags=flags)
    return got, sv.info()


def hold_to_model(fails, got, case, interp, what):
    """Every voxel: the value, the bits of the outside, the mask."""
    vals = wl.values(case, interp)
    ins = wl.geometry(case)[1]
    fails.check(got.shape == case.out_shape and got.dtype == np.float32 and bool(np.isfinite(got).all()), case.name, what, 'shape / dtype / finite')
    err = float(np.abs(got.astype(np.float64) - vals).max())
    VOXELS['compared'] += got.size
    WORST[(20, interp)] = max(WORST.get((20, interp), 0.0), err)
    fails.check(err <= TOL[interp], case.name, what, 'max|got - model|', err)
    fails.check(not bits(got)[~ins].any(), case.name, what, 'outside voxels are not all +0')
    if interp in POSITIVE:
        differs = int(((got != 0) != ins).sum())
        fails.check(differs == 0, case.name, what, 'inside mask differs on', differs, 'voxels')
    if case.affine is not None:
        err = float(np.abs(got.astype(np.float64) - oracle_result(case, interp)).max())
        fails.check(err <= TOL[interp], case.name, what, 'max|got - oracle(combined matrix)|', err)


def hold_record(fails, info, case, interp, direct):
    p, what = wl.plan_of(case, interp)
    fails.check(info.last_kernel == 20 and info.last_grid == int(np.prod(p.nT)) and tuple(info.last_tile) == tuple(p.tile), case.name,
                'kernel / grid / tile', info.last_kernel, info.last_grid, tuple(info.last_tile))
    dims, nbytes = ((0, 0, 0), (wm.SCRATCH_FLOATS + p.node_floats) * 4) if direct else (tuple(p.lds_dims), p.lds_bytes)
    fails.check(tuple(info.last_lds_dims) == dims and info.last_lds_bytes == nbytes <= 160 * 1024, case.name, 'direct' if direct else 'default',
                'lds dims / bytes', tuple(info.last_lds_dims), info.last_lds_bytes, 'model', dims, nbytes)
    return p, what


def both_routes(fails, sv, case, interp, ledger=True):
    got, info = run(sv, case)
    p, what = hold_record(fails, info, case, interp, False)
    hold_to_model(fails, got, case, interp, 'default')
    direct, info = run(sv, case, N.FORCE_DIRECT)
    hold_record(fails, info, case, interp, True)
    if interp == 'linear':
        fails.check(same_bits_up_to_zero_sign(got, direct), case.name, 'the two routes differ')
    hold_to_model(fails, direct, case, interp, 'direct')
    if ledger:
        t = case.traits
        CASES[(_icls(interp), tuple(p.tile), t['group'], t['eps_sign'])] += 1
        for route in set(what.ravel()):
            LEDGER[(20, _icls(interp), tuple(p.tile), t['group'], t['eps_sign'], case.kind, route)] += 1
    return what


def default_route(fails, sv, case, interp):
    """Cases that leave the staged route on their own: default flags, the model on every voxel, FORCE_DIRECT's bits for linear."""
    got, info = run(sv, case)
    p, what = hold_record(fails, info, case, interp, False)
    hold_to_model(fails, got, case, interp, 'default')
    if interp == 'linear':
        fails.check(np.array_equal(bits(got), bits(run(sv, case, N.FORCE_DIRECT)[0])), case.name, 'default != FORCE_DIRECT')
    return what


def every_second(cases, shift):
    out = []
    for group in sorted({c.traits['group'] for c in cases}):
        out += [c for j, c in enumerate(c for c in cases if c.traits['group'] == group) if (j + shift) % 2 == 0]
    return out


for _oi in range(len(wl.OUTS)):
    for _interp in wc.INTERPS:
        NODES_ALL.add(f'warp-{_oi}-{_interp}')


@pytest.mark.parametrize('interp', wc.INTERPS)
@pytest.mark.parametrize('oi', range(len(wl.OUTS)), ids=['x'.join(map(str, o)) for o in wl.OUTS])
def test_warp_on_lattice_face_margin_and_hull_cases(oi, interp):
    t_start = time.time()
    out = wl.OUTS[oi]
    shift = wc.INTERPS.index(interp) + oi
    sv = vt.StaticVolume(wl.source_volume(), interpolation=interp, device='gpu:0')
    fails = Failures()
    try:
        exact = every_second(wl.exact_cases(out), shift)
        for case in exact:
            both_routes(fails, sv, case, interp)
        zero, const = wl.margin_cases(out, interp in wm.CUBIC)
        fails.check(len(zero) >= 8, 'margin cases', len(zero))
        for case in zero + const:
            both_routes(fails, sv, case, interp, ledger=False)
        hull = every_second(wl.hull_cases(out), shift)
        for case in hull:
            what = default_route(fails, sv, case, interp)
            fails.check(bool((what == 'direct').all()), case.name, 'a tile beyond the hull grant does not gather')
        single = wl.single_node_case(out)
        what = wl.plan_of(single, interp)[1]
        assert (what == 'direct').any() and (what == 'stage').any()
        default_route(fails, sv, single, interp)
        LEDGER[(20, _icls(interp), tuple(wl.plan_of(single, interp)[0].tile), 'single', 0, 'single', 'both')] += 1
        what = default_route(fails, sv, wl.extent_case(out), interp)
        fails.check(not (what == 'stage').any(), 'extent case stages')
        COUNTS[f'warp-{oi}-{interp}'] = (len(exact), len(zero), len(const), len(hull))
    finally:
        sv.close()
    NODES_RUN.add(f'warp-{oi}-{interp}')
    WALL[f'warp-{oi}-{interp}'] = time.time() - t_start
    fails.done()


NODES_ALL.add('degenerate')


def test_outputs_with_axes_of_length_one_and_two():
    t_start = time.time()
    fails = Failures()
    for interp in wc.INTERPS:
        sv = vt.StaticVolume(wl.source_volume(), interpolation=interp, device='gpu:0')
        try:
            for case in wl.degenerate_cases():
                both_routes(fails, sv, case, interp, ledger=False)
        finally:
            sv.close()
    NODES_RUN.add('degenerate')
    WALL['degenerate'] = time.time() - t_start
    fails.done()


SCIPY_INTERPS = ('linear', 'bspline', 'filt_bspline')
for _interp in SCIPY_INTERPS:
    NODES_ALL.add(f'scipy-{_interp}')


@pytest.mark.parametrize('interp', SCIPY_INTERPS)
def test_edge_scipy_on_chain_exact_faces(interp):
    """edge='scipy': the cut moves to s = 0 and s = dim - 1 (both inside).  scipy forms its coordinates in its own order, hence the zero
    grid and the constant field only; against device='cpu' at TOL_EDGE of tests/test_gpu_edge_scipy.py."""
    t_start = time.time()
    out = wl.OUTS[0]
    vol = wl.source_volume()
    cpu = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    fails = Failures()
    cases = every_second(wl.scipy_cases(out), SCIPY_INTERPS.index(interp))
    try:
        for case in cases:
            want = np.asarray(cpu.warp(case.grid, case.m, out), np.float64)
            for flags in (0, N.FORCE_DIRECT):
                got, info = run(sv, case, flags)
                err = float(np.abs(got.astype(np.float64) - want).max())
                VOXELS['compared'] += got.size
                fails.check(info.last_kernel == 20 and err <= TOL_EDGE[interp], case.name, flags, 'max|got - cpu|', err)
    finally:
        sv.close()
    assert len(cases) >= 30
    NODES_RUN.add(f'scipy-{interp}')
    WALL[f'scipy-{interp}'] = time.time() - t_start
    fails.done()


# ---- place (kernel 17) ----------------------------------------------------------------------------------------------------------
PLACE_FLAGS = (0, N.FORCE_DIRECT, N.PLACE_DENSE)
for _bi in range(len(BOXES)):
    for _interp in wc.INTERPS:
        NODES_ALL.add(f'place-{_bi}-{_interp}')


def tile_regions(box, tile):
    for d0 in range(0, box[0], tile[0]):
        for h0 in range(0, box[1], tile[1]):
            for w0 in range(0, box[2], tile[2]):
                yield (slice(d0, d0 + tile[0]), slice(h0, h0 + tile[1]), slice(w0, w0 + tile[2]))


@pytest.mark.parametrize('interp', wc.INTERPS)
@pytest.mark.parametrize('bi', range(len(BOXES)), ids=['x'.join(map(str, b)) for b in BOXES])
def test_place_on_lattice_and_face_cases(bi, interp):
    t_start = time.time()
    box = BOXES[bi]
    ii = wc.INTERPS.index(interp)
    vol, src, kind = box_source(interp, 341 + bi)
    tol = TOL[interp]
    tile = TILE_OF[(_icls(interp), box)]
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    fails = Failures()
    try:
        margin = bm.whole_margin_cases(SHAPE, box, bm.TILES.index(tile))
        fails.check(len(margin) >= 8, 'margin cases', len(margin))
        for cases, ms in batches(selected(box, bi, ii) + margin):
            n = len(cases)
            names = [c[0] for c in cases]
            dt = str(ms.dtype)
            want = np.stack([oracle.affine_ex(src, m64, kind, box) for _, m64, _ in cases]).astype(np.float64)
            w = weights(n)
            ones = [np.ones(1)] * n
            results = {}
            for flags in PLACE_FLAGS:
                ref = sv.extract(ms, box, _flags=N.FORCE_DIRECT if flags == N.FORCE_DIRECT else 0)
                fails.check(sv.info().last_kernel == (1 if flags == N.FORCE_DIRECT else 11), dt, flags, 'extract ran kernel', sv.info().last_kernel)
                alone = []
                for i in range(n):
                    one = sv.place(ms[i:i + 1], box, ones[i], _flags=flags)
                    info = sv.info()
                    alone.append(one)
                    fails.check(info.last_kernel == 17, names[i], dt, flags, 'place ran kernel', info.last_kernel)
                    if flags == 0:
                        fails.check(tuple(info.last_tile) == tile, names[i], 'tile', tuple(info.last_tile))
                        if min(info.last_lds_dims) > 0:
                            t = cases[i][2]
                            LEDGER[(17, _icls(interp), tile, t['group'], t['eps_sign'], None, 'whole' if t['whole'] else 'cut')] += 1
                    fails.check(np.array_equal(bits(one + 0.0), bits(ref[i] + 0.0)), names[i], dt, flags, 'place(n = 1, w = 1) != extract')
                    if interp in POSITIVE:
                        differs = int(((one == 0) != (want[i] == 0)).sum())
                        fails.check(differs == 0, names[i], dt, flags, 'inside mask differs on', differs, 'voxels')
                    if flags != N.PLACE_DENSE:
                        dense = sv.place(ms[i:i + 1], box, ones[i], _flags=flags | N.PLACE_DENSE)
                        fails.check(np.array_equal(bits(one), bits(dense)), names[i], dt, flags, 'sparse != dense, entry alone')
                total = results[flags] = sv.place(ms, box, w, _flags=flags)
                fails.check(sv.info().last_kernel == 17, dt, flags, 'place ran kernel', sv.info().last_kernel)
                WORST[(17, interp)] = max(WORST.get((17, interp), 0.0), float(np.abs(total - np.tensordot(w, want, axes=1)).max()))
                try:
                    check_sum(total, want, w, tol, (interp, box, dt, flags))
                except AssertionError as e:
                    fails.check(False, dt, flags, 'place', str(e)[:200])
                if flags == N.FORCE_DIRECT:
                    fails.check(np.array_equal(bits(total), bits(sv.place(ms, box, w, _flags=flags | N.PLACE_DENSE))), dt, flags, 'sparse != dense, batch')
            fails.check(np.array_equal(bits(results[0]), bits(results[N.PLACE_DENSE])), dt, 'sparse != dense, batch')
            fails.check(np.array_equal(bits(results[0]), bits(sv.place(ms, box, w, _flags=N.PLACE_DENSE))), dt, 'dense lists are not deterministic')
            if ms.dtype != np.float64:
                continue
            # ---- accumulate: the tile that most copies leave alone holds NaN, Inf, -Inf and -0; those copies are added in one pass ----
            reached = want != 0
            region, members = max(((r, [i for i in range(n) if not reached[i][r].any()]) for r in tile_regions(box, tile)), key=lambda x: len(x[1]))
            fails.check(len(members) >= 2, 'accumulate: no tile that two copies leave alone')
            if len(members) >= 2:
                base = np.random.RandomState(9).standard_normal(box).astype(np.float32)
                special = np.zeros(box, bool)
                special[region] = True
                spots = np.argwhere(special)
                for k, v in enumerate((np.nan, np.inf, -0.0, -np.inf)):
                    base[tuple(spots[(k * (len(spots) - 1)) // 3])] = v
                untouched = ~reached[members].any(axis=0)
                host = base.copy()
                sv.place(ms[members], box, w[members], output=host, accumulate=True)
                fails.check(sv.info().last_kernel == 17, 'accumulate ran kernel', sv.info().last_kernel)
                fails.check(np.array_equal(bits(host)[region], bits(base)[region]), 'accumulate changed the tile no copy reaches')
                fails.check(np.array_equal(bits(host)[untouched], bits(base)[untouched]), 'accumulate changed voxels no copy reaches')
                fails.check(not np.array_equal(bits(host)[~untouched], bits(base)[~untouched]), 'accumulate added nothing')
    finally:
        sv.close()
    NODES_RUN.add(f'place-{bi}-{interp}')
    WALL[f'place-{bi}-{interp}'] = time.time() - t_start
    fails.done()


# ---- the ledger -------------------------------------------------------------------------------------------------------------------
WARP_TILES = (('linear', ((8, 16, 16), (8, 8, 16))), ('cubic', ((8, 8, 16),)))


def ledger_report():
    lines = ['coverage ledger, kernel 20: cases per (class, tile) x (group and sign of eps), x field kind, x route seen in the plan']
    cols = [(g, s) for g in wl.GROUPS for s in (1, -1, 0)]
    lines.append('%-22s' % 'class tile' + ''.join('%13s' % (g + '0+-'[s]) for g, s in cols))
    for c, tile in sorted({(k[1], k[2]) for k in LEDGER if k[0] == 20}):
        def count(**kw):
            return sum(v for k, v in LEDGER.items() if k[:3] == (20, c, tile) and all(k[dict(group=3, sign=4, kind=5, route=6)[a]] == b for a, b in kw.items()))
        name = f'{c} {"x".join(map(str, tile))}'
        lines.append('%-22s' % name + ''.join('%13d' % CASES[(c, tile, g, s)] for g, s in cols))
        lines.append('%-22s' % '' + ' '.join(f'{kind}: {count(kind=kind, route="stage")}/{count(kind=kind, route="direct")}/{count(kind=kind, route="zero")}'
                                             for kind in wl.FIELD_KINDS) + '   (cases with staged / gathering / empty tiles)')
    lines.append('coverage ledger, kernel 17: single copies in staged launches per (class, tile) x group, whole / cut')
    for c, tile in sorted({(k[1], k[2]) for k in LEDGER if k[0] == 17}):
        row = {g: sum(v for k, v in LEDGER.items() if k[:4] == (17, c, tile, g)) for g in TEXTURE_GROUPS}
        wc_ = {x: sum(v for k, v in LEDGER.items() if k[:3] == (17, c, tile) and k[6] == x) for x in ('whole', 'cut')}
        lines.append('%-22s' % f'{c} {"x".join(map(str, tile))}' + ' '.join(f'{g}: {v}' for g, v in row.items()) + f'   whole: {wc_["whole"]} cut: {wc_["cut"]}')
    lines.append('largest |got - model| per (kernel, interpolation) [17: of the weighted sum against the oracle\'s]: ' +
                 ', '.join(f'{k}: {v:.3e}' for k, v in sorted(WORST.items())))
    lines.append('cases per warp node (exact, margin with the zero grid, margin with the constant field, hull): ' +
                 ', '.join(f'{k}: {v}' for k, v in sorted(COUNTS.items())))
    lines.append('wall time per node (s): ' + ', '.join(f'{k}: {v:.2f}' for k, v in sorted(WALL.items())))
    lines.append(f'voxels compared: {VOXELS["compared"]}, left out: {VOXELS["left out"]}')
    return '\n'.join(lines)


def test_zz_coverage_ledger():
    """Kernel 20: each class met each group on each of its tiles with eps of either sign, and staged, gathering and empty tiles on each;
    kernel 17: each group on each tile of each class, whole and cut copies both.  No voxel was left out.  Last in the file; skips itself
    when only a selection of the file ran."""
    print('\n' + ledger_report())
    assert VOXELS['left out'] == 0
    if NODES_RUN != NODES_ALL:
        pytest.skip(f'only {len(NODES_RUN)} of {len(NODES_ALL)} nodes ran: the ledger describes a selection')
    missing = []
    for c, tiles in WARP_TILES:
        for tile in tiles:
            for g in wl.GROUPS:
                for s in (1, -1):
                    if not any(v for k, v in LEDGER.items() if k[:5] == (20, c, tile, g, s)):
                        missing.append((20, c, tile, g, s))
            for route in ('stage', 'direct', 'zero'):
                if not any(v for k, v in LEDGER.items() if k[:3] == (20, c, tile) and k[6] == route):
                    missing.append((20, c, tile, route))
            for kind in wl.FIELD_KINDS:
                if not any(v for k, v in LEDGER.items() if k[:3] == (20, c, tile) and k[5] == kind):
                    missing.append((20, c, tile, kind))
            for g in TEXTURE_GROUPS:
                if not any(v for k, v in LEDGER.items() if k[:4] == (17, c, tile, g)):
                    missing.append((17, c, tile, g))
            for x in ('whole', 'cut'):
                if not any(v for k, v in LEDGER.items() if k[:3] == (17, c, tile) and k[6] == x):
                    missing.append((17, c, tile, x))
    assert not missing, missing
