"""-m gpu: the box kernels (kinds 11-16) on integer-lattice and skirt-face coordinates (lattice_cases.box_cases), against the CPU oracle.

The suites of these kernels draw random rotations at fractional positions; here a known share of every box's voxels sits within
2^-50 .. 2^-20 of an integer source coordinate and whole planes, rows and columns sit exactly on the hard cut of the inside test.  What
that attacks is the geometry the six kernels repeat: the float64 tile bounding box, the origin of the staged box, the Q32.32 coordinates
restarted per tile column and stepped with a rounded increment, and the "whole" tiles that skip the per-voxel inside test
(tests/box_index_model.py models the tap indices on the host; tests/test_box_index_model.py asserts them without a GPU).

All selected cases of a node travel as ONE batch per launch (float64 matrices through the _f64 entry points, the float32 twins as a
float32 batch).  The source data lie in [1, 2): under non-negative weights an inside voxel is strictly positive, so `got == 0` must
equal `want == 0` voxel for voxel -- the inside mask, which a box result otherwise hides (tests/test_lattice_cases.py asserts that the
oracle alone has this property).  Checked per node, flags 0 / FORCE_TILED / FORCE_DIRECT, every voxel or pixel, no new tolerance:
  11  |got - oracle| <= TOL[interp]; the mask equality; each box alone holds its bits of the batch
  12  against the float64 depth sum of the oracle's boxes, TOL * depth (tests/test_gpu_project_batch.py)
  13  n = 1, w = 1 holds kernel 11's bits; the weighted sum of the batch by check_sum (tests/test_gpu_extract_sum.py)
  14  sums over the oracle's boxes by sums_and_bounds / check_dot, sums over the library's own kind-11 boxes at ACC
  15  columns hold kernel 14's bits (K = 9);  16  columns hold kernel 13's bits (G = 9)
The coverage ledger at the end counts (kernel, interpolation class, group, sign of eps, tile, whole / cut) per staged launch and
asserts that each kernel met each group on every tile the planner gives its class.

Which check would catch a wrong kernel (argued on the CPU in tests/test_box_index_model.py, never by running one): an origin one too high
-- the value test, on every whole box (the model with that origin reports a lowest tap of -1 everywhere); `whole` without kTileMargin --
the mask equality on `box_index_model.whole_margin_cases`, which every node appends to its batch (tiles whose float64 bounding box is
inside by a bare comparison while the canonical chain puts one of their voxels outside); an inside test taken from the fixed-point
coordinate -- the mask equality on the face-chain cases (hundreds of voxels change sides).
"""
import collections
import time

import numpy as np
import pytest

import box_index_model as bm
import lattice_cases as lc
import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle
from test_gpu_extract import TOL, TOL_EDGE, ALL_INTERPS, rand_vol
from test_gpu_extract_sum import check_sum, weights
from test_gpu_extract_dot import ACC, check_dot, sums_and_bounds, template_and_mask
from test_gpu_extract_dot_multi import K, templates_of
from test_gpu_extract_sum_multi import G, weight_matrix
from test_gpu_project_batch import segments_of

pytestmark = pytest.mark.gpu

N = _native
SHAPE = (96, 100, 104)                              # the box suites' source
BOXES = ((10, 18, 18), (10, 26, 18))                # trilinear: tiles (8, 8, 16) and (8, 16, 16); cubic: (8, 8, 16) both (the planner gives it no other)
TILE_OF = {('linear', BOXES[0]): (8, 8, 16), ('linear', BOXES[1]): (8, 16, 16), ('cubic', BOXES[0]): (8, 8, 16), ('cubic', BOXES[1]): (8, 8, 16)}
PROJ_ONLY = ((6, 18, 18), (40, 18, 18))             # kernel 12 besides: one depth segment, five
FLAGS = (0, N.FORCE_TILED, N.FORCE_DIRECT)
TEXTURE_GROUPS = ('lattice', 'f32twin', 'face_exact', 'face_chain')
STRIDE = 2                                          # a node takes every second case of each group, shifted from node to node
POSITIVE = ('linear', 'bspline', 'bspline_simple')  # non-negative weights on the data itself: zeros are the inside mask

LEDGER = collections.Counter()                      # (kernel, 'linear' | 'cubic', group, sign of eps, tile, 'whole' | 'cut') -> cases in staged launches
WORST = {}                                          # (kernel, interp) -> largest |got - oracle| (12: per plane of depth)
WALL = {}                                           # node -> seconds
NODES_RUN = set()
NODES_ALL = set()


class Failures(list):
    def check(self, ok, *what):
        if not ok:
            self.append(what)

    def done(self):
        assert not self, f'{len(self)} failed checks, first: ' + '; '.join(repr(w) for w in self[:8])


def _icls(interp):
    return 'linear' if interp == 'linear' else 'cubic'


def positive(unit):
    """Unit-range data moved into [1, 2) (a float32 sample that rounded up to 1.0 is clipped to the float32 below 2)."""
    vol = np.minimum(unit + np.float32(1.0), np.nextafter(np.float32(2.0), np.float32(0.0))).astype(np.float32)
    assert vol.min() >= 1.0 and vol.max() < 2.0
    return vol


def source(interp, seed):
    """(volume in [1, 2), what the oracle samples: the volume, or its B-spline coefficients)"""
    vol = positive(rand_vol(SHAPE, seed))
    return vol, (oracle.prefilter(vol) if interp.startswith('filt') else vol), (interp[5:] if interp.startswith('filt') else interp)


def selected(box, bi, ii, groups=TEXTURE_GROUPS, stride=STRIDE, exact_only=False):
    out = []
    for g in groups:
        cases = [c for c in lc.box_cases(SHAPE, box, (g,)) if c[2]['exact'] or not exact_only]
        out += [c for j, c in enumerate(cases) if (j + ii + 2 * bi) % stride == 0]
    return out


def batches(cases):
    """[(dtype, cases, matrices)]: the float64 cases as a float64 batch, the float32 twins as a float32 batch."""
    out = []
    for f32 in (False, True):
        mine = [c for c in cases if c[2]['f32'] == f32]
        if mine:
            out.append((mine, np.ascontiguousarray(np.stack([m for _, m, _ in mine]), dtype=np.float32 if f32 else np.float64)))
    return out


def note(info, kernel, interp, cases, err=None):
    """One launch into the ledger -- when it ran the kernel it was meant for AND staged boxes (FORCE_DIRECT entries gather from global
    memory inside the same kernel; a declined flag set falls back silently)."""
    if info.last_kernel != kernel:
        return False
    if err is not None:
        WORST[(kernel, interp)] = max(WORST.get((kernel, interp), 0.0), float(err))
    if min(info.last_lds_dims) <= 0:
        return False
    for _, _, t in cases:
        LEDGER[(kernel, _icls(interp), t['group'], t['eps_sign'], tuple(info.last_tile), 'whole' if t['whole'] else 'cut')] += 1
    return True


def bits32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def tol_failures(fails, got, want, tol, names, *what):
    err = np.abs(got.astype(np.float64) - want).reshape(len(names), -1).max(axis=1)
    for i in np.nonzero(~(err <= tol))[0]:
        fails.check(False, names[i], *what, 'err', float(err[i]), 'tol', tol)
    return float(err.max())


for _bi in range(len(BOXES)):
    for _interp in ALL_INTERPS:
        NODES_ALL.add(f'box-{_bi}-{_interp}')


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('bi', range(len(BOXES)), ids=['x'.join(map(str, b)) for b in BOXES])
def test_box_kernels_on_lattice_and_face_cases(bi, interp):
    t_start = time.time()
    box = BOXES[bi]
    ii = ALL_INTERPS.index(interp)
    vol, src, kind = source(interp, 301 + bi)
    tol = TOL[interp]
    tmpl, mask = template_and_mask(box)
    tmpls = templates_of(box)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    fails = Failures()
    try:
        # ... and the cases aimed at kTileMargin on this node's tile (a tile "inside" by a bare comparison that holds an outside voxel)
        margin = bm.whole_margin_cases(SHAPE, box, bm.TILES.index(TILE_OF[(_icls(interp), box)]))
        fails.check(len(margin) >= 8, 'margin cases', len(margin))
        for cases, ms in batches(selected(box, bi, ii) + margin):
            n = len(cases)
            names = [c[0] for c in cases]
            dt = str(ms.dtype)
            want = np.stack([oracle.affine_ex(src, m64, kind, box) for _, m64, _ in cases])
            want_img = want.astype(np.float64).sum(axis=1)
            w = weights(n)
            wm = weight_matrix(n)
            want_dot, bound_dot, _ = sums_and_bounds(want, tmpl, mask, tol)
            for flags in FLAGS:
                # ---- 11 ----
                got = sv.extract(ms, box, _flags=flags)
                info = sv.info()
                staged = info.last_kernel == 11
                fails.check(info.last_kernel == (1 if flags == N.FORCE_DIRECT else 11), dt, flags, 'extract ran kernel', info.last_kernel)
                if staged:
                    fails.check(tuple(info.last_tile) == TILE_OF[(_icls(interp), box)], dt, flags, 'tile', tuple(info.last_tile))
                err = tol_failures(fails, got, want, tol, names, dt, flags, 'kernel', info.last_kernel)
                note(info, 11, interp, cases, err)
                if interp in POSITIVE:
                    differs = ((got == 0) != (want == 0)).reshape(n, -1).sum(axis=1)
                    for i in np.nonzero(differs)[0]:
                        fails.check(False, names[i], dt, flags, 'kernel', info.last_kernel, 'inside mask differs on', int(differs[i]), 'voxels')
                for i in range(n):
                    alone = sv.extract(ms[i:i + 1], box, _flags=flags)
                    fails.check(np.array_equal(bits32(alone[0]), bits32(got[i])), names[i], dt, flags, 'box alone != its bits in the batch')
                    if flags == N.FORCE_DIRECT:          # (kernel 11 is not in this launch: the batched direct kernel served it)
                        continue
                    # ---- 13: n = 1, w = 1 ----
                    one = sv.extract_sum(ms[i:i + 1], box, _flags=flags)
                    k13 = note(sv.info(), 13, interp, cases[i:i + 1]) or sv.info().last_kernel == 13
                    fails.check(k13 and np.array_equal(bits32(one), bits32(got[i])), names[i], dt, flags, 'extract_sum(n = 1) != extract')
                # ---- 13: the batch ----
                total = sv.extract_sum(ms, box, w, _flags=flags)
                note(sv.info(), 13, interp, cases, float(np.abs(total - np.tensordot(w, want.astype(np.float64), axes=1)).max()))
                try:
                    check_sum(total, want.astype(np.float64), w, tol, (interp, box, dt, flags))
                except AssertionError as e:
                    fails.check(False, dt, flags, 'extract_sum', str(e)[:200])
                # ---- 16: columns are kernel 13's ----
                multi = sv.extract_sum_multi(ms, box, wm, _flags=flags)
                k16 = note(sv.info(), 16, interp, cases) or sv.info().last_kernel == 16
                fails.check(k16 and multi.shape == (G,) + box, dt, flags, 'extract_sum_multi ran kernel', sv.info().last_kernel)
                for j in range(G):
                    col = sv.extract_sum(ms, box, np.ascontiguousarray(wm[:, j]), _flags=flags)
                    fails.check(np.array_equal(bits32(multi[j]), bits32(col)), dt, flags, 'extract_sum_multi column', j, '!= extract_sum')
                # ---- 14 ----
                dots = sv.extract_dot(ms, tmpl, mask, _flags=flags)
                info = sv.info()
                note(info, 14, interp, cases, float((np.abs(dots - want_dot) / np.maximum(bound_dot, 1e-300)).max()) * tol)
                fails.check(info.last_kernel == 14, dt, flags, 'extract_dot ran kernel', info.last_kernel)
                try:
                    check_dot(dots, want_dot, bound_dot, (interp, box, dt, flags))
                    if flags != N.FORCE_DIRECT:          # the samples are kernel 11's: accumulation error only
                        own, _, mag = sums_and_bounds(got, tmpl, mask, 0.0)
                        check_dot(dots, own, ACC * mag, (interp, box, dt, flags, 'own boxes'))
                except AssertionError as e:
                    fails.check(False, dt, flags, 'extract_dot', str(e)[:200])
                # ---- 15: columns are kernel 14's ----
                dm = sv.extract_dot_multi(ms, tmpls, mask, _flags=flags)
                k15 = note(sv.info(), 15, interp, cases) or sv.info().last_kernel == 15
                fails.check(k15 and dm.shape == (n, 2 + K), dt, flags, 'extract_dot_multi ran kernel', sv.info().last_kernel)
                fails.check(np.array_equal(bits64(dm[:, :2]), bits64(dots[:, :2])), dt, flags, 'extract_dot_multi mask sums != extract_dot')
                for j in range(K):
                    single = sv.extract_dot(ms, tmpls[j], mask, _flags=flags)
                    fails.check(np.array_equal(bits64(dm[:, 2 + j]), bits64(single[:, 2])), dt, flags, 'extract_dot_multi column', j, '!= extract_dot')
                # ---- 12 ----
                img = sv.projection_batch(ms, box, _flags=flags)
                info = sv.info()
                err = tol_failures(fails, img, want_img, tol * box[0], names, dt, flags, 'projection_batch, kernel', info.last_kernel)
                note(info, 12, interp, cases, err / box[0])
                fails.check((info.last_kernel == 12) == (flags == N.FORCE_TILED) or flags == 0, dt, flags, 'projection_batch ran kernel', info.last_kernel)
    finally:
        sv.close()
    NODES_RUN.add(f'box-{bi}-{interp}')
    WALL[f'box-{bi}-{interp}'] = time.time() - t_start
    fails.done()


for _pi in range(len(PROJ_ONLY)):
    for _interp in ALL_INTERPS:
        NODES_ALL.add(f'proj-{_pi}-{_interp}')


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('pi', range(len(PROJ_ONLY)), ids=['x'.join(map(str, s)) for s in PROJ_ONLY])
def test_projection_stack_with_one_and_with_several_depth_segments(pi, interp):
    """Kernel 12 on an output with one depth segment and on one with five (the march over the tiles of a segment restarts the
    fixed-point coordinates per tile), every pixel against the float64 depth sum of the oracle's volume at TOL * depth."""
    t_start = time.time()
    oshape = PROJ_ONLY[pi]
    ii = ALL_INTERPS.index(interp)
    vol, src, kind = source(interp, 311 + pi)
    tol = TOL[interp] * oshape[0]
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    fails = Failures()
    try:
        for cases, ms in batches(selected(oshape, pi, ii, stride=2 + 2 * pi)):
            names = [c[0] for c in cases]
            want = np.stack([oracle.affine_ex(src, m64, kind, oshape).astype(np.float64).sum(axis=0) for _, m64, _ in cases])
            for flags in FLAGS:
                img = sv.projection_batch(ms, oshape, _flags=flags)
                info = sv.info()
                err = tol_failures(fails, img, want, tol, names, str(ms.dtype), flags, 'kernel', info.last_kernel)
                note(info, 12, interp, cases, err / oshape[0])
                fails.check((info.last_kernel == 12) == (flags == N.FORCE_TILED) or flags == 0, flags, 'projection_batch ran kernel', info.last_kernel)
            sv.projection_batch(ms[:1], oshape, _flags=N.FORCE_TILED)
            fails.check(segments_of(sv, oshape) == (1, 5)[pi], 'segments', segments_of(sv, oshape))
    finally:
        sv.close()
    NODES_RUN.add(f'proj-{pi}-{interp}')
    WALL[f'proj-{pi}-{interp}'] = time.time() - t_start
    fails.done()


SCIPY_INTERPS = list(TOL_EDGE)
for _interp in SCIPY_INTERPS:
    NODES_ALL.add(f'scipy-{_interp}')


@pytest.mark.parametrize('interp', SCIPY_INTERPS)
def test_edge_scipy_handles_on_chain_exact_box_cases(interp):
    """edge='scipy': the cut moves to s = 0 and s = dim - 1 (both inside).  Chain-exact cases only (scipy forms its coordinates in another
    order), kernels 11, 12 and 14 against device='cpu' at TOL_EDGE."""
    t_start = time.time()
    box = BOXES[0]
    ii = SCIPY_INTERPS.index(interp)
    vol = positive(rand_vol(SHAPE, 321))
    tol = TOL_EDGE[interp]
    tmpl, mask = template_and_mask(box)
    cpu = vt.StaticVolume(vol, interpolation=interp, device='cpu')
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    fails = Failures()
    n = 0
    try:
        for cases, ms in batches(selected(box, 0, ii, groups=('lattice', 'f32twin', 'face_scipy'), stride=2, exact_only=True)):
            n += len(cases)
            names = [c[0] for c in cases]
            want = np.asarray(cpu.extract(ms, box), np.float64)
            want_dot, bound_dot, _ = sums_and_bounds(want, tmpl, mask, tol)
            for flags in FLAGS:
                got = sv.extract(ms, box, _flags=flags)
                tol_failures(fails, got, want, tol, names, flags, 'edge=scipy extract, kernel', sv.info().last_kernel)
                img = sv.projection_batch(ms, box, _flags=flags)
                tol_failures(fails, img, want.sum(axis=1), tol * box[0], names, flags, 'edge=scipy projection_batch, kernel', sv.info().last_kernel)
                dots = sv.extract_dot(ms, tmpl, mask, _flags=flags)
                try:
                    check_dot(dots, want_dot, bound_dot, (interp, 'edge=scipy', flags))
                except AssertionError as e:
                    fails.check(False, flags, 'edge=scipy extract_dot', str(e)[:200])
    finally:
        sv.close()
    assert n >= 40
    NODES_RUN.add(f'scipy-{interp}')
    WALL[f'scipy-{interp}'] = time.time() - t_start
    fails.done()


def test_model_tile_and_box_dims_are_the_librarys():
    """tests/box_index_model.py cannot drift from the code: on single-matrix launches of kernel 11 its tile and staged dims are what
    vt_volume_info reports (last_tile, last_lds_dims, last_lds_bytes); for a batch last_lds_bytes is the largest entry's."""
    vol = rand_vol(SHAPE, 331)
    fails = Failures()
    n = 0
    for interp in ('linear', 'bspline'):
        sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
        try:
            for box in BOXES + ((32, 32, 32), (17, 23, 29)):
                cases = [c for j, c in enumerate(lc.box_cases(SHAPE, box, TEXTURE_GROUPS)) if j % 5 == 0]
                worst = 0
                for name, m64, t in cases:
                    res = bm.model(m64, box, interp, src_shape=SHAPE)
                    sv.extract(np.ascontiguousarray(m64[None]), box, _flags=N.FORCE_TILED)
                    info = sv.info()
                    n += 1
                    fails.check(info.last_kernel == 11 and tuple(info.last_tile) == res.tile, name, interp, box, 'tile', tuple(info.last_tile), res.tile)
                    fails.check(res.tiled and tuple(info.last_lds_dims) == res.L and info.last_lds_bytes == res.lds_bytes, name, interp, box,
                                'dims', tuple(info.last_lds_dims), info.last_lds_bytes, 'model', res.L, res.lds_bytes)
                    worst = max(worst, res.lds_bytes)
                f64 = np.ascontiguousarray(np.stack([m for _, m, t in cases if not t['f32']]))
                worst = max(bm.model(m, box, interp, src_shape=SHAPE).lds_bytes for m in f64)
                sv.extract(f64, box, _flags=N.FORCE_TILED)
                fails.check(sv.info().last_lds_bytes == worst, interp, box, 'batch lds bytes', sv.info().last_lds_bytes, worst)
        finally:
            sv.close()
    assert n >= 300
    fails.done()


def ledger_report():
    groups = (('lattice', 1), ('lattice', -1), ('lattice', 0), ('f32twin', None), ('face_exact', None), ('face_chain', None))
    lines = ['coverage ledger: cases in staged launches per (kernel, class, tile) x (group and sign of eps), whole / cut boxes']
    lines.append('%-28s' % 'kernel class tile' + ''.join('%14s' % (g + ('' if s is None else '0+-'[s])) for g, s in groups) + '%10s%10s' % ('whole', 'cut'))
    for k, c, tile in sorted({(key[0], key[1], key[4]) for key in LEDGER}):
        def count(g=None, s=None, wc=None):
            return sum(v for (kk, cc, gg, ss, tt, ww), v in LEDGER.items() if (kk, cc, tt) == (k, c, tile) and (g is None or gg == g) and
                       (s is None or ss == s) and (wc is None or ww == wc))
        lines.append('%-28s' % f'{k} {c} {"x".join(map(str, tile))}' + ''.join('%14d' % count(g, s) for g, s in groups) +
                     '%10d%10d' % (count(wc='whole'), count(wc='cut')))
    lines.append('largest |got - oracle| per (kernel, interpolation) [12: per plane of depth; 13: of the weighted sum; 14: worst err / bound x TOL]: ' +
                 ', '.join(f'{k}: {v:.3e}' for k, v in sorted(WORST.items())))
    lines.append('wall time per node (s): ' + ', '.join(f'{k}: {v:.2f}' for k, v in sorted(WALL.items())))
    return '\n'.join(lines)


def test_zz_coverage_ledger():
    """Each of kinds 11-16 served, for trilinear and for cubic, on every tile the planner gives that class: lattice cases with eps of
    either sign, float32 twins, face-exact and face-chain-dependent cases, with whole and cut boxes both present.  Last in the file;
    skips itself when only a selection of the file ran."""
    print('\n' + ledger_report())
    if NODES_RUN != NODES_ALL:
        pytest.skip(f'only {len(NODES_RUN)} of {len(NODES_ALL)} nodes ran: the ledger describes a selection')
    missing = []
    for k in (11, 12, 13, 14, 15, 16):
        for c, tiles in (('linear', ((8, 16, 16), (8, 8, 16))), ('cubic', ((8, 8, 16),))):
            for tile in tiles:
                for g, s in (('lattice', 1), ('lattice', -1), ('f32twin', None), ('face_exact', None), ('face_chain', None)):
                    if not any(v for (kk, cc, gg, ss, tt, _), v in LEDGER.items() if (kk, cc, gg, tt) == (k, c, g, tile) and (s is None or ss == s)):
                        missing.append((k, c, tile, g, s))
                for wc in ('whole', 'cut'):
                    if not any(v for (kk, cc, _, _, tt, ww), v in LEDGER.items() if (kk, cc, tt, ww) == (k, c, tile, wc)):
                        missing.append((k, c, tile, wc))
    assert not missing, missing
