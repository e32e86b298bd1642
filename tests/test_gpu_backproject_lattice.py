"""-m gpu: StaticVolume.backproject (kernel 18) on integer-lattice, skirt-face and tile-margin coordinates (tests/backproject_cases.py),
against the float64 model of tests/backproject_model.py.

tests/test_gpu_backproject.py draws everything from one batch in which, the identity apart, no voxel lies on an integer image coordinate
and none on y = -0.5, y = H - 0.5, x = -0.5 or x = W - 0.5.  Here a known share of every entry's voxels sits within 2^-50 .. 2^-20 of an
integer y or x, whole rows and columns sit exactly on the hard cut of the inside test, and the margin cases hold tiles whose float64
bounding box is inside by a bare comparison while the chain puts a voxel outside (tests/test_backproject_cases_host.py asserts all of
that without a GPU).  What that attacks: the patch origin lowered by kBoxMargin, the Q32.32 coordinate restarted per tile and stepped
along depth (the taps) against the canonical float64 chain (the inside test), and the "whole" tiles that skip the inside test when they
clear the skirt by kTileMargin.

Source data in [1, 2): under the non-negative interpolations an inside voxel is strictly positive, so `got != 0` must equal the model's
inside mask voxel for voxel.  Per node (output shape x interpolation), flags 0 and FORCE_DIRECT, float64 batches through the float64
entry point and the float32 twins as float32, no new tolerance:
  * every entry alone with weight 1: |got - B_i| <= TOL[interp] on every voxel; the mask equality (linear, bspline, bspline_simple);
  * all entries as one batch with mixed-sign weights: check_sum of tests/test_gpu_place.py;
  * linear: bit identity with place on the plane-row matrices.
The coverage ledger at the end counts (interpolation class, group, sign of eps, tile, whole / cut) over staged launches
(info.last_lds_dims[1] > 0) and asserts every class that tests/test_backproject_cases_host.py says exists.  backproject_entry_point's
(16, 16, 16) configuration is absent from it on purpose: extract_pick_tile's rule gives it to no output shape (asserted there).
"""
import collections
import functools
import time

import numpy as np
import pytest

import backproject_cases as bc
import backproject_model as bm
import voltools_amd as vt
from voltools_amd import _native
from test_backproject_cases_host import kinds_present
from test_gpu_backproject import plane_rows
from test_gpu_box_lattice import Failures, bits32, positive
from test_gpu_extract import TOL, ALL_INTERPS, rand_vol
from test_gpu_place import check_sum

pytestmark = pytest.mark.gpu

FLAGS = (0, _native.FORCE_DIRECT)
STRIDE = 2                                          # a node takes every second case of each group, shifted from node to node
POSITIVE = ('linear', 'bspline', 'bspline_simple')  # non-negative weights on the data itself: zeros are the outside

LEDGER = collections.Counter()                      # ('linear' | 'cubic', group, sign of eps, tile, 'whole' | 'cut') -> entries in staged launches
WORST = {}                                          # (interp, what) -> largest error / bound
WALL = {}
NODES_RUN = set()
NODES_ALL = {f'{oi}-{interp}' for oi in range(len(bc.OUTS)) for interp in ALL_INTERPS}


@functools.lru_cache(maxsize=None)
def stack():
    s = positive(rand_vol(bc.STACK, 401))
    s.setflags(write=False)
    return s


def batches(cases):
    """[(cases, matrices)]: the float64 cases as a float64 batch, the float32 twins as a float32 batch."""
    res = []
    for f32 in (False, True):
        mine = [c for c in cases if c[2]['f32'] == f32]
        if mine:
            res.append((mine, np.ascontiguousarray(np.stack([m for _, m, _ in mine]), dtype=np.float32 if f32 else np.float64)))
    return res


def mixed_weights(n):
    return ((np.arange(n) % 5) - 2) * 0.5 + 0.25                           # -0.75, -0.25, 0.25, 0.75, 1.25, ...


def note(interp, tile, t, mask):
    group = 'margin' if t.get('margin') else t['group']
    whole, cut = bc.tile_kinds(mask, tile)
    for s in bc.eps_signs(t):
        for kind, present in (('whole', whole), ('cut', cut), ('any', True)):
            if present:
                LEDGER[(bc.icls(interp), group, s, tile, kind)] += 1


def worst(interp, what, ratio):
    WORST[(interp, what)] = max(WORST.get((interp, what), 0.0), float(ratio))


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('oi', range(len(bc.OUTS)), ids=['x'.join(map(str, o)) for o in bc.OUTS])
def test_backproject_on_lattice_face_and_margin_cases(oi, interp):
    t_start = time.time()
    out = bc.OUTS[oi]
    ii = ALL_INTERPS.index(interp)
    tile = bc.tile_of(bc.icls(interp), out)
    tol = TOL[interp]
    margin = bc.whole_margin_cases(out, tile)
    sv = vt.StaticVolume(stack(), interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))
    fails = Failures()
    try:
        fails.check(len(margin) >= 8, 'margin cases', len(margin))
        for cases, ms in batches(bc.selected(out, oi, ii, STRIDE) + margin):
            n = len(cases)
            names = [c[0] for c in cases]
            dt = str(ms.dtype)
            planes = bc.planes_of(n)
            vols, masks = bm.per_entry(stack(), ms.astype(np.float64), planes, out, interp)
            w = mixed_weights(n)
            for flags in FLAGS:
                # ---- every entry alone, weight 1 ----
                top = 0.0
                for i in range(n):
                    got = sv.backproject(ms[i:i + 1], out, [1.0], planes=planes[i:i + 1], _flags=flags)
                    info = sv.info()
                    fails.check(info.last_kernel == 18 and tuple(info.last_tile) == tile, names[i], dt, flags, 'kernel / tile',
                                info.last_kernel, tuple(info.last_tile))
                    staged = info.last_lds_dims[1] > 0
                    fails.check(staged == (flags == 0), names[i], dt, flags, 'staged', tuple(info.last_lds_dims))
                    err = float(np.abs(got.astype(np.float64) - vols[i]).max())
                    top = max(top, err)
                    fails.check(err <= tol, names[i], dt, flags, 'err', err, 'tol', tol)
                    if interp in POSITIVE:
                        differs = int(((got != 0) != masks[i]).sum())
                        fails.check(differs == 0, names[i], dt, flags, 'inside mask differs on', differs, 'voxels')
                    if staged:
                        note(interp, tile, cases[i][2], masks[i])
                print(f'{interp} {out} {dt} flags {flags}: {n} entries alone, max|hip - model| {top:.3e}  bound {tol:.1e}')
                worst(interp, 'entry', top / tol)
                # ---- the batch, mixed-sign weights ----
                total = sv.backproject(ms, out, w, planes=planes, _flags=flags)
                want = np.tensordot(w, vols, axes=1)
                worst(interp, 'batch', (np.abs(total - want) / (np.abs(w).sum() * tol + 2.0 ** -23 * np.abs(want))).max())
                try:
                    check_sum(total, vols, w, tol, (interp, out, dt, flags))
                except AssertionError as e:
                    fails.check(False, dt, flags, 'batch', str(e)[:200])
                # ---- linear: place's bits on the plane-row matrices ----
                if interp == 'linear':
                    placed = sv.place(plane_rows(ms, planes), out, w, _flags=flags)
                    fails.check(sv.info().last_kernel == 17 and total.any() and np.array_equal(bits32(total), bits32(placed)),
                                dt, flags, 'backproject != place on plane rows')
    finally:
        sv.close()
    NODES_RUN.add(f'{oi}-{interp}')
    WALL[f'{oi}-{interp}'] = time.time() - t_start
    fails.done()


def ledger_report():
    cols = (('lattice', 1), ('lattice', -1), ('lattice', 0), ('f32twin', 1), ('f32twin', -1), ('face_exact', None), ('face_chain', None),
            ('margin', None))
    lines = ['coverage ledger: entries in staged launches per (class, tile) x (group and sign of eps), with a whole tile / with a cut tile']
    lines.append('%-22s' % 'class tile' + ''.join('%13s' % (g + ('' if s is None else '0+-'[s])) for g, s in cols) + '%9s%9s' % ('whole', 'cut'))
    for c, tile in sorted({(k[0], k[3]) for k in LEDGER}):
        def count(g=None, s=None, kind='any'):
            return sum(v for (cc, gg, ss, tt, kk), v in LEDGER.items() if (cc, tt, kk) == (c, tile, kind) and (g is None or gg == g) and
                       (s is None or ss == s))
        lines.append('%-22s' % f'{c} {"x".join(map(str, tile))}' + ''.join('%13d' % count(g, s) for g, s in cols) +
                     '%9d%9d' % (count(kind='whole'), count(kind='cut')))
    lines.append('no output shape selects the (16, 16, 16) configuration (tests/test_backproject_cases_host.py): it has no row')
    lines.append('worst error / bound per (interpolation, check): ' + ', '.join(f'{k[0]} {k[1]}: {v:.3f}' for k, v in sorted(WORST.items())))
    lines.append('wall time per node (s): ' + ', '.join(f'{k}: {v:.2f}' for k, v in sorted(WALL.items())))
    return '\n'.join(lines)


def test_zz_coverage_ledger():
    """Every group met, in a staged launch, every tile its class is given -- eps of either sign for the lattice groups -- as a whole tile
    and as a cut tile wherever tests/test_backproject_cases_host.py says such tiles exist.  Last in the file; skips itself when only a
    selection of the file ran."""
    print('\n' + ledger_report())
    if NODES_RUN != NODES_ALL:
        pytest.skip(f'only {len(NODES_RUN)} of {len(NODES_ALL)} nodes ran: the ledger describes a selection')
    missing = []
    for cls in ('linear', 'cubic'):
        for out in bc.OUTS:
            tile = bc.tile_of(cls, out)
            present = kinds_present(out, tile)

            def met(g, s=None, kind='any'):
                return any(v for (cc, gg, ss, tt, kk), v in LEDGER.items() if (cc, gg, tt, kk) == (cls, g, tile, kind) and (s is None or ss == s))
            for g, s in (('lattice', 1), ('lattice', -1), ('f32twin', 1), ('f32twin', -1), ('face_exact', None), ('face_chain', None),
                         ('margin', None)):
                if not met(g, s):
                    missing.append((cls, tile, g, s))
            for g in bc.GROUPS:
                for k, kind in enumerate(('whole', 'cut')):
                    if present[g][k] and not met(g, None, kind):
                        missing.append((cls, tile, g, kind))
    assert not any(k[3] == (16, 16, 16) for k in LEDGER)
    assert not missing, missing
