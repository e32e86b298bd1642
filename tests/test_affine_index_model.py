"""The host model of the general-matrix kernels' tap indices (tests/affine_index_model.py: kinds 2, 9 and 6) on every case of
tests/lattice_cases.py and on the random general matrices of the GPU suites: no tap of any voxel of any tile leaves what the tile
staged.  CPU only (runs under -m "not gpu"); tests/test_gpu_affine_index.py pins the model's tile, box dims and LDS bytes to what the
library reports, so the model cannot drift from the code.

`PARAMS_BEFORE` is the bare `o = floor(lo) - HALO`, `L = floor(ext) + 3 + halo2` these three kernels kept after the box kernels (kinds
11-16) got kBoxMargin: the model shows taps at box index -1 with it on all three (a coordinate that is exactly floor(lo) loses a few
units of 2^-32 to the rounded increments and its integer part drops by one), and none with the rules the kernels have now.  The counts
are printed, not asserted: they are whatever the model finds.
"""
import os
import re

import numpy as np
import pytest

import affine_index_model as am
import lattice_cases as lc
from test_box_index_model import lead_matrix

SHAPES = ((70, 66, 72), (33, 47, 50))          # the two smallest of test_gpu_lattice.SHAPES
KINDS = (2, 9, 6)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'voltools_amd', 'csrc')


def matrix_of(m64, t):
    return m64.astype(np.float32).astype(np.float64) if t.get('f32') else m64


def sweep(kind, shape, interp, params, cases, **force):
    """(modelled launches, [(name, tile, violations)], launches whose box grew against PARAMS_BEFORE)."""
    n, bad, grew = 0, [], 0
    for name, m64, t in cases:
        m = matrix_of(m64, t)
        res = am.model(kind, m, shape, interp, params=params, **force)
        if not res.tiled:
            continue
        n += 1
        v = am.violations(res)
        if v:
            bad.append((name, res.tile, v))
        if params is am.PARAMS:
            old = am.plan_of(kind, m, am.is_cubic(interp), am.PARAMS_BEFORE, **force)
            if old is None or old['reported'] != res.reported or old['tile'] != res.tile:
                grew += 1
                # the planner's own limit tests, with the planner's arithmetic, on the grown box
                assert res.lds_bytes <= am.LDS_CAP, (name, res.lds_bytes)
                if kind == 9:
                    assert res.alloc // 4 <= 256 * am.BLK_MAX_IT[res.tile[1]], (name, res.alloc)
                if kind == 6:
                    assert res.plan['nvec'] * 4 <= res.alloc and res.alloc // 4 <= 256 * am.PACK_MAX_IT, (name, res.alloc)
    return n, bad, grew


def test_lead_rows_underflow_before_and_not_after():
    """The known answer of test_box_index_model, carried over to kind 2 (the 16^3 tile of affine_tiled is the same chain: one lane group,
    16 planes per column): matrix row (-0.8, 0.6, 0) at an integer offset.  inc_lo = round(0.2 * 2^32) is 0.2 units low; after 15 steps the
    coordinate that is exactly floor(lo) has hi = floor(lo) - 1: 16 voxels read tap index -1 (and the row (-2/3, 2/3, -1/3): one voxel).
    Offsets k - 2^-40 and k + 0.5 do not.  With the origin margin nothing does, and setting the origin margin alone back to 0 brings the
    16 voxels back: the model looks at what the fix touches."""
    report = []
    extent_only = am.Params(0.0, am.PARAMS.extent_margin)
    for interp in ('linear', 'bspline'):
        for label, row, off, bad in (('345', (-0.8, 0.6, 0.0), 40.0, 16), ('thirds', (-2 / 3, 2 / 3, -1 / 3), 40.0, 1),
                                     ('345 - 2^-40', (-0.8, 0.6, 0.0), 40.0 - lc.P40, 0), ('345 + 0.5', (-0.8, 0.6, 0.0), 40.5, 0)):
            m = lead_matrix(row, (off, 30.0, 30.0))
            before = am.model(2, m, (16, 16, 16), interp, src_shape=(96, 100, 104), params=am.PARAMS_BEFORE, cfg=0)
            after = am.model(2, m, (16, 16, 16), interp, src_shape=(96, 100, 104), cfg=0)
            half = am.model(2, m, (16, 16, 16), interp, src_shape=(96, 100, 104), params=extent_only, cfg=0)
            report.append(f'{interp:8s} {label:12s} before: axis-0 taps [{before.lo[0]}, {before.hi[0]}] of L={before.plan["used"][0]}, {len(before.below)} voxels '
                          f'below | after: [{after.lo[0]}, {after.hi[0]}] of L={after.plan["used"][0]}, {len(after.below)} below')
            assert len(before.below) == bad and (before.lo[0] == -1) == (bad > 0), (interp, label, before.lo, len(before.below))
            assert before.hi[0] <= before.plan['used'][0] - 2, (interp, label, before.hi)          # the slack the fix hands to the low side
            assert not am.violations(after) and not after.below, (interp, label, am.violations(after))
            assert len(half.below) == bad and bool(am.violations(half)) == (bad > 0), (interp, label, 'origin margin 0', len(half.below))
            if bad:
                # a tap on axis 0 at index -1 is an address below the allocation
                assert all(f < 0 for b in before.below for _, f in b.reads), (interp, label)
    print('\n' + '\n'.join(report))


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_every_lattice_case_stays_inside_what_was_staged(shape, kind, interp):
    """Every case of lattice_cases.cases(shape), float32 twins as float32-rounded matrices, on the tile the planner picks when the family is
    forced: 0 <= lowest and highest tap < L on every axis, every address read inside the allocation, every tap on a cell the tile staged
    (kinds 9 and 6 stage footprint rows, not the box) and, for kind 6, through a row-table entry that exists.  The highest tap stays
    <= L - 1 although the fix hands the planner's one voxel of slack to the low side.  Where the extent margin grows a box, the planner's own
    limits still hold (inside sweep())."""
    cases = list(lc.cases(shape))
    n0, bad0, _ = sweep(kind, shape, interp, am.PARAMS_BEFORE, cases)
    n, bad, grew = sweep(kind, shape, interp, am.PARAMS, cases)
    print(f'\nkind {kind} {interp} {shape}: taps outside the staged image under o = floor(lo) - HALO on {len(bad0)} of {n0} launches '
          f'(first: {bad0[:1]}); with kBoxMargin on {len(bad)} of {n}; boxes the extent margin grew: {grew}')
    assert n == n0 and n >= 0.9 * len(cases), (n, n0, len(cases))
    assert not bad, bad[:5]


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_every_tile_configuration_stays_inside(interp):
    """The tiles the planner does not pick for these matrices but can for others: all five of tile_config() (kind 2), the full-height
    lane-block tile with and without footprint trimming (kind 9), all three of packed_config() (kind 6); every third case of the smaller
    shape (a configuration whose box does not fit is skipped as the planner skips it)."""
    shape = SHAPES[1]
    cases = list(lc.cases(shape))[::3]
    total = 0
    for kind, forces in ((2, [dict(cfg=c) for c in range(len(am.AFFINE_TILES))]), (9, [dict(th=16), dict(th=16, trim=False), dict(th=8, trim=False)]),
                         (6, [dict(cfg=c) for c in range(len(am.PACK_TILES))])):
        for force in forces:
            n, bad, _ = sweep(kind, shape, interp, am.PARAMS, cases, **force)
            assert not bad, (kind, force, bad[:5])
            total += n
    assert total >= 8 * len(cases), total


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_random_general_matrices_stay_inside(interp):
    """The general and affine draws of tests/test_gpu_fuzz.py (random rotations; rotation + scale + shear) and the matrices of
    tests/test_gpu_ranges.py, on all three kernels."""
    from test_gpu_fuzz import random_matrix
    from test_gpu_ranges import matrices
    shape = SHAPES[1]
    ms = [np.asarray(m, np.float64) for m in matrices(shape).values()]
    for seed in range(12):
        rs = np.random.RandomState(1000 + seed)
        ms += [np.asarray(random_matrix(rs, shape, k), np.float64) for k in ('general', 'affine')]
    n = 0
    for kind in KINDS:
        for m in ms:
            res = am.model(kind, m, shape, interp)
            if res.tiled:
                n += 1
                assert not am.violations(res), (kind, m.tolist(), am.violations(res))
    assert n >= 2 * len(ms), n


def test_an_origin_one_too_high_is_seen_by_every_kernel():
    """o = floor(lo) - HALO + 1 (a negative origin margin of one voxel): taps that carry weight leave the box, on all three kernels."""
    too_high = am.Params(-1.0, 0.0)
    shape = SHAPES[1]
    for kind in KINDS:
        for name, m, t in list(lc.cases(shape, ('lattice',)))[::40]:
            res = am.model(kind, m, shape, 'bspline', params=too_high)
            assert res.tiled and min(res.lo) <= -1 and am.violations(res), (kind, name, res.lo)


def _poison_cases():
    for (kind, icls), lst in sorted(am.POISON_CASES.items()):
        for si, name in lst:
            shape = SHAPES[si]
            table = {n: matrix_of(m64, t) for n, m64, t in lc.cases(shape)}
            m = table[name] if name in table else dict(am.lead_cases(shape))[name]
            yield kind, ('linear' if icls == 'linear' else 'bspline'), shape, name, m


def test_poison_cases_hold_their_condition():
    """Every entry of POISON_CASES: under PARAMS_BEFORE the model lists output voxels below the box whose wrapped read lies inside the
    allocation on a staged source voxel inside the volume (what tests/test_gpu_affine_index.py poisons), every family and class the model
    finds one for has an entry (the lane-block kernel's cubic form has none: see POISON_CASES), and under PARAMS no voxel is below the box.
    The fixed-point contract the GPU test's rule rests on, on the same launches: the floor tap of every output voxel is the floor of its
    float64 chain coordinate or one beside it, and one beside it only within 2^-24 of an integer."""
    assert set(am.POISON_CASES) == {(2, 'linear'), (2, 'cubic'), (6, 'linear'), (6, 'cubic'), (9, 'linear')}
    for kind, interp, shape, name, m in _poison_cases():
        pp = am.poison_plan(kind, m, shape, interp)
        assert len(pp['listed']) >= 1 and len(pp['poison']) >= 1, (kind, interp, name)
        assert not pp['allowed'][tuple(pp['listed'].T)].any(), (kind, interp, name)
        mr, sshape, pi = am.reoriented(m, shape)
        res = am.model(kind, mr, shape, interp, src_shape=sshape, origins=True)
        if not res.tiled:
            mr, sshape, pi = m, shape, (0, 1, 2)
            res = am.model(kind, mr, shape, interp, src_shape=sshape, origins=True)
        assert res.tiled and not res.below and not am.violations(res), (kind, interp, name)
        s = lc.chain_coords(mr, shape)
        f = np.floor(s)
        staged = res.origin[0] > np.iinfo(np.int64).min
        d = (res.origin - f.astype(np.int64))[:, staged]
        frac = (s - f)[:, staged]
        assert np.abs(d).max() <= 1, (kind, interp, name)
        assert np.all(frac[d == -1] < 2.0 ** -24) and np.all(frac[d == 1] > 1.0 - 2.0 ** -24), (kind, interp, name)


def test_inplane_origin_of_the_per_pixel_kernels():
    """Kinds 8, 3, 4, 5 place their in-plane box by floor(lo) too, but form the in-plane coordinate once per pixel from the float64 chain:
    no Q32.32 stepping, only the double rounding of `base + neg` (a sum of rounded products) against the pixel's own fma chain can put
    floor(coordinate) below the origin.  It does: with the bare floor(lo) the check finds pixels one below the box on the tables (row
    (0, 0.6, -0.8): -0.8 * 31 rounds to -24.8 while the chain gives base - 24.800000000000001).  Every one of them is exactly one below with
    a float32 fraction of 1.0f -- a zero-weight tap.  The kernels of the test build index a box with it (kinds 3, 4, 5): they get the origin
    margin, with which no pixel is below.  The plane-quad kernel (kind 8) keeps the bare floor: it clamps its row index to [0, kRowsMax) and
    takes each row's columns from the pixels' own integer indices, so the tap lands on row 0 of the box (the pixel's own floor row) or on the
    source column floor - 1 -- inside what it staged (pinned to its source below)."""
    tiles = ((16, 32), (8, 32), (32, 32), (16, 64), (32, 64), (16, 16), (8, 16))
    n = hits = with_margin = 0
    for shape in SHAPES:
        for name, m64, t in lc.cases(shape):
            if t['family'] == 'general':
                continue
            a = int(t['family'][-1])
            for rest in ([k for k in range(3) if k != a], [k for k in range(2, -1, -1) if k != a]):
                perm = [a] + rest
                m = np.eye(4)
                m[:3, :3] = matrix_of(m64, t)[:3, :3][np.ix_(perm, perm)]
                m[:3, 3] = matrix_of(m64, t)[:3, 3][perm]
                oshape = tuple(shape[k] for k in perm)
                for th, tw in tiles:
                    for cubic in (False, True):
                        n += 1
                        bad = am.inplane_origin_check(m, oshape, th, tw, cubic)
                        hits += len(bad)
                        assert all(b[3] == -1 and b[4] == 1.0 for b in bad), (name, th, tw, cubic, bad[:3])
                        if bad:
                            with_margin += len(am.inplane_origin_check(m, oshape, th, tw, cubic, am.BOX_MARGIN))
    print(f'\nin-plane origin of kinds 8 / 3 / 4 / 5: {hits} pixels one below the box (all with fraction 1.0f) over {n} (case, orientation, tile, '
          f'class) combinations under the bare floor(lo); {with_margin} with the origin margin')
    assert n >= 5000 and with_margin == 0


# ---- pinned to the sources ---------------------------------------------------------------------------------------------------------
def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _table(text, name):
    body = re.search(name + r'\[\] = \{(.*?)\};', text, re.S).group(1)
    return tuple(tuple(int(x) for x in row.split(',')) for row in re.findall(r'\{([^{}]*)\}', body))


def test_model_constants_and_origin_expressions_match_the_sources():
    """The constants the model repeats and the origin / extent expressions, grepped from the .hip / .h text: an edit of the kernels fails
    here instead of silently diverging from the model."""
    affine, block, packed, plan, dev = (_src(n) for n in ('vt_kernels_affine.hip', 'vt_kernels_block.hip', 'vt_kernels_packed.hip', 'vt_plan.hip',
                                                           'vt_device.h'))
    assert _table(affine, 'kTiles') == am.AFFINE_TILES
    assert _table(packed, 'kPack') == am.PACK_TILES
    assert f'constexpr int kPackMaxIt = {am.PACK_MAX_IT};' in packed and f'constexpr int kPackRowsMax = {am.PACK_ROWS_MAX};' in packed
    assert f'constexpr int kBlkTD = {am.BLK_TD}, kBlkTW = {am.BLK_TW};' in block
    assert 'static const int kBlkRS[] = {%s};' % ', '.join(map(str, am.BLK_RS)) in block
    assert 'static const int kOrder16[] = {%s};' % ', '.join(map(str, am.BLK_ORDER[16])) in block
    assert 'static const int kOrder8[] = {%s};' % ', '.join(map(str, am.BLK_ORDER[8])) in block
    assert f'return th == 16 ? {am.BLK_MAX_IT[16]} : {am.BLK_MAX_IT[8]};' in block
    assert 'constexpr int which[7] = {0, TH == 16 ? 1 : 3, 2, 3, 0, 4, 2};' in block
    assert 'c[r] = to_fx((base[r] - (double)o[r]) + toff[r]);' in block
    assert 'constexpr double kBoxMargin = 0x1p-24;' in dev and am.BOX_MARGIN == 2.0 ** -24
    assert 'constexpr double kTileMargin = 1.0e-6;' in dev and am.TILE_MARGIN == 1.0e-6
    assert 'r.lo = (unsigned)((x - fl) * 4294967296.0);' in dev
    # the origin: one expression in each of the three kernels, with the margin
    origin = 'for (int r = 0; r < 3; ++r) o[r] = (int)floor(lo[r] - kBoxMargin) - HALO;'
    for text in (affine, block, packed):
        assert text.count(origin) == 1 and 'o[r] = (int)floor(lo[r]) - HALO' not in text
        assert 'o[2] &= ~3;' in text
    # the extent: floor(ext + 2 kBoxMargin) + 3 + halo2 for the box and lane-block planners and the packed kernel's branch of PackGeom's
    assert plan.count('L[r] = (int)std::floor(ext + 2.0 * kBoxMargin) + 3 + c.halo2;') == 2
    assert 'L[r] = (int)std::floor(ext + (span ? 1.0e-8 : 2.0 * kBoxMargin)) + 3 + c.halo2;' in plan
    assert 'L[r] = (int)std::floor(ext) + 3 + c.halo2' not in plan
    assert plan.count('L[2] = (L[2] + 3 + 3) & ~3;') >= 2 and 'const int lx_used = (L[2] + 3 + 3) & ~3;' in plan
    for cap in ('if (!(ext < 4096.0)) { ok = false; break; }', 'if (!(ext < 256.0)) return false;', 'if (!(ext < 1000.0)) { ok = false; break; }'):
        assert cap in plan
    assert 'const int cap_vec_' not in plan and 'int cap_vec = nvec + rows / 16 + 8;' in plan
    assert 'const int table_floats = span ? (pipe ? 4 * rows + 84 : 4 * rows + 8) : (2 * rows + 8 + 3) & ~3;' in plan
    assert 'const int box_bytes = (int)((vectors + 63) / 64 * 64 * 16);' in plan and 'const int lds_bytes = box_bytes + 16;' in plan
    # the per-pixel kernels: the test build's box-indexing ones carry the margin, the plane-quad kernel its row clamp and integer spans
    march, quad = _src('vt_kernels_march.hip'), _src('vt_kernels_quad.hip')
    assert march.count('const int o1 = (int)floor(lo[1] - kBoxMargin) - HALO;') == 2 and 'floor(lo[1])' not in march and 'floor(lo[2])' not in march
    assert 'o[1] = (int)floor(lo[1] - kBoxMargin) - HALO;' in affine and 'o[2] = ((int)floor(lo[2] - kBoxMargin) - HALO) & ~3;' in affine
    assert plan.count('inplane_box(m, th, tw, c.halo2, L, 2.0 * kBoxMargin)') == 2 and 'L[r] = (int)std::floor(ext + margin) + 3 + halo2;' in plan
    assert 'const int f1 = (int)floor(lo[1]), f2 = (int)floor(lo[2]);' in quad
    assert quad.count('const int row = min(max(iy[px] - HALO + r, 0), kRowsMax - 1);') == 2
    assert 'atomicMin(&tab[row], ix[px] - HALO);' in quad and 'atomicMax(&tab[kRowsMax + row], ix[px] + HALO + 1);' in quad
