"""The host model of the box kernels' tap indices (tests/box_index_model.py) on every box case of tests/lattice_cases.py and on the
random batches of the box suites: no tap of any voxel of any tile leaves the staged box [0, L).  CPU only (runs under -m "not gpu");
tests/test_gpu_box_lattice.py pins the model's tile and box dims to what the library reports, so the model cannot drift from the code.

`PARAMS_BEFORE` are the origin and extent rules the kernels had before kBoxMargin: the model shows taps at index -1 with them (a
coordinate that is exactly floor(lo) loses a few units of 2^-32 to the rounded depth increment and its integer part drops by one),
and none with the rules the kernels have now.
"""
import numpy as np
import pytest

import box_index_model as bm
import lattice_cases as lc

SHAPE = (96, 100, 104)
TILES_OF = {'linear': {(10, 18, 18): 2, (10, 26, 18): 1}, 'bspline': {(10, 18, 18): 2, (10, 26, 18): 2}}
PROJ_EXTRA = ((6, 18, 18), (40, 18, 18))          # one depth segment; five


def lead_matrix(row, offset=(40.0, 30.0, 30.0)):
    m = np.eye(4)
    m[0, :3] = row
    m[:3, 3] = offset
    return m


def test_planner_gives_these_tiles_and_no_others():
    """The boxes of the GPU test select tile 2 and tile 1 for trilinear and tile 2 for cubic, with two or more tiles and a ragged last
    tile on every axis; over a scan of box shapes the planner gives trilinear no other tile than 1 and 2 and cubic none but 2 (the cube,
    tile 0, pays the two-workgroups-per-CU penalty and never wins)."""
    for interp, boxes in TILES_OF.items():
        for box, cfg in boxes.items():
            got, _ = bm.extract_pick_tile(bm.is_cubic(interp), box)
            assert got == cfg, (interp, box, got)
            assert all(b > t and b % t for b, t in zip(box, bm.TILES[cfg])), (interp, box)
    seen = {False: set(), True: set()}
    for d in (1, 7, 8, 9, 16, 24, 33, 64, 96, 200):
        for h in (1, 8, 9, 16, 17, 32, 48, 65, 96, 200):
            for w in (1, 15, 16, 17, 32, 47, 64, 96, 200):
                for cubic in (False, True):
                    seen[cubic].add(bm.extract_pick_tile(cubic, (d, h, w))[0])
    assert seen == {False: {1, 2}, True: {2}}, seen
    assert bm.segments_of(False, PROJ_EXTRA[0]) == 1 and bm.segments_of(True, PROJ_EXTRA[0]) == 1
    assert bm.segments_of(False, PROJ_EXTRA[1]) == 5 and bm.segments_of(True, PROJ_EXTRA[1]) == 5
    assert bm.segments_of(False, (10, 18, 18)) == 2


def test_lead_rows_underflow_before_and_not_after():
    """The one-axis lead: matrix row (-0.8, 0.6, 0) at an integer offset on the 16^3 tile.  inc_lo = round(0.2 * 2^32) is 0.2 units low;
    after 15 depth steps the coordinate that is exactly floor(lo) has hi = floor(lo) - 1, lo = 2^32 - 3: 16 voxels read tap index -1 (and
    the row (-2/3, 2/3, -1/3): one voxel).  Offsets k - 2^-40 and k + 0.5 do not.  With the origin margin nothing does."""
    report = []
    for interp in ('linear', 'bspline'):
        for label, row, off, bad in (('345', (-0.8, 0.6, 0.0), 40.0, 16), ('thirds', (-2 / 3, 2 / 3, -1 / 3), 40.0, 1),
                                     ('345 - 2^-40', (-0.8, 0.6, 0.0), 40.0 - lc.P40, 0), ('345 + 0.5', (-0.8, 0.6, 0.0), 40.5, 0)):
            m = lead_matrix(row, (off, 30.0, 30.0))
            before = bm.model(m, (16, 16, 16), interp, cfg=0, params=bm.PARAMS_BEFORE)
            after = bm.model(m, (16, 16, 16), interp, cfg=0)
            report.append(f'{interp:8s} {label:12s} before: axis-0 taps [{before.lo[0]}, {before.hi[0]}] of L={before.L[0]}, {before.one_below} voxels below'
                          f' | after: [{after.lo[0]}, {after.hi[0]}] of L={after.L[0]}, {after.one_below} below')
            assert before.one_below == bad and (before.lo[0] == -1) == (bad > 0), (interp, label, before)
            assert before.hi[0] <= before.L[0] - 2, (interp, label, before)          # the slack the fix hands to the low side
            assert not bm.violations(after) and after.one_below == 0, (interp, label, after)
    print('\n' + '\n'.join(report))


def _sweep(cases, box, interp, params, cfgs=(None,), project=False):
    bad = []
    n = 0
    for name, m64, t in cases:
        m = m64.astype(np.float32).astype(np.float64) if t.get('f32') else m64
        for cfg in cfgs:
            res = bm.model(m, box, interp, src_shape=SHAPE, cfg=cfg, params=params, project=project)
            if not res.tiled:
                continue
            n += 1
            v = bm.violations(res)
            if v:
                bad.append((name, res.tile, v))
    return n, bad


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
@pytest.mark.parametrize('box', list(TILES_OF['linear']) + list(PROJ_EXTRA), ids=lambda b: 'x'.join(map(str, b)))
def test_every_box_case_stays_inside_the_staged_box(box, interp):
    """0 <= lowest and highest < L on every axis, and every address read inside the box, for every box case on the planner's tile and on
    the other two (kernels 11, 13-16), and for kernel 12's march over its depth segments."""
    cases = list(lc.box_cases(SHAPE, box))
    n, bad = _sweep(cases, box, interp, bm.PARAMS, cfgs=(None, 0, 1, 2))
    n12, bad12 = _sweep(cases, box, interp, bm.PARAMS, project=True)
    n0, bad0 = _sweep(cases, box, interp, bm.PARAMS_BEFORE)
    print(f'\n{box} {interp}: taps outside [0, L) before the origin margin on {len(bad0)} of {n0} cases (planner\'s tile; first: {bad0[:1]}), '
          f'now on {len(bad) + len(bad12)} of {n} + {n12} modelled launches (all three tiles; kernel 12)')
    assert n >= 3 * len(cases) and n12 == len(cases)
    assert not bad, bad[:5]
    assert not bad12, bad12[:5]


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_random_batches_of_the_box_suites_stay_inside(interp):
    """The batches of tests/test_gpu_extract.py (random rotations at fractional positions, faces, a corner, scales, a mirror, a shear) for
    all three tiles: entries a tile cannot stage are skipped as the planner skips them (they gather from global memory)."""
    from test_gpu_extract import BOXES, batch
    n = 0
    for shape in ((150, 170, 190), (96, 100, 104)):
        for box in (BOXES if shape == SHAPE else BOXES[:3]):          # (the 96-cube on one source: it is the slow one)
            for i, m in enumerate(batch(shape, box)):
                for cfg in (0, 1, 2):
                    res = bm.model(m.astype(np.float64), box, interp, src_shape=shape, cfg=cfg)
                    if res.tiled:
                        n += 1
                        assert not bm.violations(res), (shape, box, i, cfg, bm.violations(res))
    assert n >= 300


# ---- what a wrong kernel would do: CPU arguments for the checks of tests/test_gpu_box_lattice.py (no broken kernel is ever run) ---------
PLANNED = (((10, 18, 18), 2), ((10, 26, 18), 1), ((10, 26, 18), 2))          # (box, tile) pairs the GPU test launches


def _canonical_inside(m, box):
    s = lc.chain_coords(m, box)
    ins = np.ones(box, bool)
    for r in range(3):
        ins &= (s[r] >= -0.5) & (s[r] < SHAPE[r] - 0.5)
    return ins


def test_an_origin_one_too_high_is_seen_on_every_whole_case():
    """o = floor(lo) - HALO + 1 (as a negative origin margin of one voxel): the lowest tap is below the box on every lattice and twin
    case, on a tap that carries weight -- the GPU test's value check fails there (data >= 1; below the box lies another row or 0)."""
    too_high = bm.Params(-1.0, 0.0)
    for box, cfg in PLANNED[:2]:
        for interp in ('linear', 'bspline'):
            for name, m, t in list(lc.box_cases(SHAPE, box, ('lattice', 'f32twin')))[::7]:
                res = bm.model(m, box, interp, src_shape=SHAPE, cfg=cfg, params=too_high)
                assert min(res.lo) == -1 and res.one_below > 0, (name, res.lo)


@pytest.mark.parametrize('box,cfg', PLANNED)
def test_whole_without_the_margin_is_seen_by_the_margin_cases(box, cfg):
    """Every case of whole_margin_cases has a depth-complete tile that a bare comparison of its float64 bounding box calls inside while
    the canonical chain -- the oracle's -- puts voxels of it outside: a kernel that skipped the inside test there would return samples
    of positive data where the oracle has 0, which the mask equality of the GPU test sees.  With kTileMargin the model calls none of
    these tiles whole, and their taps stay inside the staged box."""
    cases = bm.whole_margin_cases(SHAPE, box, cfg)
    assert len(cases) >= 8
    for name, m, t in cases:
        ins = _canonical_inside(m, box)
        T = bm.TILES[cfg]
        fooled = [(d0, h0, w0) for d0, h0, w0 in bm.tiles_whole_without_margin(m, box, cfg, SHAPE)
                  if not ins[d0:d0 + T[0], h0:h0 + T[1], w0:w0 + T[2]].all()]
        assert fooled and t['fooled'] > 0 and not t['whole'], name
        for interp in ('linear', 'bspline'):
            res = bm.model(m, box, interp, src_shape=SHAPE, cfg=cfg)
            assert not bm.violations(res), (name, bm.violations(res))
            assert res.whole <= res.tiles - len(fooled), (name, res.whole, res.tiles, fooled)


def test_an_inside_test_on_the_fixed_point_coordinate_is_seen_by_the_face_chain_cases():
    """The Q32.32 coordinate truncated by to_fx agrees with the canonical chain at a column's first plane (the cuts lie on the 2^-32 grid)
    but not after steps with a rounded increment: on the face-chain cases an inside test taken from it changes the side of hundreds of
    voxels, each of which the mask equality of the GPU test sees; on chain-exact cases (dyadic parts: exact increments) of none."""
    for box, cfg in PLANNED:
        flipped = cases = 0
        for name, m, t in lc.box_cases(SHAPE, box, ('face_chain', 'face_exact')):
            n = int((bm.inside_by_fixed_point(m, box, cfg, SHAPE) != _canonical_inside(m, box)).sum())
            if t['exact']:
                assert n == 0, (name, n)
            elif n:
                flipped, cases = flipped + n, cases + 1
        print(f'\n{box} tile {bm.TILES[cfg]}: a fixed-point inside test changes the side of {flipped} voxels on {cases} face-chain cases')
        assert cases >= 5 and flipped >= 100, (box, cfg, cases, flipped)
