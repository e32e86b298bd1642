"""The lattice, face and tile-margin cases of tests/backproject_cases.py, checked without a GPU: what makes them adversarial for
StaticVolume.backproject (kernel 18), and how many of them there are.  This file is the only place where case counts and minimum shares
are fixed; everything counted comes from tests/backproject_model.py and the project's oracle, never from the library.

  * per group and output shape, how many cases survive the filter "the property lies on image axis 1 or 2";
  * lattice groups: the share of voxels whose y or x lies within the case's eps of an integer, eps of either sign;
  * face_exact: whole rows or columns of voxels with y + 0.5 == 0, y + 0.5 == H or the x counterparts (exact in float64: the matrices
    are dyadic), the equality at 0 inside, the equality at H / W outside;
  * face_chain and the margin cases: the model's mask is the oracle's inside decision on every voxel (positive data, trilinear at an
    integer plane: the tie of tests/test_backproject_host.py);
  * margin cases: tiles whose float64 bounding box on rows 1 and 2 is inside by a bare comparison while the chain puts a voxel outside;
  * which cases hold whole tiles and tiles cut by the skirt, per tile: what the GPU file's ledger must have met;
  * the (16, 16, 16) configuration of backproject_entry_point: no output shape selects it;
  * stage_patch's walk over a patch with its single wrap of cx, and what two wrong walks would do to the patches the GPU tests stage.
"""
import itertools

import numpy as np
import pytest

import backproject_cases as bc
import backproject_model as bm
import box_index_model as bi
import lattice_cases as lc
from oracle import oracle
from test_lattice_cases import ROUNDING

T, H, W = bc.STACK
DIM = {1: H, 2: W}
# cases left by the axis filter, per group (the same on both output shapes: the filter reads the spec, not the placement)
MIN_KEPT = {'lattice': 120, 'f32twin': 20, 'face_exact': 70, 'face_chain': 45}
MIN_SHARE = 0.5                # of the share 1 / q the lattice predicts (tests/test_lattice_cases.py: a box axis of 10 voxels and q = 5)
MIN_MARGIN = 8                 # margin cases per (output, tile)
MIN_FACE_LINES = 4             # face_exact cases with eps = 0 per (axis, side): FACE_EPS holds five values, so a fifth of the ~ 20 cases per
                               # (axis, side) put their line exactly on the face
# cases that hold a depth-complete all-inside tile / a tile cut by the skirt, per group, on every (output, tile)
MIN_WHOLE = {'lattice': 120, 'f32twin': 20, 'face_exact': 55, 'face_chain': 30}
MIN_CUT = {'lattice': 0, 'f32twin': 0, 'face_exact': 50, 'face_chain': 40}       # (a face line at the first voxel with eps >= 0 cuts nothing)
OUT_IDS = ['x'.join(map(str, o)) for o in bc.OUTS]


def plane_row(m, plane):
    p = np.array(m, np.float64)
    p[0] = (0.0, 0.0, 0.0, float(plane))
    return p


def positive_stack(seed=7):
    unit = np.random.RandomState(seed).random_sample(bc.STACK).astype(np.float32)
    vol = np.minimum(unit + np.float32(1.0), np.nextafter(np.float32(2.0), np.float32(0.0))).astype(np.float32)
    assert vol.min() >= 1.0 and vol.max() < 2.0
    return vol


def kinds_present(out, tile):
    """{group: (cases with a whole tile, cases with a cut tile)} on one (output, tile), by the model's masks."""
    res = {}
    for g in bc.GROUPS:
        kinds = [bc.tile_kinds(bc.mask_of(m, out)[0], tile) for _, m, _ in bc.kept(out, g)]
        res[g] = (sum(k[0] for k in kinds), sum(k[1] for k in kinds))
    return res


def tiles_met(out):
    return sorted({bc.tile_of(cls, out) for cls in ('linear', 'cubic')})


@pytest.mark.parametrize('out', bc.OUTS, ids=OUT_IDS)
def test_axis_filter_keeps_enough_of_every_group(out):
    for g in bc.GROUPS:
        cases = bc.kept(out, g)
        everything = list(lc.box_cases(bc.STACK, out, (g,)))
        print(g, len(cases), 'of', len(everything))
        assert len(cases) >= MIN_KEPT[g], (g, len(cases))
        assert len(cases) < len(everything)                          # the filter drops the axis-0 cases
        dropped = [t for _, _, t in everything if not bc.on_image_axes(t)]
        assert all((t['face'][0] and not t['face'][1] and not t['face'][2]) if t['group'].startswith('face') else
                   tuple(t['eps_axes']) == (0,) for t in dropped)
        signs = {s for _, _, t in cases for s in bc.eps_signs(t)}
        assert {1, -1} <= signs, (g, signs)
        # float32 twins are float32 matrices, the others are not
        assert all(t['f32'] == (g == 'f32twin') for _, _, t in cases)


def test_tiles_are_the_ones_the_issue_names():
    assert bc.tile_of('linear', bc.OUTS[0]) == (8, 8, 16) and bc.tile_of('linear', bc.OUTS[1]) == (8, 16, 16)
    assert bc.tile_of('cubic', bc.OUTS[0]) == (8, 8, 16) and bc.tile_of('cubic', bc.OUTS[1]) == (8, 8, 16)


@pytest.mark.parametrize('out', bc.OUTS, ids=OUT_IDS)
def test_lattice_cases_put_voxels_within_eps_of_an_integer(out):
    """On every image axis that received eps: the share of voxels within 2|eps| (+ float64 rounding of the chain) of an integer is at
    least MIN_SHARE of 1 / q, q the lattice period of that row; every voxel is inside the image; eps of either sign occurs."""
    worst = {}
    for g in ('lattice', 'f32twin'):
        signs = set()
        for name, m, t in bc.kept(out, g):
            ins, y, x = bc.mask_of(m.astype(np.float32).astype(np.float64) if t['f32'] else m, out)
            assert ins.all(), name
            for r, s in ((1, y), (2, x)):
                if r not in t['eps_axes']:
                    continue
                eps = abs(m[r, 3] - np.round(m[r, 3])) if t['f32'] else abs(t['eps'][r])
                share = float((np.abs(s - np.round(s)) <= 2.0 * eps + ROUNDING).mean())
                assert share >= MIN_SHARE * t['share'][r], (name, r, share, t['share'][r])
                worst[(g, t['share'][r])] = min(worst.get((g, t['share'][r]), 1.0), share)
                if t['eps'][r]:
                    signs.add(int(np.sign(t['eps'][r])))
        assert signs == {1, -1}, (g, signs)
    print('lowest share per (group, predicted): ' + ', '.join(f'{k[0]} {k[1]:.3f} -> {v:.3f}' for k, v in sorted(worst.items())))


@pytest.mark.parametrize('out', bc.OUTS, ids=OUT_IDS)
def test_face_exact_cases_hold_whole_lines_exactly_on_a_face(out):
    """Dyadic matrices: the chain is exact, so y == face + eps holds with ==.  A full row or column of output voxels sits there; with
    eps = 0 that is y + 0.5 == 0 (inside) or y + 0.5 == H (outside), likewise x."""
    lines = {}
    for name, m, t in bc.kept(out, 'face_exact'):
        assert t['exact'], name
        _, y, x = bc.mask_of(m, out)
        for r, s in ((1, y), (2, x)):
            f = t['face'][r]
            if not f:
                continue
            face = -0.5 if f[0] == 'lo' else DIM[r] - 0.5
            on = s == face + t['eps'][r]
            assert any(bool(on.all(axis=a).any()) for a in range(3)), (name, r, f, int(on.sum()))
            if t['eps'][r] == 0.0:
                assert np.array_equal(on, (s + 0.5 == 0.0) if f[0] == 'lo' else (s + 0.5 == DIM[r]))
                lines[(r, f[0])] = lines.get((r, f[0]), 0) + 1
                # the rule on this axis alone (the other coordinate held inside)
                other = np.zeros_like(s)
                alone = bm.inside(s, other, H, W) if r == 1 else bm.inside(other, s, H, W)
                assert alone[on].all() if f[0] == 'lo' else not alone[on].any(), (name, r, f)
    print('face_exact cases with eps = 0 per (axis, side):', lines)
    assert all(lines.get((r, side), 0) >= MIN_FACE_LINES for r in bc.AXES for side in ('lo', 'hi')), lines


def test_inside_puts_the_equality_at_zero_inside_and_at_the_far_face_outside():
    one = np.ones(1)
    for lo, hi, n in ((-0.5, H - 0.5, 'y'), (-0.5, W - 0.5, 'x')):
        def ins(v):
            return bool(bm.inside(v * one, 5.0 * one, H, W)[0] if n == 'y' else bm.inside(5.0 * one, v * one, H, W)[0])
        assert ins(lo) and not ins(np.nextafter(lo, -1.0)) and not ins(hi) and ins(np.nextafter(hi, 0.0))


@pytest.mark.parametrize('out', bc.OUTS, ids=OUT_IDS)
def test_chain_dependent_masks_are_the_oracles(out):
    """face_chain and margin cases: 3-4-5 and thirds entries, whose products round, so the side of the cut a voxel falls on depends on the
    chain.  The model's mask must be the oracle's decision on every voxel: the oracle's trilinear sample at an integer plane of positive
    data is non-zero exactly inside (tests/test_lattice_cases.py), the tie of tests/test_backproject_host.py."""
    stack = positive_stack()
    cases = list(bc.kept(out, 'face_chain'))
    for tile in tiles_met(out):
        cases += bc.whole_margin_cases(out, tile)
    planes = bc.planes_of(len(cases))
    near = 0
    for (name, m, t), k in zip(cases, planes):
        assert not t['exact'], name
        mask, y, x = bc.mask_of(m, out)
        want = oracle.affine_ex(stack, plane_row(m, k), 'linear', out)
        assert np.array_equal(want != 0, mask), (name, int(((want != 0) != mask).sum()))
        near += int(((np.abs(y + 0.5) < 1e-9) | (np.abs(y + 0.5 - H) < 1e-9) | (np.abs(x + 0.5) < 1e-9) | (np.abs(x + 0.5 - W) < 1e-9)).sum())
    print(f'{len(cases)} chain-dependent cases, {near} voxels within 1e-9 of a face')
    assert near >= 500


@pytest.mark.parametrize('out', bc.OUTS, ids=OUT_IDS)
def test_margin_cases_fool_a_bare_comparison(out):
    """The 3-D generator (box_index_model.whole_margin_cases) yields none on a stack of three planes; the 2-D one does, per tile."""
    for tile in tiles_met(out):
        assert not bi.whole_margin_cases(bc.STACK, out, bi.TILES.index(tile))
        cases = bc.whole_margin_cases(out, tile)
        print(out, tile, len(cases), 'margin cases,', sum(t['fooled'] for _, _, t in cases), 'voxels')
        assert len(cases) >= MIN_MARGIN, (tile, len(cases))
        # both image axes; the sides are whatever the rounding of base + reach against the chain gives (here: the low faces)
        assert {t['eps_axis'] for _, _, t in cases} == {1, 2}
        for name, m, t in cases:
            mask, y, x = bc.mask_of(m, out)
            fooled = 0
            for d0, h0, w0 in bc.tiles_whole_without_margin(m, out, tile):
                blk = mask[d0:d0 + tile[0], h0:h0 + tile[1], w0:w0 + tile[2]]
                fooled += int((~blk).sum())
                # ... and with the margin the same bounding box is not called inside
                neg, pos = bc._reach(m, tile)
                bare = margin = True
                for r in bc.AXES:
                    base = float(bm._fma(m[r, 0], d0, bm._fma(m[r, 1], h0, bm._fma(m[r, 2], w0, m[r, 3]))))
                    bare &= base + neg[r] >= -0.5 and base + pos[r] < DIM[r] - 0.5
                    margin &= base + neg[r] >= -0.5 + bi.TILE_MARGIN and base + pos[r] < DIM[r] - 0.5 - bi.TILE_MARGIN
                assert bare and (blk.all() or not margin), name
            assert fooled == t['fooled'] > 0, name


@pytest.mark.parametrize('out', bc.OUTS, ids=OUT_IDS)
def test_whole_and_cut_tiles_exist_where_the_ledger_expects_them(out):
    for tile in tiles_met(out):
        present = kinds_present(out, tile)
        print(out, tile, present)
        for g in bc.GROUPS:
            assert present[g][0] >= MIN_WHOLE[g] and present[g][1] >= MIN_CUT[g], (tile, g, present[g])
        # lattice cases lie inside the image: no tile of theirs is cut by the skirt
        assert present['lattice'][1] == 0 and present['f32twin'][1] == 0


def test_no_output_shape_selects_the_cube_tile():
    """backproject_entry_point has a (16, 16, 16) configuration.  extract_pick_tile's cost of a configuration is
    bytes x tiles / voxels x penalty.  For every shape ceil(n / 8) <= 2 ceil(n / 16), so the (8, 16, 16) tile needs at most twice the
    tiles of the cube; its box of the typical rotation is less than half the penalised bytes of the cube's, for linear and for cubic.  The
    cube is tried first and replaced by anything strictly cheaper: it is never the answer.  Checked on a sample of shapes besides."""
    typical = [[0.5, 0.5, 0.5, 0.0]] * 3
    for cubic in (False, True):
        cost = []
        for tile in bi.TILES[:2]:
            L = bi.extract_box_dims(typical, tile, 2 if cubic else 0)
            nbytes = L[0] * L[1] * L[2] * 4
            wg = min(8, bi.LDS_CAP // nbytes)
            cost.append(nbytes * (1.0 if wg >= 3 else (1.25 if wg == 2 else 2.0)))
        assert 2 * cost[1] < cost[0], (cubic, cost)
        sample = list(range(1, 70, 4)) + [16, 32, 48, 64, 128, 512]
        for shape in itertools.product(sample, repeat=3):
            assert bi.extract_pick_tile(cubic, shape)[0] != 0, (cubic, shape)


# ---- stage_patch's index arithmetic (argued here, never by a mutated run) -----------------------------------------------------------
def stage_patch_order(Ly, Lx, wrap='single'):
    """[(vector slot, y, cx)] as stage_patch walks them: thread tid starts at v = tid, (y, cx) = divmod(v, nvx), and advances by 256
    vectors per trip with y += step_y, cx += step_cx and a single wrap of cx.  `wrap`: 'single' (the kernel's), 'none', 'no_carry'
    (cx wraps, y is not advanced) -- two ways to get it wrong."""
    nvx = Lx >> 2
    total = Ly * nvx
    step_y = 256 // nvx
    step_cx = 256 - step_y * nvx
    res = []
    for tid in range(256):
        v, (y, cx) = tid, divmod(tid, nvx)
        while v < total:
            res.append((v, y, cx))
            v += 256
            cx += step_cx
            y += step_y
            if cx >= nvx and wrap != 'none':
                cx -= nvx
                y += 1 if wrap == 'single' else 0
    return sorted(res)


def test_stage_patch_single_wrap_is_exact_and_the_gpu_tests_would_see_a_wrong_one():
    """For rows of 1 .. 71, 250 .. 269 and 300 vectors (the regime step_y == 0 beyond 256 included) slot v holds
    vector (v // nvx, v % nvx): cx + step_cx < 2 nvx, so one wrap is enough.  A walk without the wrap, or one that wraps cx without
    carrying into y, misplaces vectors in every patch of more than 256 vectors whose row length does not divide 256 -- the anisotropic
    entries of tests/test_gpu_backproject_schedule.py ((3, 1064), (5, 1052): step_y == 0) and the large patches of its scale sweep."""
    for nvx in list(range(1, 72)) + list(range(250, 270)) + [299, 300]:
        for Ly in (1, 3, 5, 17, 96):
            want = [(v,) + divmod(v, nvx) for v in range(Ly * nvx)]
            assert stage_patch_order(Ly, 4 * nvx) == want, (Ly, nvx)
    for Ly, Lx in ((3, 1064), (5, 1064), (3, 1052), (5, 1052), (96, 208), (60, 132)):
        want = [(v,) + divmod(v, Lx >> 2) for v in range(Ly * (Lx >> 2))]
        assert Ly * (Lx >> 2) > 256
        for wrong in ('none', 'no_carry'):
            got = stage_patch_order(Ly, Lx, wrong)
            assert got != want, (Ly, Lx, wrong)
            assert sum(a != b for a, b in zip(got, want)) >= Ly * (Lx >> 2) // 8, (Ly, Lx, wrong)
