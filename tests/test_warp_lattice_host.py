"""What makes the cases of tests/warp_lattice_cases.py adversarial, asserted on the model (tests/warp_model.py) without a GPU, and the
argument that the checks of tests/test_gpu_warp_lattice.py would catch a wrong kernel: the model with one of three switches thrown
(`whole` without kTileMargin, an inside test on an inexact coordinate, a box origin that ignores umin) changes the inside mask or
breaks the staging invariant ON THESE CASES.  No wrong kernel is ever run."""
import collections

import numpy as np
import pytest

import box_index_model as bm
import warp_lattice_cases as wl
import warp_model as wm
from oracle import oracle

SRC = wl.SRC
ROUNDING = 2.0 ** -46            # t = k + eps is rounded to float64 once: below 64 that moves the offset by 2^-47 at most
INTEGER_KINDS = ('kink_small', 'kink_big', 'kink_out', 'const', 'zero')


def every_case():
    for out in wl.OUTS:
        yield from wl.exact_cases(out)
        for cubic in (False, True):
            for part in wl.margin_cases(out, cubic):
                yield from part
        yield from wl.hull_cases(out)
        yield wl.single_node_case(out)
        yield wl.extent_case(out)
        yield from wl.scipy_cases(out)
    yield from wl.degenerate_cases()


def plain_displacement(grid, shape):
    """warp_model.displacement with the lerp written as a + f * (b - a): two roundings where the fma has one."""
    u = np.asarray(grid, np.float32).astype(np.float64)
    for axis in (2, 1, 0):
        g, o = u.shape[axis], shape[axis]
        c, f = wm.split(o, g)
        a, b = np.take(u, c, axis=axis), np.take(u, c + 1 if g > 1 else c, axis=axis)
        f = f.reshape([-1 if k == axis else 1 for k in range(4)])
        u = a + f * (b - a)
    return u


def exact_and_special():
    for out in wl.OUTS:
        yield from wl.exact_cases(out)
        yield from wl.hull_cases(out)
        yield wl.single_node_case(out)
        yield wl.extent_case(out)
        yield from wl.scipy_cases(out)


def test_both_summands_are_exact():
    n = 0
    for c in exact_and_special():
        assert c.grid.dtype == np.float32 and np.array_equal(c.grid, c.grid.astype(np.float64).astype(np.float32)), c.name
        for g, o in zip(c.grid.shape[:3], c.out_shape):
            assert g == 1 or wl.is_pow2(wm.ratio(g, o)), (c.name, g, o)
        u = wm.displacement(c.grid, c.out_shape)
        assert np.array_equal(u, plain_displacement(c.grid, c.out_shape)), c.name            # no rounding in any lerp: bit for bit
        assert wl.chain_ambiguous(c.m, c.out_shape) == 0, c.name
        assert np.array_equal(c.m, wl.matrix_of(c).astype(np.float64)), c.name                 # the float32 twins travel unchanged
        if c.kind in INTEGER_KINDS + ('hull',):
            assert np.array_equal(u, np.round(u)), c.name
        if c.kind.startswith('kink') and min(c.grid.shape[:3]) > 2:
            assert any(np.diff(u, 2, axis=k).any() for k in range(3)), c.name                  # kinks: not an affine field
        if c.affine is not None:                                                                # s = a(combined) bit for bit
            assert np.array_equal(wl.geometry(c)[0], wm.affine_coords(c.affine, c.out_shape)), c.name
        n += 1
    assert n >= 2 * (161 + 60)


def test_every_field_kind_meets_every_group_and_either_sign():
    for out in wl.OUTS:
        seen = collections.Counter((c.traits['group'], c.kind, c.traits['eps_sign']) for c in wl.exact_cases(out))
        for group in wl.GROUPS:
            for kind in wl.FIELD_KINDS:
                if (group, kind) == ('f32twin', 'const'):
                    continue                                     # a twin's offset minus an integer is no float32: it gets the zero grid
                for sign in (1, -1):
                    assert seen[(group, kind, sign)] >= 2, (out, group, kind, sign)
        grids = {c.grid.shape[:3] for c in wl.exact_cases(out)}
        assert grids >= set(wl.GRIDS[out]) | {(1, 1, 1)}


def test_lattice_share_survives_the_placing_and_the_integer_fields():
    """Per case of the groups lattice and f32twin, the share of voxels whose coordinate lies within eps_mag (+ the rounding of t = k + eps)
    of an integer on every eps axis is at least half the product of traits['share'].  A cruder test without ROUNDING reports 0 for two
    `perm` specs (eps = 4.1e-9 next to 38 is stored as 4.10000212e-9): they have not lost the lattice, the test had.  No spec is dropped.
    The smallest share found is 0.1418 (a 0.5 scale on all three axes: 1 / 8 of the lattice, plus what an odd extent adds)."""
    worst = 1.0
    n = 0
    for out in wl.OUTS:
        for c in wl.exact_cases(out):
            t = c.traits
            if t['group'] == 'face_exact':
                continue
            want = float(np.prod([t['share'][r] for r in t['eps_axes']]))
            s = wl.geometry(c)[0]
            coords = [wm.affine_coords(c.m, out)] + ([s] if c.kind in INTEGER_KINDS else [])
            for x in coords:
                near = np.ones(out, bool)
                for r in t['eps_axes']:
                    near &= np.abs(x[r] - np.round(x[r])) <= t['eps_mag'] + ROUNDING
                share = float(near.mean())
                assert share >= 0.5 * want, (c.name, share, want)
                worst = min(worst, share)
            n += 1
    print('lattice and f32twin cases', n, 'smallest share', worst)
    assert n >= 200 and worst >= 0.14


def test_face_cases_put_voxels_on_the_cut():
    """With the zero grid or the constant field every face_exact case has a full line of voxels whose s_r is the face (-0.5: inside;
    dim - 0.5: outside) plus the spec's eps EXACTLY.  A kinked field moves the face plane by whole voxels, cell by cell: what stays on
    the cut is where u_r = 0 -- a full line in some cases, single voxels in most, none in a few (counted below, three quarters of the
    kinked cases at least keep some); the rest of such a plane lies on half-integers, where floor and the split are as sharp."""
    lines = collections.Counter()
    for out in wl.OUTS:
        for c in wl.exact_cases(out):
            t = c.traits
            if t['group'] != 'face_exact' or c.kind == 'dyadic':
                continue
            s = wl.geometry(c)[0]
            on_cut = np.zeros(out, bool)
            for r in range(3):
                if t['face'][r]:
                    face = -0.5 if t['face'][r][0] == 'lo' else SRC[r] - 0.5
                    on_cut |= s[r] == face + t['eps'][r]
            full = any(on_cut.all(axis=k).any() for k in range(3))
            lines[(c.kind, 'line' if full else ('voxels' if on_cut.any() else 'none'))] += 1
            if c.kind in ('zero', 'const'):
                assert full, c.name
    print(sorted(lines.items()))
    kinked = sum(v for (k, _), v in lines.items() if k.startswith('kink'))
    assert sum(v for (k, what), v in lines.items() if what == 'line') >= 60
    assert sum(v for (k, what), v in lines.items() if k.startswith('kink') and what != 'none') >= 0.75 * kinked


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_staging_invariant_and_what_the_kernel_samples(interp):
    """In every staged tile every tap lies in the tile's box; the voxels the planned kernel samples ('zero' tiles none, whole tiles all,
    the rest by the skirt rule) are the definition's inside mask on every case of the file; the file holds staged, gathering and empty
    tiles on every tile of the class."""
    seen = collections.Counter()
    inside_share = []
    for c in every_case():
        p, what = wl.plan_of(c, interp)
        s, ins = wl.geometry(c)
        assert wm.violations(p, s, c.out_shape, interp) == [], c.name
        assert p.lds_bytes <= 160 * 1024, c.name
        assert np.array_equal(wm.kernel_inside(p, c.m, s, SRC, c.out_shape), ins), c.name
        for w in what.ravel():
            seen[(p.tile, w)] += 1
        if c.out_shape in wl.OUTS and c.traits['group'] in wl.GROUPS:
            inside_share.append(float(ins.mean()))
    print(interp, sorted(seen.items()), 'median inside', float(np.median(inside_share)))
    for tile in (((8, 16, 16), (8, 8, 16)) if interp == 'linear' else ((8, 8, 16),)):
        for w in ('stage', 'direct', 'zero'):
            assert seen[(tile, w)] >= 100, (tile, w)
    assert np.median(inside_share) >= 0.7


def test_margin_and_hull_counts():
    counts = {}
    for out in wl.OUTS:
        for cubic in (False, True):
            interp = 'bspline' if cubic else 'linear'
            zero, const = wl.margin_cases(out, cubic)
            tile = bm.TILES[bm.extract_pick_tile(cubic, out)[0]]
            counts[(out, tile)] = (len(zero), len(const))
            assert len(zero) >= 8, (out, tile)
            for c in zero + const:
                assert wl.fooled(c, interp) > 0 and wl.chain_ambiguous(c.m, out) == 0, c.name
            for c in zero:        # the model's mask is the C oracle's (true fma) on the not chain-exact parts: zeros of a positive volume
                want = oracle.affine_ex(wl.source_volume(), c.m, 'linear', out)
                assert np.array_equal(want != 0, wl.geometry(c)[1]), c.name
    print('margin cases (zero grid, constant field) per (output, tile):', counts)
    assert counts[((17, 25, 33), (8, 16, 16))][0] == 16 and counts[((17, 25, 33), (8, 8, 16))][0] == 12
    for out in wl.OUTS:
        hull = wl.hull_cases(out)
        assert len(hull) >= 40
        assert {(c.traits['group'], c.traits['eps_sign']) for c in hull} >= {(g, s) for g in ('lattice', 'face_exact') for s in (1, 0, -1)}
        for c in hull:
            for interp in ('linear', 'bspline'):
                p, what = wl.plan_of(c, interp)
                U = float(max(np.abs(p.umin).max(), np.abs(p.umax).max()))
                assert p.gm1_max >= 8 and float(np.abs(p.umin).min()) * p.gm1_max > wm.HULL_LIMIT < U * p.gm1_max, c.name
                assert (what == 'direct').all() and not p.staged.any() and p.lds_dims == (0, 0, 0), c.name
            assert wl.geometry(c)[1].mean() > 0.5, c.name
        for interp in ('linear', 'bspline'):
            what = wl.plan_of(wl.single_node_case(out), interp)[1]
            assert (what == 'direct').any() and (what == 'stage').any(), (out, interp)
        p, what = wl.plan_of(wl.extent_case(out), 'linear')
        assert not p.staged.any() and (what == 'direct').any() and wl.geometry(wl.extent_case(out))[1].any()
        assert 600.0 * (p.tile[0] - 1) >= 4096.0
    for c in wl.degenerate_cases():
        s, ins = wl.geometry(c)
        assert ins.all() and wm.skirt_distance(s, SRC).min() > 1.0, c.name          # nothing near a face: nothing to leave out
        assert np.abs(s - np.round(s)).min() > 0.1, c.name                           # ... nor near the lattice


# ---- the checks would catch a wrong kernel ----------------------------------------------------------------------------------
def test_mutation_whole_without_the_tile_margin_changes_the_mask_on_the_margin_cases():
    n = 0
    for out in wl.OUTS:
        for cubic in (False, True):
            interp = 'bspline' if cubic else 'linear'
            for c in sum(wl.margin_cases(out, cubic), []):
                p, _ = wl.plan_of(c, interp)
                s, ins = wl.geometry(c)
                wrong = wm.kernel_inside(p, c.m, s, SRC, out, margin=0.0)
                assert (wrong != ins).sum() == wl.fooled(c, interp) > 0 and not (ins & ~wrong).any(), c.name     # outside voxels come out sampled
                n += 1
    assert n >= 80


def test_mutation_inexact_coordinate_changes_the_mask_on_the_face_cases():
    """A kernel that tested float32(a) + u: a face row at -0.5 - 2^-40 (outside) or at dim - 0.5 - 2^-40 (inside) rounds onto the face and
    changes sides.  More than a quarter of the face cases show it (those with such an eps whose row an integer field leaves on the cut)."""
    changed = total = 0
    for out in wl.OUTS:
        for c in wl.exact_cases(out):
            if c.traits['group'] != 'face_exact':
                continue
            p, _ = wl.plan_of(c, 'linear')
            s, ins = wl.geometry(c)
            s32 = wm.affine_coords(c.m, out).astype(np.float32).astype(np.float64) + np.moveaxis(wm.displacement(c.grid, out), 3, 0)
            wrong = wm.kernel_inside(p, c.m, s, SRC, out, s_test=s32)
            total += 1
            changed += bool((wrong != ins).any())
    print('face cases whose mask changes under a float32 affine part:', changed, 'of', total)
    assert changed >= total // 4


def test_mutation_origin_without_umin_breaks_the_staging_invariant():
    broken = total = 0
    for out in wl.OUTS:
        for c in wl.exact_cases(out):
            if not c.kind.startswith('kink'):
                continue
            for interp in ('linear', 'bspline'):
                p = wm.plan(c.m, c.grid, out, interp, origin_without_umin=True)
                if not (p.staged & (np.abs(p.umin).max(axis=-1) >= 2)).any():
                    continue
                total += 1
                broken += bool(wm.violations(p, wl.geometry(c)[0], out, interp))
    print('kinked cases with a staged tile of |umin| >= 2 whose taps leave the box:', broken, 'of', total)
    assert total >= 100 and broken >= 0.9 * total
