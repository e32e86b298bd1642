"""Lattice, face and tile-margin cases for StaticVolume.backproject (kernel 18): plain numpy, no GPU, no pytest.

`lattice_cases.box_cases` placed on a stack of T images of 100 x 104 (the box suites' planes).  Back-projection reads rows 1 and 2 of a
matrix only, so a case is kept when its lattice or face property lies on image axis 1 or 2; the others are ordinary matrices for this
kernel.  Everything that is counted here -- inside masks, tiles that are whole or cut -- comes from tests/backproject_model.py (the float64
chain, fma through longdouble), never from the library.  tests/test_backproject_cases_host.py asserts the properties and fixes the
counts; tests/test_gpu_backproject_lattice.py runs the kernel on the cases.
"""
import functools
import itertools

import numpy as np

import backproject_model as bm
import box_index_model as bi
import lattice_cases as lc

STACK = (3, 100, 104)                               # planes are assigned cyclically: entry i reads image i % 3
OUTS = ((10, 18, 18), (10, 26, 18))                 # linear: tiles (8, 8, 16) and (8, 16, 16); cubic: (8, 8, 16) both
GROUPS = ('lattice', 'f32twin', 'face_exact', 'face_chain')
AXES = (1, 2)                                       # the image axes


def icls(interp):
    return 'linear' if interp == 'linear' else 'cubic'


def tile_of(cls, out):
    """The tile extract_pick_tile's rule gives (the host model of tests/box_index_model.py; the GPU tests compare it with info())."""
    return bi.TILES[bi.extract_pick_tile(cls == 'cubic', out)[0]]


def on_image_axes(t):
    """Does the case's lattice / face property lie on image axis 1 or 2?"""
    if t['group'].startswith('face'):
        return any(t['face'][r] for r in AXES)
    return any(r in AXES for r in t['eps_axes'])


def eps_signs(t):
    """Signs of eps on the image axes (an 'all' case carries both)."""
    return sorted({int(np.sign(t['eps'][r])) for r in AXES if t['eps'][r]}) or [0]


@functools.lru_cache(maxsize=None)
def kept(out, group):
    """[(name, m64, traits)] of one group on one output shape after the axis filter."""
    return [c for c in lc.box_cases(STACK, out, (group,)) if on_image_axes(c[2])]


def planes_of(n):
    return np.arange(n, dtype=np.int64) % STACK[0]


def mask_of(m, out):
    """(inside mask, y, x) by the model."""
    y, x = bm.coords(m, out)
    return bm.inside(y, x, STACK[1], STACK[2]), y, x


def tile_kinds(mask, tile):
    """(some depth-complete tile has every voxel inside, some tile is cut by the skirt: voxels inside and voxels outside).  A tile
    that is all inside but runs over the end of the output's depth is neither: every case has those."""
    whole = cut = False
    for d0, h0, w0 in itertools.product(*[range(0, s, t) for s, t in zip(mask.shape, tile)]):
        blk = mask[d0:d0 + tile[0], h0:h0 + tile[1], w0:w0 + tile[2]]
        if blk.all() and d0 + tile[0] <= mask.shape[0]:
            whole = True
        elif blk.any() and not blk.all():
            cut = True
    return whole, cut


def selected(out, oi, ii, stride):
    """Every stride-th kept case of each group, shifted from node to node (oi: index of the output shape, ii: of the interpolation)."""
    res = []
    for g in GROUPS:
        res += [c for j, c in enumerate(kept(out, g)) if (j + ii + 2 * oi) % stride == 0]
    return res


# ---------------------------------------------------------------------------------------------------
# cases aimed at kTileMargin, in two dimensions
# ---------------------------------------------------------------------------------------------------
def _reach(m, tile):
    """(neg, pos) per image row of extract_fill_entry: the tile's reach below and above its first voxel."""
    e = bi.extract_fill_entry(np.asarray(m, np.float64)[:3], bi.TILES.index(tile), False)
    return e['neg'], e['pos']


def tiles_whole_without_margin(m, out, tile):
    """[(d0, h0, w0)]: depth-complete tiles whose float64 bounding box on rows 1 and 2 lies inside the image by a bare comparison (no
    kTileMargin): a kernel that called them whole would skip the per-voxel test there."""
    m = np.asarray(m, np.float64)
    neg, pos = _reach(m, tile)
    res = []
    for d0 in range(0, out[0] - tile[0] + 1, tile[0]):
        for h0 in range(0, out[1], tile[1]):
            for w0 in range(0, out[2], tile[2]):
                ok = True
                for r in AXES:
                    base = float(bm._fma(m[r, 0], d0, bm._fma(m[r, 1], h0, bm._fma(m[r, 2], w0, m[r, 3]))))
                    ok = ok and base + neg[r] >= -0.5 and base + pos[r] < STACK[r] - 0.5
                if ok:
                    res.append((d0, h0, w0))
    return res


@functools.lru_cache(maxsize=None)
def whole_margin_cases(out, tile):
    """As box_index_model.whole_margin_cases, on rows 1 and 2 alone (that generator tests all three axes, and no depth-8 tile lies
    inside three planes): 3-4-5 and thirds parts placed so that a corner voxel of the first tile sits on a face of the image in exact
    arithmetic.  Kept are those where a tile's float64 bounding box says "inside" by a bare comparison while the canonical chain puts
    one of its voxels outside.  traits['fooled'] counts those voxels."""
    parts = lc.linear_parts()
    cb = lc.box_centre_of(out, 'half')
    pos = np.floor((np.asarray(STACK, np.float64) - 1.0) / 2.0) + 0.5
    res = []
    for label, L in parts['rot345'] + parts['thirds']:
        for r in AXES:
            for side in ('lo', 'hi'):
                for corner in itertools.product(*[(0, min(tile[k], out[k]) - 1) for k in range(3)]):
                    t = pos - L @ cb
                    t[r] = (-0.5 if side == 'lo' else STACK[r] - 0.5) - float(L[r] @ np.asarray(corner, np.float64))
                    m = np.eye(4)
                    m[:3, :3] = L
                    m[:3, 3] = t
                    ins, _, _ = mask_of(m, out)
                    fooled = sum(int((~ins[d0:d0 + tile[0], h0:h0 + tile[1], w0:w0 + tile[2]]).sum())
                                 for d0, h0, w0 in tiles_whole_without_margin(m, out, tile))
                    if fooled:
                        face = tuple((side, 0) if a == r else None for a in range(3))
                        traits = dict(index=len(res), group='face_chain', cls='thirds' if label.startswith('thirds') else 'rot345',
                                      family=lc.structure(L), exact=False, f32=False, eps=(0.0, 0.0, 0.0), eps_mag=0.0, eps_axes=(r,),
                                      eps_axis=r, eps_sign=0, share={r: 1.0 / lc.lattice_period(L[r])}, face=face, centre='half',
                                      base=(0, 0, 0), whole=False, fooled=fooled, margin=True)
                        res.append(('margin%02d_%s_ax%d%s' % (len(res), label, r, side), m, traits))
    return res
