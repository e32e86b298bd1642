"""StaticVolume.warp (kernel 20) on the integer lattice of the source, on the skirt faces and on the edges of its own planning rule.

tests/warp_cases.py draws rotations with a translation that is not dyadic and random fields: no voxel of those ever sits on the
lattice or on a face, and the comparison leaves out what comes within 1e-9 of one.  Here both summands of s = a + u are EXACT, so the
one rounding of the sum lands every correct implementation on the same side of every cut and nothing is left out:

  * a: the chain-exact specs of tests/lattice_cases.py (groups lattice, f32twin, face_exact) placed on an output with place_box -- a
    known share of voxels within 2^-50 .. 2^-20 of an integer coordinate, planes / rows / columns exactly on the hard cut of the skirt;
  * u: float32 grids whose trilinear interpolation is exact in float64.  Every output / grid pair has r_k = (g_k - 1) / (o_k - 1) a
    power of two, so q, f and the three lerps carry a few bits.  `kink_*`: per component a sum over the axes of piecewise-linear node
    profiles with INTEGER cell slopes -- u(v) is an integer at every voxel, the field is not affine and has kinks on node planes; three
    amplitudes (small: most tiles stage; big: most leave kWarpBoxCap; out: the nodes above the middle of axis 2 are pushed 64 voxels
    down, whole tiles are classified outside).  `dyadic`: random multiples of 2^-6, exact but off the lattice.  `const`: one integer
    node with the translation reduced by it (s = a bit for bit, through a displacement).  `zero`: the grid (1, 1, 1) of zeros.

Besides: cases aimed at kTileMargin (box_index_model.whole_margin_cases with the zero grid, and reselected with the constant field),
cases beyond the hull grant U (g_max - 1) <= 2^20 (a kinked field plus +-2^18 / 2^19 per component, the translation compensating;
one with a SINGLE node of 2^18), a matrix whose tile extent is 4096 or more, outputs with axes of length 1 and 2, and the faces of the
edge='scipy' contract.

Plain numpy, no GPU, no pytest.  tests/test_warp_lattice_host.py asserts what makes the cases adversarial on the model alone,
tests/test_gpu_warp_lattice.py runs the kernel on them."""
import collections
import functools

import numpy as np

import box_index_model as bm
import lattice_cases as lc
import warp_cases as wc
import warp_model as wm

SRC = wc.SRC
OUTS = ((17, 25, 33), (9, 17, 17))          # trilinear tiles (8, 16, 16) / (8, 8, 16), cubic (8, 8, 16): every tile cut in every dimension
GRIDS = {OUTS[0]: ((3, 4, 5), (5, 7, 9), (9, 13, 17), OUTS[0], (3, 1, 5)),
         OUTS[1]: ((3, 3, 5), (5, 9, 9), OUTS[1], (3, 1, 5))}
GROUPS = ('lattice', 'f32twin', 'face_exact')
FIELD_KINDS = ('kink_small', 'kink_big', 'kink_out', 'dyadic', 'const', 'zero')
KINK_AMP = {'kink_small': 1, 'kink_big': 3, 'kink_out': 1}
CONST = (3.0, -5.0, 7.0)
PUSH = 64                                   # kink_out: a multiple of every node spacing
HULL_CONSTS = ((2.0 ** 18, -2.0 ** 19, 2.0 ** 19), (-2.0 ** 19, 2.0 ** 18, -2.0 ** 18), (2.0 ** 19, 2.0 ** 19, -2.0 ** 19))
P20 = 2.0 ** -20
DEGENERATE = (((1, 1, 1), (1, 1, 1)), ((1, 5, 7), (1, 2, 3)), ((2, 2, 2), (2, 2, 2)), ((3, 1, 40), (3, 1, 14)))

Case = collections.namedtuple('Case', 'name out_shape m f32 grid kind traits affine')
# m: float64 4 x 4 (f32: exact as float32, handed over as a float32 matrix);  affine: the combined matrix when the field is affine-exact


def matrix_of(case):
    return np.ascontiguousarray(case.m, dtype=np.float32 if case.f32 else np.float64)


@functools.lru_cache(maxsize=None)
def source_volume():
    """Values in [1, 2): under non-negative weights the zeros of a result are its inside mask."""
    from test_gpu_box_lattice import positive
    from test_gpu_extract import rand_vol
    vol = positive(rand_vol(SRC, 2026))
    vol.setflags(write=False)
    return vol


# ---------------------------------------------------------------------------------------------------
# fields
# ---------------------------------------------------------------------------------------------------
def is_pow2(x):
    return x > 0 and float(np.frexp(x)[0]) == 0.5


def spacing(g, o):
    """Node spacing in output voxels on an axis (an integer for every pair of GRIDS)."""
    return (o - 1) // (g - 1) if g > 1 else 0


def kinked(g, o, amp, seed, push=False):
    """float64 nodes (g, 3): u_c = P0_c[i] + P1_c[j] + P2_c[k] with P the running sum of integer cell slopes times the node spacing."""
    rs = np.random.RandomState(seed)
    u = np.zeros(tuple(g) + (3,))
    for c in range(3):
        for axis in range(3):
            n = g[axis]
            P = np.zeros(n)
            if n > 1:
                P[1:] = np.cumsum(rs.randint(-amp, amp + 1, n - 1) * spacing(n, o[axis]))
                if push and c == 2 and axis == 2:
                    P[(n - 1) // 2 + 1:] -= PUSH
            u[..., c] += P.reshape([-1 if k == axis else 1 for k in range(3)])
    keep = u[..., :, :, :(g[2] - 1) // 2 + 1, :] if push else u
    u -= np.round(keep.reshape(-1, 3).mean(axis=0))          # an integer: the field stays about the placed box
    return u


def dyadic(g, seed):
    return np.random.RandomState(seed).randint(-128, 129, tuple(g) + (3,)) / 64.0


def field(kind, g, o, seed):
    """float32 grid of a field kind, exact in float32."""
    if kind == 'zero':
        f = np.zeros((1, 1, 1, 3))
    elif kind == 'const':
        f = np.asarray(CONST).reshape(1, 1, 1, 3)
    elif kind == 'dyadic':
        f = dyadic(g, seed)
    else:
        f = kinked(g, o, KINK_AMP[kind], seed, push=kind == 'kink_out')
    grid = f.astype(np.float32)
    assert np.array_equal(grid.astype(np.float64), f)
    return grid


def shifted(m, by):
    """m with the translation reduced by `by` (exactly, or the caller's assert fails)."""
    t = np.array(m, np.float64)
    t[:3, 3] -= by
    return t


# ---------------------------------------------------------------------------------------------------
# exact cases
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def exact_cases(out_shape):
    """The chain-exact specs of GROUPS on `out_shape`, each with a field; kind and grid are spread by the spec's index (shifted by one
    per block of six, so that no kind is tied to the parity of the index, which is the sign of a twin's eps).  The specs of the two
    small groups (lattice, f32twin) appear twice, the second time with the kind three further on."""
    out = []
    grids = GRIDS[out_shape]
    nk = len(FIELD_KINDS)
    for spec in lc.SPECS:
        if spec['group'] not in GROUPS:
            continue
        name, m0, t = lc.place_box(spec, SRC, out_shape)
        if not t['exact']:
            continue
        i = spec['index']
        for rep in range(1 if spec['group'] == 'face_exact' else 2):
            kind = FIELD_KINDS[(i + i // nk + 3 * rep) % nk]
            g = grids[(i // nk + rep) % len(grids)]
            m, affine = m0, None
            if kind == 'const' and t['f32']:
                kind = 'zero'                        # (a float32 offset k + ulp minus 3 is no float32: the twin keeps its matrix)
            grid = field(kind, g, out_shape, 1000 + i)
            if kind == 'const':
                affine, m = m0, shifted(m0, CONST)
                assert np.array_equal(m[:3, 3] + CONST, affine[:3, 3]), name
            if kind == 'zero':
                affine = m0
            out.append(Case('%s_%s_g%s' % (name, kind, 'x'.join(map(str, grid.shape[:3]))), out_shape, m, t['f32'], grid, kind, t, affine))
    assert len({c.name for c in out}) == len(out)
    return out


# ---------------------------------------------------------------------------------------------------
# kTileMargin
# ---------------------------------------------------------------------------------------------------
def chain_ambiguous(m, out_shape):
    """Voxels at which the model's emulated fma (the longdouble product-sum rounded to float64) might differ from a true fma: a step whose
    64-bit sum is itself rounded (TwoSum's error term is not zero) AND lies exactly half way between two float64.  An exact 64-bit sum
    is rounded once, like the fma.  0 for every chain-exact matrix; the 3-4-5 and thirds parts of the margin cases are checked with it
    (tests/test_warp_lattice_host.py)."""
    LD = np.longdouble
    d, h, w = np.meshgrid(*[np.arange(n, dtype=LD) for n in out_shape], indexing='ij', sparse=True)
    bad = np.zeros(out_shape, bool)
    for r in range(3):
        s = LD(m[r][3])
        for coef, x in ((m[r][2], w), (m[r][1], h), (m[r][0], d)):
            prod = LD(coef) * x                                       # 53 bits by 11 bits: exact
            wide = prod + s
            bb = wide - prod
            err = (prod - (wide - bb)) + (s - bb)                     # TwoSum
            narrow = wide.astype(np.float64)
            tie = np.abs(wide - narrow.astype(LD)) == np.spacing(np.abs(narrow)).astype(LD) / 2
            bad |= np.broadcast_to((err != 0) & tie, out_shape)
            s = narrow.astype(LD)
    return int(bad.sum())


def fooled(case, interp):
    """Voxels the model puts OUTSIDE in tiles that a bare comparison (no kTileMargin) of the plan's [base + neg + umin, base + pos + umax]
    calls whole: the warp analogue of box_index_model.tiles_whole_without_margin."""
    p = wm.plan(case.m, case.grid, case.out_shape, interp)
    ins = wm.inside(wm.coords(case.m, case.grid, case.out_shape), SRC)
    bare = wm.whole_tiles(p, case.m, SRC, margin=0.0)
    T = p.tile
    n = 0
    for idx in np.ndindex(*p.nT):
        if bare[idx]:
            n += int((~ins[tuple(slice(idx[k] * T[k], (idx[k] + 1) * T[k]) for k in range(3))]).sum())
    return n


@functools.lru_cache(maxsize=None)
def margin_cases(out_shape, cubic):
    """(zero-grid set, constant-field set) for the tile the planner gives (out_shape, class).  The first is whole_margin_cases as it
    stands: s = a bit for bit.  The second moves the matrices by CONST and carries CONST in the grid -- the translation rounds, so it
    is reselected with `fooled`; what survives is kept."""
    interp = 'bspline' if cubic else 'linear'
    cfg = bm.extract_pick_tile(cubic, out_shape)[0]
    zero, const = [], []
    for name, m, t in bm.whole_margin_cases(SRC, out_shape, cfg):
        zero.append(Case(name + '_zero', out_shape, m, False, field('zero', None, out_shape, 0), 'zero', t, m))
        c = Case(name + '_const', out_shape, shifted(m, CONST), False, field('const', None, out_shape, 0), 'const', t, None)
        if fooled(c, interp) and not chain_ambiguous(c.m, out_shape):
            const.append(c)
    return zero, const


# ---------------------------------------------------------------------------------------------------
# beyond the hull grant, and beyond the extent limit
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def hull_cases(out_shape):
    """Every node carries +-2^18 / 2^19 per component and the translation takes it back: U (g_max - 1) > 2^20 in every tile, all of
    them gather.  Specs with eps 0 or +-2^-20 only (a smaller eps is below the ulp at 2^19), float64 matrices; kept are those with
    more than half of the voxels inside (a spec with faces on all three axes and a field that drifts the same way leaves too few)."""
    grids = [g for g in GRIDS[out_shape] if max(g) - 1 >= 8]
    out, seen = [], set()
    for case in exact_cases(out_shape):
        t = case.traits
        if case.f32 or not all(e == 0.0 or abs(e) == P20 for e in t['eps']):
            continue
        i = t['index']
        g = grids[i % len(grids)]
        C = np.asarray(HULL_CONSTS[i % len(HULL_CONSTS)])
        m0 = lc.place_box(lc.SPECS[i], SRC, out_shape)[1]
        f = kinked(g, out_shape, 1, 3000 + i) + C
        grid = f.astype(np.float32)
        assert np.array_equal(grid.astype(np.float64), f)
        m = shifted(m0, C)
        assert np.array_equal(m[:3, 3] + C, m0[:3, 3])
        c = Case('hull_%s_g%s' % (lc.place_box(lc.SPECS[i], SRC, out_shape)[0], 'x'.join(map(str, g))), out_shape, m, False, grid, 'hull', t, None)
        if c.name not in seen and wm.inside(wm.coords(m, grid, out_shape), SRC).mean() > 0.5:
            seen.add(c.name)
            out.append(c)
    return out


@functools.lru_cache(maxsize=None)
def single_node_case(out_shape):
    """ONE node of 2^18 in a small kinked field: the tiles that see it gather, the others stage, in one launch."""
    g = [g for g in GRIDS[out_shape] if max(g) - 1 >= 8][0]
    _, m, t = lc.place_box(next(s for s in lc.SPECS if s['group'] == 'lattice' and s['cls'] == 'identity'), SRC, out_shape)
    f = kinked(g, out_shape, 1, 4000)
    f[g[0] // 2, g[1] // 2, g[2] // 2, 1] = 2.0 ** 18
    return Case('single_node_g%s' % 'x'.join(map(str, g)), out_shape, m, False, f.astype(np.float32), 'single', t, None)


@functools.lru_cache(maxsize=None)
def extent_case(out_shape):
    """Scale 600 on row 0: the tile extent is 600 (T_0 - 1) >= 4096, so nothing stages without any flag.  The plane d = o_0 / 2 lands in
    the middle of the volume."""
    g = GRIDS[out_shape][1]
    m = np.eye(4)
    m[0, 0] = 600.0
    m[:3, 3] = (SRC[0] // 2 - 600.0 * (out_shape[0] // 2), 9.0, 10.0)
    t = dict(index=0, group='extent', eps_sign=0, f32=False, exact=True)
    return Case('extent600_g%s' % 'x'.join(map(str, g)), out_shape, m, False, field('kink_small', g, out_shape, 5000), 'kink_small', t, None)


# ---------------------------------------------------------------------------------------------------
# degenerate outputs, edge='scipy'
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_cases():
    """Outputs with axes of length 1 and 2.  r_k is no power of two here (1 / 4 and 1 / 3, 1 / 3): the translation keeps every voxel a
    quarter voxel and more from the lattice of the faces instead (dyadic field, multiples of 2^-6 within +-0.125)."""
    out = []
    for i, (o, g) in enumerate(DEGENERATE):
        m = np.eye(4)
        m[:3, 3] = (np.asarray(SRC) // 2 - np.asarray(o) // 2) + 0.25
        f = np.random.RandomState(6000 + i).randint(-8, 9, tuple(g) + (3,)) / 64.0
        t = dict(index=i, group='degenerate', eps_sign=0, f32=False, exact=False)
        out.append(Case('degenerate_%s_g%s' % ('x'.join(map(str, o)), 'x'.join(map(str, g))), o, m, False, f.astype(np.float32), 'dyadic', t, None))
    return out


@functools.lru_cache(maxsize=None)
def scipy_cases(out_shape):
    """The chain-exact face_scipy specs (faces at s = 0 and s = dim - 1) with the zero grid and with the constant field."""
    out = []
    for spec in lc.SPECS:
        if spec['group'] != 'face_scipy':
            continue
        name, m, t = lc.place_box(spec, SRC, out_shape)
        if not t['exact']:
            continue
        if spec['index'] % 2:
            out.append(Case(name + '_const', out_shape, shifted(m, CONST), False, field('const', None, out_shape, 0), 'const', t, m))
            assert np.array_equal(out[-1].m[:3, 3] + CONST, m[:3, 3])
        else:
            out.append(Case(name + '_zero', out_shape, m, False, field('zero', None, out_shape, 0), 'zero', t, m))
    return out


# ---------------------------------------------------------------------------------------------------
# model results, computed once per case and sampling class
# ---------------------------------------------------------------------------------------------------
SAMPLING = {'linear': 'linear', 'bspline': 'cubic', 'bspline_simple': 'cubic', 'filt_bspline': 'filt', 'filt_bspline_simple': 'filt'}
BY_KEY = {}


@functools.lru_cache(maxsize=None)
def _sources():
    vol = source_volume().astype(np.float64)
    return {'linear': vol, 'cubic': vol, 'filt': wm.source(source_volume(), 'filt_bspline')}


@functools.lru_cache(maxsize=None)
def _geometry(key):
    c = BY_KEY[key]
    s = wm.coords(c.m, c.grid, c.out_shape)
    ins = wm.inside(s, SRC)
    s.setflags(write=False)
    ins.setflags(write=False)
    return s, ins


@functools.lru_cache(maxsize=None)
def _values(key, sampling):
    s, ins = _geometry(key)
    vals = np.where(ins, wm.sample(_sources()[sampling], s, 'linear' if sampling == 'linear' else 'bspline'), 0.0)
    vals.setflags(write=False)
    return vals


@functools.lru_cache(maxsize=None)
def _plan(key, cubic):
    c = BY_KEY[key]
    p = wm.plan(c.m, c.grid, c.out_shape, 'bspline' if cubic else 'linear')
    return p, wm.tile_outcome(p, c.m, SRC)


def key_of(case):
    key = (case.name, case.out_shape)
    BY_KEY.setdefault(key, case)
    return key


def geometry(case):
    """(coordinates (3, oD, oH, oW), inside mask)"""
    return _geometry(key_of(case))


def values(case, interp):
    """The model's float64 result."""
    return _values(key_of(case), SAMPLING[interp])


def plan_of(case, interp):
    """(plan, tile_outcome)"""
    return _plan(key_of(case), interp in wm.CUBIC)
