"""Pull matrices that put output voxels ON the integer lattice of the source, and on the skirt faces.

Every tiled kernel family replaces the per-voxel gather of the direct kernel by a box, a span table or a ring of planes that the
host sizes and a tile-level coordinate places; whether a voxel's taps land inside what was staged is decided by floor() of a
float64 coordinate, defended by hand-picked margins (1e-9 at the row kernel's box origin, 4e-9 / 2.1e-9 at the span kernel's
Q32.32 coordinates, 1e-8 at both box extents, `fz == 0.0f` / `fz == 1.0f` at the axis-0 split of the plane-quad planner).  The
matrices here put a known share of all voxels within `eps` of an integer coordinate, for `eps` on either side of each margin,
and whole planes / rows / columns of voxels exactly on the hard cut of the skirt rule (`s + 0.5 == 0`: inside; `== dim`: outside).

Plain numpy, no GPU, no pytest: `cases(shape)` yields `(name, m64, traits)`; `tests/test_lattice_cases.py` anchors the oracle on
them and asserts what makes them adversarial, `tests/test_gpu_lattice.py` runs the kernels on them.

A case is a SPEC (linear part, centre kind, integer bases, eps vector) that is independent of the volume; `cases(shape)` places
it on a shape (the centre and the face positions depend on it).  The full product of the lists below is far too large to launch:
`SPECS` is a fixed sample, drawn with `SEED` and built so that every class of linear part meets every `eps` of either sign,
every residue of the base mod 4 and every axis at least once (asserted by the tests).
"""
from fractions import Fraction
from math import gcd

import numpy as np

SEED = 20261016

P20, P40, P50 = 2.0 ** -20, 2.0 ** -40, 2.0 ** -50
# |eps|: the set straddles the margins named above.  2^-50 is an addition to the list the margins suggest: for `t = k - 2^-50` the
# planner's split gives fz = 1.0f like 2^-40, and `d + t` ROUNDS to the integer from d = 8 on (ulp(8 + k) > 2^-50), so the canonical
# coordinate of most planes is an exact integer while the tile-level offset is not.
EPS_ABS = (P50, P40, 1e-12, 1e-10, 9e-10, 1.1e-9, 3.9e-9, 4.1e-9, 9e-9, 1.1e-8, 1e-7, P20)
EPS = (0.0,) + tuple(s * e for e in EPS_ABS for s in (1.0, -1.0))
# the row kernel stages 16 or 18 vectors according to floor(t) & 3; 61 pushes a run over the far end of a 72-wide row
BASES = (0, 1, 2, 3, 4, -3, 61)
FACE_EPS = (0.0, P40, -P40, P20, -P20)

GROUPS = ('lattice', 'f32twin', 'face_exact', 'face_chain', 'face_scipy')
CLASSES = ('identity', 'perm', 'rot345', 'scale', 'shear', 'thirds')


# ---------------------------------------------------------------------------------------------------
# linear parts
# ---------------------------------------------------------------------------------------------------
def _signed_permutations():
    out = []
    for perm in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)):
        for signs in range(8):
            L = np.zeros((3, 3))
            for r in range(3):
                L[r, perm[r]] = -1.0 if (signs >> r) & 1 else 1.0
            out.append(L)
    return out


def _quarter(axis):
    """Quarter turn about an array axis."""
    i, j = [a for a in range(3) if a != axis]
    Q = np.eye(3)
    Q[i, i] = Q[j, j] = 0.0
    Q[i, j], Q[j, i] = -1.0, 1.0
    return Q


def _rot345(axis):
    """Rotation with cosine 0.6 and sine 0.8 AS FLOAT64 (not rounded to float32: their float32 forms are no lattice)."""
    i, j = [a for a in range(3) if a != axis]
    R = np.eye(3)
    R[i, i] = R[j, j] = 0.6
    R[i, j], R[j, i] = -0.8, 0.8
    return R


def linear_parts():
    """{class: [(label, 3x3 float64)]}"""
    sp = _signed_permutations()
    rots = [L for L in sp if round(np.linalg.det(L)) == 1 and not np.array_equal(L, np.eye(3))]
    assert len(rots) == 23
    mirrors = [np.diag([1.0, -1.0, 1.0]), np.array([[1.0, 0, 0], [0, 0, 1.0], [0, 1.0, 0]])]
    parts = {'identity': [('I', np.eye(3))],
             'perm': [('p%02d' % i, L) for i, L in enumerate(rots)] + [('mir%d' % i, L) for i, L in enumerate(mirrors)]}
    r345 = []
    for a in range(3):
        r345.append(('r345_ax%d' % a, _rot345(a)))
        r345.append(('r345q_ax%d' % a, _quarter(a) @ _rot345(a)))       # lands on the exchanged / transposed orientation
    parts['rot345'] = r345
    sc = []
    for s in (0.5, 2.0, 0.25):
        for a in range(3):
            d = np.ones(3); d[a] = s
            sc.append(('sc%g_ax%d' % (s, a), np.diag(d)))
        sc.append(('sc%g_all' % s, np.diag([s, s, s])))
    parts['scale'] = sc
    sh = []
    for k in (1.0, 0.5):
        for i in range(3):
            for j in range(3):
                if i != j:
                    L = np.eye(3); L[i, j] = k
                    sh.append(('sh%g_%d%d' % (k, i, j), L))
    parts['shear'] = sh
    T = np.array([[2.0, -1.0, 2.0], [2.0, 2.0, -1.0], [-1.0, 2.0, 2.0]]) / 3.0
    parts['thirds'] = [('thirds', T), ('thirdsT', T.T.copy())]
    return parts


def structure(L):
    """Which launch class the planner sees: 'axis0' (axis-0-separable: plane-quad kernel, fused projection), 'axis1' / 'axis2' (the same
    after an axis exchange; 'axis2' is also the row kernel's class), 'general'."""
    def sep(a):
        e = np.zeros(3); e[a] = 1.0
        return np.array_equal(L[a], e) and np.array_equal(L[:, a], e)
    if sep(0):
        return 'axis0'
    if sep(2):
        return 'axis2'
    if sep(1):
        return 'axis1'
    return 'general'


def _denominator(x):
    return Fraction(float(x)).limit_denominator(16).denominator


def lattice_period(row):
    """Smallest q with q * row integral: row . x runs through the residues k / q uniformly (numerators coprime to q), so a share 1 / q of
    all voxels has an integer coordinate on this axis."""
    q = 1
    for x in row:
        d = _denominator(x)
        q = q * d // gcd(q, d)
    return q


def is_dyadic(L, bits=4):
    s = np.asarray(L, np.float64) * (1 << bits)
    return bool(np.all(s == np.round(s)))


# ---------------------------------------------------------------------------------------------------
# the sample
# ---------------------------------------------------------------------------------------------------
def _build_specs():
    rs = np.random.RandomState(SEED)
    parts = linear_parts()
    specs = []
    axes_cycle = (0, 1, 2, 'all')
    for ci, cls in enumerate(CLASSES):
        members = list(parts[cls])
        order = list(rs.permutation(len(members)))
        eps_order = list(rs.permutation(len(EPS)))
        for n, ei in enumerate(eps_order):
            eps = EPS[ei]
            label, L = members[order[n % len(members)]]
            axis = axes_cycle[(n + ci) % 4]
            base = BASES[(n + 2 * ci) % len(BASES)]
            # scales and dyadic shears keep the lattice about an integer centre only (0.5 * (k + 0.5) is no integer)
            centre = 'int' if cls in ('scale', 'shear') else ('half', 'int')[(n + ci) % 2]
            if axis == 'all':
                ev = (eps, -eps, eps)
                bv = (base, BASES[(n + 1) % len(BASES)], BASES[(n + 3) % len(BASES)])
            else:
                ev = tuple(eps if a == axis else 0.0 for a in range(3))
                bv = tuple(base if a == axis else int(rs.randint(-2, 3)) for a in range(3))
            specs.append(dict(group='lattice', cls=cls, label=label, L=L, centre=centre, base=bv, eps=ev, eps_axis=axis))
    # the three forms of the axis-0 split on the plain and on both exchanged orientations (and the in-plane transposed one): offset on
    # the rotation axis k (fz == 0), k + 1e-12 (fz tiny), k - 2^-40 and k - 2^-50 (fz == 1.0f)
    for a in range(3):
        for label, L in parts['rot345'][2 * a: 2 * a + 2]:
            for e in (0.0, 1e-12, -P40, -P50):
                specs.append(dict(group='lattice', cls='rot345', label=label, L=L, centre='half', base=tuple(3 if r == a else 0 for r in range(3)),
                                  eps=tuple(e if r == a else 0.0 for r in range(3)), eps_axis=a))
    # float32 twins: dyadic linear parts, offsets one float32 ulp above / below an integer, handed over as a float32 matrix
    n = 0
    for cls in ('identity', 'perm', 'scale', 'shear'):
        members = list(parts[cls])
        for k, sign in enumerate((1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0)):
            label, L = members[int(rs.randint(len(members)))]
            axis = axes_cycle[(k // 2 + n) % 4]
            base = BASES[(k + n) % len(BASES)]
            bv = (base, BASES[(k + 2) % len(BASES)], BASES[(k + 4) % len(BASES)]) if axis == 'all' else \
                tuple(base if a == axis else 0 for a in range(3))
            if all(b == 0 for b in bv):
                bv = tuple(1 if (axis == 'all' or a == axis) else 0 for a in range(3))      # (nextafter(0) is a denormal: no twin of a margin)
            specs.append(dict(group='f32twin', cls=cls, label=label, L=L, centre='int', base=bv, eps=(sign, -sign, sign) if axis == 'all' else
                              tuple(sign if a == axis else 0.0 for a in range(3)), eps_axis=axis))
        n += 1
    # face cases: a plane / row / column of output voxels exactly on the cut.  `face`: per axis None, or (side, n): the output voxel
    # n steps from the low / high end of the axis that drives this source axis lands on the low / high face
    face_L = [('identity', 'I', np.eye(3)), ('perm', 'p_swap01', np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]])),
              ('perm', 'p_cyc', np.array([[0.0, 0, 1], [1, 0, 0], [0, 1, 0]])), ('perm', 'mir0', np.diag([1.0, -1.0, 1.0])),
              ('scale', 'sc0.5_all', np.diag([0.5, 0.5, 0.5])), ('scale', 'sc2_ax1', np.diag([1.0, 2.0, 1.0])),
              ('shear', 'sh1_12', np.array([[1.0, 0, 0], [0, 1, 1], [0, 0, 1]])), ('shear', 'sh0.5_21', np.array([[1.0, 0, 0], [0, 1, 0], [0, 0.5, 1]])),
              ('shear', 'sh1_01', np.array([[1.0, 1, 0], [0, 1, 0], [0, 0, 1]]))]
    face_L += [('rot345', lab, L) for lab, L in parts['rot345']]
    k = 0
    for cls, label, L in face_L:
        chain = cls == 'rot345'
        for axis in (0, 1, 2, 'all'):
            for side in ('lo', 'hi'):
                e = FACE_EPS[k % len(FACE_EPS)]
                k += 1
                nsteps = (0, 3, 1, 5)[k % 4]
                face = tuple((side, nsteps) if (axis == 'all' or a == axis) else None for a in range(3))
                specs.append(dict(group='face_chain' if chain else 'face_exact', cls=cls, label=label, L=L, centre='half', base=(0, 1, -1),
                                  eps=tuple(e if f else 0.0 for f in face), eps_axis=axis, face=face))
    # ... and every face eps at least once per class of linear part and side
    for cls, label, L in (face_L[0], face_L[4], face_L[6], face_L[9], face_L[13]):
        for e in FACE_EPS:
            for side in ('lo', 'hi'):
                axis = k % 3
                k += 1
                face = tuple((side, 2) if a == axis else None for a in range(3))
                specs.append(dict(group='face_chain' if cls == 'rot345' else 'face_exact', cls=cls, label=label, L=L, centre='half',
                                  base=(0, 0, 0), eps=tuple(e if f else 0.0 for f in face), eps_axis=axis, face=face))
    # faces of the edge='scipy' contract (s == 0 and s == dim - 1, both inside): chain-exact linear parts only
    for cls, label, L in face_L[:9]:
        for axis in (0, 1, 2, 'all'):
            for side in ('lo', 'hi'):
                e = FACE_EPS[k % len(FACE_EPS)]
                k += 1
                face = tuple((side, (0, 2, 4)[k % 3]) if (axis == 'all' or a == axis) else None for a in range(3))
                specs.append(dict(group='face_scipy', cls=cls, label=label, L=L, centre='int', base=(0, 0, 0),
                                  eps=tuple(e if f else 0.0 for f in face), eps_axis=axis, face=face))
    for i, s in enumerate(specs):
        s['index'] = i
        s['family'] = structure(s['L'])
    return specs


SPECS = _build_specs()


# ---------------------------------------------------------------------------------------------------
# placing a spec on a shape
# ---------------------------------------------------------------------------------------------------
def centre_of(shape, kind):
    c = np.floor(np.asarray(shape, np.float64) / 2.0)
    return c if kind == 'int' else c - 0.5          # 'half': the default centre (dim - 1) / 2 of an even-sized volume


def _base_for(b, dim):
    return (b if dim >= 72 else 5) if b == 61 else b      # 61 only where the axis is long enough to keep voxels inside (same residue mod 4)


def _driving_axis(L, r):
    return int(np.argmax(np.abs(L[r])))


def _face_offset(L, r, side, nsteps, shape, scipy, src_shape=None):
    """Offset t_r for which the output voxel `nsteps` from the low / high end of the axis driving source axis r (the other two output
    coordinates at their first voxel) has s_r exactly on the face, in exact arithmetic; float64 rounds it for the 3-4-5 parts.
    `shape` is the OUTPUT extent; the source extent is `src_shape` where it differs (box cases)."""
    src_shape = shape if src_shape is None else src_shape
    j = _driving_axis(L, r)
    x = np.zeros(3)
    x[j] = nsteps if (side == 'lo') == (L[r, j] > 0) else shape[j] - 1 - nsteps
    lo, hi = (0.0, src_shape[r] - 1.0) if scipy else (-0.5, src_shape[r] - 0.5)
    return (lo if side == 'lo' else hi) - float(L[r] @ x)


def place(spec, shape):
    """(name, m64, traits) of a spec on a volume shape."""
    L = spec['L']
    c = centre_of(shape, spec['centre'])
    t = c - L @ c
    face = spec.get('face')
    for r in range(3):
        if face and face[r]:
            t[r] = _face_offset(L, r, face[r][0], face[r][1], shape, spec['group'] == 'face_scipy') + spec['eps'][r]
        elif spec['group'] == 'f32twin':
            k = np.float32(np.round(t[r]) + _base_for(spec['base'][r], shape[r]))
            t[r] = float(np.nextafter(k, np.float32(np.inf * spec['eps'][r]))) if spec['eps'][r] else float(k)
        else:
            t[r] = t[r] + _base_for(spec['base'][r], shape[r]) + spec['eps'][r]
    m = np.eye(4)
    m[:3, :3] = L
    m[:3, 3] = t
    f32 = spec['group'] == 'f32twin'
    if f32:
        assert np.array_equal(m, m.astype(np.float32).astype(np.float64))
    eps_axes = tuple(r for r in range(3) if spec['eps'][r] != 0.0) or \
        ((0, 1, 2) if spec['eps_axis'] == 'all' else (spec['eps_axis'],))
    # chain-exact: every product and partial sum of the fma chain is representable (dyadic entries, offsets on a 2^-41 grid, coordinates
    # below 2^11), so every correct implementation must agree with the oracle on the side of every cut
    grid = m[:3, 3] * 2.0 ** 41
    exact = is_dyadic(L) and bool(np.all(grid == np.round(grid))) and max(shape) < 2048
    eps_mag = max(abs(e) for e in spec['eps'])
    if f32:
        eps_mag = float(max(abs(m[r, 3] - np.round(m[r, 3])) for r in eps_axes))
    traits = dict(index=spec['index'], group=spec['group'], cls=spec['cls'], family=spec['family'], exact=exact, f32=f32,
                  eps=spec['eps'], eps_mag=eps_mag, eps_axes=eps_axes, eps_axis=spec['eps_axis'],
                  eps_sign=int(np.sign(next((e for e in spec['eps'] if e), 0.0))),
                  share={r: 1.0 / lattice_period(L[r]) for r in eps_axes}, face=face, centre=spec['centre'],
                  base=tuple(_base_for(b, d) for b, d in zip(spec['base'], shape)))
    name = '%03d_%s_%s' % (spec['index'], spec['group'], spec['label'])
    return name, m, traits


def cases(shape, groups=None):
    """Every sampled case placed on `shape`, as (name, m64, traits); `groups` filters by group name."""
    for spec in SPECS:
        if groups is None or spec['group'] in groups:
            yield place(spec, tuple(int(s) for s in shape))


# ---------------------------------------------------------------------------------------------------
# placing a spec on a box cut out of a larger volume (the box kernels, kinds 11-16)
# ---------------------------------------------------------------------------------------------------
BOX_TAP_MARGIN = 2          # a 'whole' box keeps every tap, the cubic ones included, this many voxels inside the volume


def box_centre_of(box, kind):
    """The box centre (box - 1) / 2 of an even-sized box for 'half', its floor for 'int'.  (On an odd extent 'half' still takes
    floor + 0.5: a centre with integer and half-integer components breaks the lattice of the rotated parts.)"""
    c = np.floor((np.asarray(box, np.float64) - 1.0) / 2.0)
    return c if kind == 'int' else c + 0.5


def _box_reach(L, cb, box):
    """Per source axis the lowest and highest value of L @ (x - cb) over the box."""
    hi_x = np.asarray(box, np.float64) - 1.0
    lo = np.array([sum(min(L[r, k] * (0.0 - cb[k]), L[r, k] * (hi_x[k] - cb[k])) for k in range(3)) for r in range(3)])
    hi = np.array([sum(max(L[r, k] * (0.0 - cb[k]), L[r, k] * (hi_x[k] - cb[k])) for k in range(3)) for r in range(3)])
    return lo, hi


def place_box(spec, shape, box):
    """(name, m64, traits) of a spec on an output box cut out of a volume of `shape`.  The linear part turns about the box centre; the
    centre samples a source position that keeps the lattice (integer, or half-integer for a 'half' spec) and puts the middle of the
    box's footprint at the middle of the volume; the spec's base (its residue mod 4: what the alignment of the staged box's origin sees)
    and eps go on top.  Face axes take the offset that puts an output plane / row / column on a face of the SOURCE volume."""
    L = spec['L']
    cb = box_centre_of(box, spec['centre'])
    rlo, rhi = _box_reach(L, cb, box)
    half = 0.0 if spec['centre'] == 'int' else 0.5
    pos = np.floor((np.asarray(shape, np.float64) - 1.0) / 2.0 - (rlo + rhi) / 2.0 - 1.5) + half
    t = pos - L @ cb
    face = spec.get('face')
    base = tuple(b % 4 for b in spec['base'])
    for r in range(3):
        if face and face[r]:
            t[r] = _face_offset(L, r, face[r][0], face[r][1], box, spec['group'] == 'face_scipy', shape) + spec['eps'][r]
        elif spec['group'] == 'f32twin':
            k = np.float32(np.round(t[r]) + base[r])
            t[r] = float(np.nextafter(k, np.float32(np.inf * spec['eps'][r]))) if spec['eps'][r] else float(k)
        else:
            t[r] = t[r] + base[r] + spec['eps'][r]
    m = np.eye(4)
    m[:3, :3] = L
    m[:3, 3] = t
    f32 = spec['group'] == 'f32twin'
    if f32:
        assert np.array_equal(m, m.astype(np.float32).astype(np.float64))
    eps_axes = tuple(r for r in range(3) if spec['eps'][r] != 0.0) or \
        ((0, 1, 2) if spec['eps_axis'] == 'all' else (spec['eps_axis'],))
    grid = m[:3, 3] * 2.0 ** 41
    exact = is_dyadic(L) and bool(np.all(grid == np.round(grid))) and max(max(shape), max(box)) < 2048
    eps_mag = max(abs(e) for e in spec['eps'])
    if f32:
        eps_mag = float(max(abs(m[r, 3] - np.round(m[r, 3])) for r in eps_axes))
    # whole: every tap of every voxel (floor - 1 .. floor + 2) at least BOX_TAP_MARGIN voxels inside the volume
    zero = np.zeros(3)
    flo, fhi = _box_reach(L, zero, box)
    whole = all(t[r] + flo[r] >= BOX_TAP_MARGIN + 1.0 and t[r] + fhi[r] < shape[r] - 1.0 - BOX_TAP_MARGIN - 2.0 for r in range(3))
    traits = dict(index=spec['index'], group=spec['group'], cls=spec['cls'], family=spec['family'], exact=exact, f32=f32,
                  eps=spec['eps'], eps_mag=eps_mag, eps_axes=eps_axes, eps_axis=spec['eps_axis'],
                  eps_sign=int(np.sign(next((e for e in spec['eps'] if e), 0.0))),
                  share={r: 1.0 / lattice_period(L[r]) for r in eps_axes}, face=face, centre=spec['centre'],
                  base=base, whole=bool(whole))
    name = '%03d_%s_%s' % (spec['index'], spec['group'], spec['label'])
    return name, m, traits


def box_cases(shape, box, groups=None):
    """Every sampled case placed on an output box `box` cut out of a volume `shape`, as (name, m64, traits); `traits['whole']` says
    whether every tap lies BOX_TAP_MARGIN voxels inside the volume (lattice and f32twin cases, on boxes the volume has room for) or
    the box is cut by a face (face cases, by construction)."""
    shape = tuple(int(s) for s in shape)
    box = tuple(int(s) for s in box)
    for spec in SPECS:
        if groups is None or spec['group'] in groups:
            yield place_box(spec, shape, box)


def chain_coords(m64, out_shape):
    """float64 source coordinates by the oracle's own chain: fma(m0, d, fma(m1, h, fma(m2, w, t))).  numpy has no fma; the chain is
    evaluated in longdouble with each step rounded to float64, which is the fma result whenever the longdouble product-sum is exact
    or unambiguous (64-bit significands: the dyadic and 3-4-5 entries times indices below 2^11 are exact products)."""
    d, h, w = np.meshgrid(*[np.arange(n, dtype=np.longdouble) for n in out_shape], indexing='ij', sparse=True)
    out = []
    for r in range(3):
        m0, m1, m2, t = (np.longdouble(v) for v in m64[r])
        s = (m2 * w + t).astype(np.float64).astype(np.longdouble)
        s = (m1 * h + s).astype(np.float64).astype(np.longdouble)
        s = (m0 * d + s).astype(np.float64)
        out.append(np.broadcast_to(s, out_shape))
    return out
