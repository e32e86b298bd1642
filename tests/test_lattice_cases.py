"""The lattice / skirt-face cases of tests/lattice_cases.py, checked on the CPU (runs under -m "not gpu").

The oracle is what tests/test_gpu_lattice.py compares the kernels with, so it is anchored first: an independent reference -- numpy,
longdouble coordinates by plain multiplies and adds, float64 weights and sums, the cubic B-spline from its closed form -- against
`oracle.affine_ex` on every generated case.  Then the properties that make the cases adversarial are asserted, so that a later edit
of the generator cannot defuse them: the sample's coverage, the share of voxels within 2|eps| of an integer, the planes / rows / columns
that sit on a skirt face.
"""
import numpy as np
import pytest

import lattice_cases as lc
from oracle import oracle
from test_gpu_parity import TOL

SHAPE = (32, 50, 60)          # even: the 'half' centre is the default centre; every axis holds several periods of every lattice (2 .. 5)
FACE_BAND = 1e-9              # "away from the faces"
ROUNDING = 2.5e-13            # float64 rounding of a chain whose terms stay below 2^7: what "an integer" means for the 3-4-5 and thirds parts


def _vol(shape, seed=3):
    return np.random.RandomState(seed).random_sample(shape).astype(np.float32)


def ld_coords(m64, out_shape):
    d, h, w = np.meshgrid(*[np.arange(n, dtype=np.longdouble) for n in out_shape], indexing='ij')
    return [np.longdouble(m64[r, 0]) * d + np.longdouble(m64[r, 1]) * h + np.longdouble(m64[r, 2]) * w + np.longdouble(m64[r, 3])
            for r in range(3)]


def reference(srcs, m64, cubic):
    """([values float64 per source], inside mask, distance of every voxel to the nearest skirt face) -- texture contract, whole volume.
    The taps are gathered from zero-padded copies, for the inside voxels only."""
    shape = srcs[0].shape
    s = ld_coords(m64, shape)
    half = np.longdouble(0.5)
    inside = np.ones(shape, bool)
    dist = np.full(shape, np.inf)
    for r in range(3):
        inside &= (s[r] + half >= 0) & (s[r] + half < shape[r])
        dist = np.minimum(dist, np.minimum(np.abs(s[r] + half), np.abs(s[r] + half - shape[r])).astype(np.float64))
    s = [x[inside] for x in s]
    fl = [np.floor(x) for x in s]
    fr = [(x - f).astype(np.float64) for x, f in zip(s, fl)]
    pad = 2                                                       # taps reach floor - 1 .. floor + 2 with floor in [-1, dim - 1]
    Hp, Wp = shape[1] + 2 * pad, shape[2] + 2 * pad
    base = ((fl[0].astype(np.int64) + pad) * Hp + fl[1].astype(np.int64) + pad) * Wp + fl[2].astype(np.int64) + pad
    if not cubic:
        wts = [[1.0 - f, f] for f in fr]
        offs = (0, 1)
    else:
        wts = [[(1 - f) ** 3 / 6.0, (4 - 6 * f ** 2 + 3 * f ** 3) / 6.0, (1 + 3 * f + 3 * f ** 2 - 3 * f ** 3) / 6.0, f ** 3 / 6.0] for f in fr]
        offs = (-1, 0, 1, 2)
    padded = [np.pad(src.astype(np.float64), pad).ravel() for src in srcs]
    vals = [np.zeros(base.shape) for _ in srcs]
    for a, oz in enumerate(offs):
        for b, oy in enumerate(offs):
            wzy = wts[0][a] * wts[1][b]
            for c, ox in enumerate(offs):
                w = wzy * wts[2][c]
                at = base + ((oz * Hp + oy) * Wp + ox)
                for v, p in zip(vals, padded):
                    v += w * p[at]
    out = []
    for v in vals:
        full = np.zeros(shape)
        full[inside] = v
        out.append(full)
    return out, inside, dist


ALL = list(lc.cases(SHAPE))
TEXTURE = [c for c in ALL if c[2]['group'] != 'face_scipy']


def test_sample_covers_every_class_eps_sign_residue_and_axis():
    """Every class of linear part meets every eps of either sign, every residue of the base mod 4 and every axis (and all three at once)."""
    lat = [t for _, _, t in ALL if t['group'] == 'lattice']
    for cls in lc.CLASSES:
        mine = [t for t in lat if t['cls'] == cls]
        seen_eps = {e for t in mine for e in t['eps'] if e} | ({0.0} if any(not any(t['eps']) for t in mine) else set())
        assert seen_eps >= set(lc.EPS), (cls, sorted(set(lc.EPS) - seen_eps))
        assert {t['base'][a] % 4 for t in mine for a in t['eps_axes']} == {0, 1, 2, 3}, cls
        assert {t['eps_axis'] for t in mine} == {0, 1, 2, 'all'}, cls
    assert {t['family'] for t in lat} == {'axis0', 'axis1', 'axis2', 'general'}
    for g in lc.GROUPS:
        assert sum(t['group'] == g for _, _, t in ALL) >= 8, g
    twins = [t for _, _, t in ALL if t['group'] == 'f32twin']
    assert {t['eps_sign'] for t in twins} == {1, -1} and {t['cls'] for t in twins} == {'identity', 'perm', 'scale', 'shear'}
    for g in ('face_exact', 'face_chain', 'face_scipy'):
        faces = [t for _, _, t in ALL if t['group'] == g]
        assert {e for t in faces for e in t['eps']} >= set(lc.FACE_EPS), g
        assert {t['eps_axis'] for t in faces} == {0, 1, 2, 'all'}, g
        assert {f[0] for t in faces for f in t['face'] if f} == {'lo', 'hi'}, g
    assert all(t['exact'] for _, _, t in ALL if t['group'] in ('face_exact', 'face_scipy'))
    assert not any(t['exact'] for _, _, t in ALL if t['group'] == 'face_chain')
    assert len({n for n, _, _ in ALL}) == len(ALL)
    print(f'\n{len(ALL)} cases: ' + ', '.join(f'{g} {sum(t["group"] == g for _, _, t in ALL)}' for g in lc.GROUPS))


def test_cases_are_adversarial():
    """Share of voxels within 2|eps| of an integer on every axis that received eps: at least nine tenths of what the lattice predicts (1
    for permutations and integer shears, 1/2 for a scale of 0.5, 1/5 on the rotated axes of a 3-4-5 rotation, 1/3 for the thirds)."""
    worst = {}
    for name, m, t in ALL:
        if t['group'] not in ('lattice', 'f32twin'):
            continue
        s = lc.chain_coords(m, SHAPE)
        for r in t['eps_axes']:
            if t['f32']:
                window = 2.0 * abs(m[r, 3] - np.round(m[r, 3])) + ROUNDING
            else:
                window = 2.0 * abs(t['eps'][r]) + ROUNDING
            near = np.abs(s[r] - np.round(s[r])) <= window
            share = float(near.mean())
            assert share >= 0.9 * t['share'][r], (name, r, share, t['share'][r])
            key = (t['cls'], t['share'][r])
            worst[key] = min(worst.get(key, 1.0), share)
    print('\nmeasured share of near-integer voxels (class, predicted): ' + ', '.join(f'{k[0]} {k[1]:.3f} -> {v:.3f}' for k, v in sorted(worst.items())))


def test_face_cases_hold_a_full_line_of_voxels_on_a_face():
    """Every face case has at least one full plane, row or column of output voxels within 1e-9 of where it aims: a face of its contract,
    or the case's eps beside it (for the sheared and rotated parts the face voxels form lattice lines in a plane: a column along the
    third axis)."""
    for name, m, t in ALL:
        if not t['group'].startswith('face'):
            continue
        s = lc.chain_coords(m, SHAPE)
        for r, f in enumerate(t['face']):
            if not f:
                continue
            lo, hi = (0.0, SHAPE[r] - 1.0) if t['group'] == 'face_scipy' else (-0.5, SHAPE[r] - 0.5)
            # (the 2^-20 / 2^-40 variants sit that far from the face, on the side their sign says)
            on = np.abs(s[r] - (lo if f[0] == 'lo' else hi) - t['eps'][r]) <= FACE_BAND
            full_line = any(bool(on.all(axis=a).any()) for a in range(3))
            assert full_line, (name, r, f, int(on.sum()))
            if t['eps'][r] == 0.0 and t['exact']:
                assert np.any(s[r] == (lo if f[0] == 'lo' else hi)), name


# ---- the same properties on box cases: an output box cut out of a larger volume (tests/test_gpu_box_lattice.py) ---------------------
BOX_SOURCE = (96, 100, 104)
BOXES = ((10, 18, 18), (10, 26, 18))          # the boxes of the GPU test (tests/test_box_index_model.py: which tile each selects)
BOX_ALL = {box: list(lc.box_cases(BOX_SOURCE, box)) for box in BOXES}


def _inside(m, box, src_shape, scipy=False):
    s = lc.chain_coords(m, box)
    ins = np.ones(box, bool)
    for r in range(3):
        lo, hi = (0.0, src_shape[r] - 1.0) if scipy else (-0.5, src_shape[r] - 0.5)
        ins &= (s[r] >= lo) & ((s[r] <= hi) if scipy else (s[r] < hi))
    return ins, s


@pytest.mark.parametrize('box', BOXES, ids=lambda b: 'x'.join(map(str, b)))
def test_box_cases_cover_every_class_eps_sign_and_axis(box):
    """Placing a spec on a box keeps what the sample promises: every class of linear part meets every eps of either sign and every axis;
    names are unique; everything but `whole` and the base (its residue mod 4) is what place() gives."""
    cases = BOX_ALL[box]
    lat = [t for _, _, t in cases if t['group'] == 'lattice']
    for cls in lc.CLASSES:
        mine = [t for t in lat if t['cls'] == cls]
        seen_eps = {e for t in mine for e in t['eps'] if e} | ({0.0} if any(not any(t['eps']) for t in mine) else set())
        assert seen_eps >= set(lc.EPS), (cls, sorted(set(lc.EPS) - seen_eps))
        assert {t['base'][a] % 4 for t in mine for a in t['eps_axes']} == {0, 1, 2, 3}, cls
        assert {t['eps_axis'] for t in mine} == {0, 1, 2, 'all'}, cls
    assert len({n for n, _, _ in cases}) == len(cases) == len(ALL)
    for (n0, _, t0), (n1, _, t1) in zip(ALL, cases):
        assert n0 == n1
        for key in ('index', 'group', 'cls', 'family', 'f32', 'eps', 'eps_axes', 'eps_axis', 'eps_sign', 'share', 'face', 'centre'):
            assert t0[key] == t1[key], (n0, key)
        assert all((a - b) % 4 == 0 for a, b in zip(t0['base'], t1['base'])), n0
    assert all(t['exact'] for _, _, t in cases if t['group'] in ('face_exact', 'face_scipy'))
    assert not any(t['exact'] for _, _, t in cases if t['group'] == 'face_chain')


@pytest.mark.parametrize('box', BOXES, ids=lambda b: 'x'.join(map(str, b)))
def test_box_cases_are_adversarial_and_whole_where_they_say(box):
    """Share of box voxels within 2|eps| of an integer on every axis that received eps (as test_cases_are_adversarial; a box axis of n
    voxels holds at least floor(n / q) of every q-th lattice plane, so the share is at least (1 - q / n) / q for the shortest axis n = 10
    and the longest period q = 5: half of what the lattice predicts, asserted as such); lattice and float32-twin boxes lie, cubic taps
    included, at least two voxels inside the volume, and `whole` says so for every case."""
    n_whole = 0
    for name, m, t in BOX_ALL[box]:
        ins, s = _inside(m, box, BOX_SOURCE)
        whole = all(s[r].min() >= lc.BOX_TAP_MARGIN + 1.0 and s[r].max() < BOX_SOURCE[r] - 1.0 - lc.BOX_TAP_MARGIN - 2.0 for r in range(3))
        assert whole == t['whole'], (name, [(float(s[r].min()), float(s[r].max())) for r in range(3)])
        n_whole += whole
        if t['group'] in ('lattice', 'f32twin'):
            assert whole and ins.all(), name
            for r in t['eps_axes']:
                window = 2.0 * (abs(m[r, 3] - np.round(m[r, 3])) if t['f32'] else abs(t['eps'][r])) + ROUNDING
                share = float((np.abs(s[r] - np.round(s[r])) <= window).mean())
                assert share >= 0.5 * t['share'][r], (name, r, share, t['share'][r])
        elif t['group'] != 'face_scipy':
            assert not whole, name                     # cut by construction
    assert n_whole >= 200


@pytest.mark.parametrize('box', BOXES, ids=lambda b: 'x'.join(map(str, b)))
def test_box_face_cases_hold_a_full_line_of_voxels_on_a_face(box):
    """As test_face_cases_hold_a_full_line_of_voxels_on_a_face, with the face of the SOURCE volume and the extent of the box."""
    for name, m, t in BOX_ALL[box]:
        if not t['group'].startswith('face'):
            continue
        s = lc.chain_coords(m, box)
        for r, f in enumerate(t['face']):
            if not f:
                continue
            lo, hi = (0.0, BOX_SOURCE[r] - 1.0) if t['group'] == 'face_scipy' else (-0.5, BOX_SOURCE[r] - 0.5)
            on = np.abs(s[r] - (lo if f[0] == 'lo' else hi) - t['eps'][r]) <= FACE_BAND
            assert any(bool(on.all(axis=a).any()) for a in range(3)), (name, r, f, int(on.sum()))
            if t['eps'][r] == 0.0 and t['exact']:
                assert np.any(s[r] == (lo if f[0] == 'lo' else hi)), name


def test_oracle_is_nonzero_exactly_inside_on_positive_data():
    """Source data in [1, 2): under trilinear and unfiltered cubic B-spline weights (non-negative, the nearest tap at least 1/8 per axis)
    an inside voxel is strictly positive, so the oracle's zeros ARE its inside mask -- which a box result otherwise hides.  Asserted
    for the oracle alone against the chain_coords inside set, on every texture-contract box case."""
    vol = np.minimum(_vol(BOX_SOURCE, 5) + np.float32(1.0), np.nextafter(np.float32(2.0), np.float32(0.0))).astype(np.float32)
    assert vol.min() >= 1.0 and vol.max() < 2.0
    box = BOXES[0]
    n_cut = 0
    for name, m, t in BOX_ALL[box]:
        if t['group'] == 'face_scipy':
            continue
        ins, _ = _inside(m, box, BOX_SOURCE)
        n_cut += int(not ins.all())
        for kind in ('linear', 'bspline', 'bspline_simple'):
            want = oracle.affine_ex(vol, m, kind, box)
            assert np.array_equal(want != 0, ins), (name, kind, int(((want != 0) != ins).sum()))
    assert n_cut >= 50


def test_oracle_matches_longdouble_reference():
    """`oracle.affine_ex` against the independent reference on every case, trilinear, cubic and cubic on prefiltered coefficients: within
    the family tolerance away from the faces; the same inside mask on chain-exact cases; on chain-dependent cases (3-4-5 and thirds
    parts, offsets off the 2^-41 grid) the voxels where the two disagree about the side of a cut are at most 0.5 % of the volume -- more
    would mean the generator, not rounding, is at fault -- and every one of them sits on a face."""
    vol = _vol(SHAPE)
    coef = oracle.prefilter(vol)
    runs = (('linear', 'linear', [vol]), ('bspline', 'bspline', [vol, coef]))
    init = np.full(SHAPE, 7.0, np.float32)
    worst_err = {'linear': 0.0, 'bspline': 0.0, 'filt_bspline': 0.0}
    worst_flip, n_exact = 0.0, 0
    for name, m, t in TEXTURE:
        keep = init.copy()
        rc = oracle.lib().vt_oracle_affine_ex(vol, *SHAPE, 0, SHAPE[0], keep, *SHAPE, 0, np.ascontiguousarray(m.reshape(16)), oracle.INTERP['linear'],
                                              oracle.KEEP_OUTSIDE)
        assert rc == 0
        inside_o = keep != 7.0
        n_exact += int(t['exact'])
        for kind, _, srcs in runs:
            wants, inside_r, dist = reference(srcs, m, kind != 'linear')
            flips = inside_o != inside_r
            if t['exact']:
                assert not flips.any(), (name, int(flips.sum()))
            else:
                worst_flip = max(worst_flip, float(flips.mean()))
                assert flips.mean() <= 0.005, (name, float(flips.mean()))
                assert not (flips & (dist > FACE_BAND)).any(), name
            away = (dist > FACE_BAND) & ~flips
            for src, want, interp in zip(srcs, wants, (kind, 'filt_' + kind)):
                got = oracle.affine_ex(src, m, kind, SHAPE)
                err = float(np.abs(got - want)[away].max()) if away.any() else 0.0
                worst_err[interp] = max(worst_err[interp], err)
                assert err <= TOL[interp], (name, interp, err)
    print(f'\n{len(TEXTURE)} cases ({n_exact} chain-exact): max |oracle - longdouble reference| away from the faces: ' +
          ', '.join(f'{k} {v:.3e} (tolerance {TOL[k]:.0e})' for k, v in worst_err.items()) +
          f'; largest share of voxels on the other side of a cut, chain-dependent cases: {100 * worst_flip:.3f} %')
