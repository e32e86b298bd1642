"""-m gpu: every kernel family on integer-lattice and skirt-face coordinates (tests/lattice_cases.py), against the CPU oracle.

The generic matrices of the other files (rotations by 33 / 45 / 100 degrees, translations such as 0.5 / -1.25) keep every coordinate far
from an integer and every voxel far from a skirt face.  Here a known share of all voxels sits within 2^-50 .. 2^-20 of an integer
coordinate -- on either side of the margins the tiled families defend their staged boxes with -- and whole planes, rows and columns sit
exactly on the hard cut of the inside test.  Checked per launch:
  * |got - oracle.affine_ex(src, m64)| <= TOL[interp] on EVERY voxel, face voxels included (the tolerances of tests/test_gpu_parity.py);
  * keep_outside on a random initial array: the set of untouched voxels equals the oracle's, bit for bit (the inside mask);
  * the bit identities the project promises elsewhere: row kernel (kind 10) == FORCE_DIRECT, affine_rows_db == affine_rows,
    VT_NO_PLANSHARE == shared plans, VT_SPAN_PIPE 0 == 1.
No voxel is left out of any comparison.

The full product (cases x shapes x interpolations x flag sets) is thinned pairwise: a (shape, interpolation) node takes every k-th case,
shifted from node to node, and a case takes the flag sets that reach the family it is aimed at plus two of the others in turn.  The
coverage ledger at the end of the file is what keeps that thinning honest: it counts (last_kernel, interpolation class, case group, sign of
eps) per launch and asserts that every product family served every group it can serve.  A flag set the planner declines falls back
silently, so without the ledger this file could test the direct kernel fourteen times.
"""
import collections
import ctypes

import numpy as np
import pytest

import lattice_cases as lc
import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle
from test_gpu_parity import TOL, ALL_INTERPS, LEGACY, rand_vol
from test_gpu_edge_scipy import TOL as TOL_SCIPY

pytestmark = pytest.mark.gpu

N = _native
FT = N.FORCE_TILED
# the flag sets of test_tiled_and_direct_match_oracle
PARITY_SETS = (FT | N.FORCE_XSWAP, FT | N.FORCE_XSWAP | N.NO_ZPAIR, FT | N.FORCE_XSWAP | N.NO_QUAD, FT | N.NO_QUAD | N.NO_RSWAP, FT, FT | N.NO_RSWAP,
               FT | N.NO_MARCH, FT | N.NO_ZSEP, FT | N.NO_ZSEP | N.NO_BLOCK, FT | N.NO_ZSEP | N.FORCE_PACKED, FT | N.NO_ZSEP | N.NO_PACKED, N.FORCE_DIRECT)
PACKED = FT | N.NO_ZSEP | N.FORCE_PACKED
# the sets that reach the family a case is aimed at (plane-quad kernel, directly or through an axis exchange; row kernel; general kernels)
PRIMARY = {'axis0': (FT,), 'axis1': (FT,), 'axis2': (FT, FT | N.FORCE_XSWAP), 'general': (FT,)}
SECONDARY = tuple(f for f in PARITY_SETS if f not in (FT, N.FORCE_DIRECT))
LEGACY_SETS = (FT | N.NO_QUAD, FT | N.NO_ZPAIR, FT | N.NO_MARCH)          # kinds 5 / 4, 4, 3 in the test build (tests/test_gpu_legacy.py)

SHAPES = ((70, 66, 72), (33, 47, 50), (97, 65, 200), (48, 200, 130), (8, 520, 1030))      # several tiles, chunk layers, ragged ends; coordinates beyond 1024
STRIDE = (2, 2, 4, 4, 8)                           # a node takes every STRIDE-th case of the texture-contract cases (time budget: see profiles/pr_lattice_tests.txt)
TEXTURE_GROUPS = ('lattice', 'f32twin', 'face_exact', 'face_chain')

# ---- the coverage ledger (module level: no conftest) -------------------------------------------------------------------------------
LEDGER = collections.Counter()          # (last_kernel, 'linear' | 'cubic', group, sign of eps) -> launches
QUAD_FORMS = collections.Counter()      # (orientation, form of the axis-0 split, 'linear' | 'cubic') -> kind-8 launches
WORST = {}                              # (last_kernel, interp) -> largest |got - oracle|
IDENTITIES = collections.Counter()      # bit identities compared (a form the planner declined is not compared: counted here)
NODES_RUN = set()
NODES_ALL = set()


def _icls(interp):
    return 'linear' if interp == 'linear' else 'cubic'


def _fz_form(t):
    fz = np.float32(t - np.floor(t))
    return 'zero' if fz == 0 else ('one' if fz == 1 else ('tiny' if fz < 1e-6 else 'other'))


def note(kernel, interp, traits, m64, err):
    LEDGER[(int(kernel), _icls(interp), traits['group'], traits['eps_sign'])] += 1
    key = (int(kernel), interp)
    WORST[key] = max(WORST.get(key, 0.0), float(err))
    if kernel == 8 and traits['family'] in ('axis0', 'axis1', 'axis2'):
        a = int(traits['family'][-1])
        QUAD_FORMS[(('plain', 'axis1', 'axis2')[a], _fz_form(m64[a, 3]), _icls(interp))] += 1


def node(name):
    NODES_RUN.add(name)


def selected(si, ii, groups=TEXTURE_GROUPS, stride=None):
    """The cases of node (shape si, interpolation ii): every k-th case of each group, shifted from node to node so that the nodes of a
    shape together see every case."""
    shape = SHAPES[si]
    k = stride or STRIDE[si]
    out = []
    for g in groups:
        for j, case in enumerate(lc.cases(shape, (g,))):
            if (j + 3 * ii + si) % k == 0:
                out.append(case)
    return out


def oracle_pair(src, m64, kind, out_shape, init, **window):
    """(zero-filled result, inside mask, keep_outside result) of the oracle: one run over `init` with KEEP_OUTSIDE; the voxels it left
    alone are the outside ones (init lies in [2, 3): no interpolated value of unit-range data gets there)."""
    keep = init.copy()
    m = np.ascontiguousarray(np.asarray(m64, np.float64).reshape(16))
    rc = oracle.lib().vt_oracle_affine_ex(src, *src.shape, window.get('plane0', 0), window.get('global_depth', src.shape[0]), keep, *out_shape,
                                          window.get('out_plane0', 0), m, oracle.INTERP[kind], oracle.KEEP_OUTSIDE)
    assert rc == 0
    inside = keep != init
    return np.where(inside, keep, np.float32(0)), inside, keep


def matrix_for(m64, traits):
    return np.ascontiguousarray(m64, dtype=np.float32) if traits['f32'] else np.ascontiguousarray(m64)


class Failures(list):
    def check(self, ok, *what):
        if not ok:
            self.append(what)

    def done(self):
        assert not self, f'{len(self)} failed checks, first: ' + '; '.join(repr(w) for w in self[:8])


def flag_sets_for(traits, interp, ii):
    """(flags, also with keep_outside) of one case on one node."""
    i = traits['index']
    sets = [(f, not (f & N.FORCE_XSWAP)) for f in PRIMARY[traits['family']]]
    sets += [(N.FORCE_DIRECT, True), (0, False)]
    extra = [SECONDARY[(i + ii) % len(SECONDARY)], SECONDARY[(i + ii + 5) % len(SECONDARY)]]
    if interp == 'linear':
        extra.append(PACKED)                      # the packed-span kernel: the family with the Q32.32 coordinates
    if traits['family'] == 'general':
        extra.append(FT | N.NO_ZSEP | N.NO_PACKED)
    if LEGACY and traits['family'] != 'general':
        extra.append(LEGACY_SETS[(i + ii) % 3])
    for f in extra:
        if all(f != g for g, _ in sets):
            sets.append((f, False))
    return sets


for _si in range(len(SHAPES)):
    for _interp in ALL_INTERPS:
        NODES_ALL.add(f'cases-{_si}-{_interp}')


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('si', range(len(SHAPES)), ids=['x'.join(map(str, s)) for s in SHAPES])
def test_lattice_and_face_cases_match_oracle(si, interp, monkeypatch):
    node(f'cases-{si}-{interp}')
    shape = SHAPES[si]
    ii = ALL_INTERPS.index(interp)
    vol = rand_vol(shape, 101 + si)
    filt = interp.startswith('filt')
    src = oracle.prefilter(vol) if filt else vol
    kind = interp[5:] if filt else interp
    init = (rand_vol(shape, 202 + si) + np.float32(2.0)).astype(np.float32)
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    monkeypatch.setenv('VT_ROWS', '2')            # knobs are read when a handle is created
    monkeypatch.setenv('VT_SPAN_PIPE', '1')
    sv_alt = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    monkeypatch.delenv('VT_SPAN_PIPE')
    monkeypatch.setenv('VT_ROWS_DB', '1')
    sv_db = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    monkeypatch.delenv('VT_ROWS_DB')
    monkeypatch.delenv('VT_ROWS')
    fails = Failures()
    tol = TOL[interp]
    try:
        for name, m64, t in selected(si, ii):
            m = matrix_for(m64, t)
            want, inside, want_keep = oracle_pair(src, m64, kind, shape, init)
            got_by_flags = {}
            last_tile = [None]

            def launch(handle, flags, keep, tag):
                if keep:
                    out = init.copy()
                    handle.affine(m, output=out, keep_outside=True, _flags=flags)
                else:
                    out = handle.affine(m, _flags=flags)
                info = handle.info()
                k = info.last_kernel
                last_tile[0] = tuple(info.last_tile)
                err = float(np.abs(out - (want_keep if keep else want)).max())
                note(k, interp, t, m64, err)
                fails.check(err <= tol, name, tag, flags, 'keep' if keep else 'zero', 'kernel', k, 'err', err)
                if keep:
                    untouched = out == init
                    fails.check(np.array_equal(untouched, ~inside), name, tag, flags, 'kernel', k, 'inside mask differs on',
                                int((untouched == inside).sum()), 'voxels')
                return out, k

            for flags, with_keep in flag_sets_for(t, interp, ii):
                got_by_flags[flags] = launch(sv, flags, False, 'default')
                if with_keep:
                    got_by_flags[(flags, 'keep')] = launch(sv, flags, True, 'default')
            direct, direct_keep = got_by_flags[N.FORCE_DIRECT][0], got_by_flags[(N.FORCE_DIRECT, 'keep')][0]
            tiled, k_tiled = got_by_flags[FT]
            if k_tiled == 10:                     # same chain of operations as affine_direct
                IDENTITIES['row kernel == direct'] += 1
                fails.check(np.array_equal(tiled, direct), name, 'row kernel != direct', float(np.abs(tiled - direct).max()))
                fails.check(np.array_equal(got_by_flags[(FT, 'keep')][0], direct_keep), name, 'row kernel != direct (keep_outside)')
            if t['family'] == 'axis2':
                a, ka = launch(sv_alt, FT, False, 'VT_ROWS=2')
                if ka == 10:
                    fails.check(np.array_equal(a, direct), name, 'row kernel (VT_ROWS=2) != direct', float(np.abs(a - direct).max()))
                    b, kb = launch(sv_db, FT, False, 'VT_ROWS_DB=1')
                    IDENTITIES['affine_rows_db == affine_rows'] += 1
                    fails.check(kb == 10 and np.array_equal(a, b), name, 'affine_rows_db != affine_rows', kb)
                    ak, _ = launch(sv_alt, FT, True, 'VT_ROWS=2')
                    bk, _ = launch(sv_db, FT, True, 'VT_ROWS_DB=1')
                    fails.check(np.array_equal(ak, bk) and np.array_equal(ak, direct_keep), name, 'row kernel forms differ (keep_outside)')
            if interp != 'linear' and k_tiled == 8:
                u, ku = launch(sv, FT | N.NO_PLANSHARE, False, 'VT_NO_PLANSHARE')
                IDENTITIES['VT_NO_PLANSHARE == shared'] += 1
                fails.check(ku == 8 and np.array_equal(u, tiled), name, 'VT_NO_PLANSHARE != shared plans', ku)
            if interp == 'linear':
                p0, k0 = launch(sv, PACKED, False, 'default')
                tile0 = last_tile[0]
                p1, k1 = launch(sv_alt, PACKED, False, 'VT_SPAN_PIPE=1')
                # the two forms do the same arithmetic per voxel ON THE SAME TILE: a voxel's Q32.32 coordinate is the sum of its tile's
                # base, its column's offset and its steps along the tile's depth, so another tile shape rounds it differently (2^-33 per
                # term) and a coordinate that sits on an integer changes its tap origin and its weight together, a last-bit difference
                if k0 == 6 and k1 == 6 and tile0 == last_tile[0]:
                    IDENTITIES['VT_SPAN_PIPE 0 == 1'] += 1
                    fails.check(np.array_equal(p0, p1), name, 'VT_SPAN_PIPE 0 != 1', float(np.abs(p0 - p1).max()), tile0)
    finally:
        sv.close(); sv_alt.close(); sv_db.close()
    fails.done()


PROJ_SHAPES = ((40, 44, 48), (33, 47, 50))
for _si in range(len(PROJ_SHAPES)):
    for _interp in ALL_INTERPS:
        NODES_ALL.add(f'proj-{_si}-{_interp}')


@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('pi', range(len(PROJ_SHAPES)), ids=['x'.join(map(str, s)) for s in PROJ_SHAPES])
def test_projection_on_axis0_lattice_and_face_offsets(pi, interp):
    """sum(axis=0) of the transformed volume on the axis-0-separable cases (fused kernel 7) and through the unfused path, tolerance
    TOL * depth as in test_projection_matches_oracle."""
    node(f'proj-{pi}-{interp}')
    shape = PROJ_SHAPES[pi]
    ii = ALL_INTERPS.index(interp)
    vol = rand_vol(shape, 7)
    tol = TOL[interp] * shape[0]
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    fails = Failures()
    n = 0
    try:
        for j, (name, m64, t) in enumerate(c for c in lc.cases(shape, TEXTURE_GROUPS) if c[2]['family'] == 'axis0'):
            if (j + ii + pi) % 2:
                continue
            n += 1
            m = matrix_for(m64, t)
            want = oracle.affine_ex(oracle.prefilter(vol) if interp.startswith('filt') else vol, m64,
                                    interp[5:] if interp.startswith('filt') else interp, shape).astype(np.float64).sum(axis=0)
            got = sv.projection(m)
            k = sv.info().last_kernel
            err = float(np.abs(got - want).max())
            note(k, interp, t, m64, err / shape[0])
            fails.check(k == 7 and err <= tol, name, 'fused', k, err)
            got = sv.projection(m, _flags=N.NO_ZSEP)
            err = float(np.abs(got - want).max())
            fails.check(sv.info().last_kernel != 7 and err <= tol, name, 'unfused', sv.info().last_kernel, err)
    finally:
        sv.close()
    assert n >= 20
    fails.done()


SLAB_INTERPS = ('linear', 'bspline', 'filt_bspline')
for _interp in SLAB_INTERPS:
    NODES_ALL.add(f'slab-{_interp}')


def slab_cases(G, H, W):
    """Axis-0 lattice offsets (every eps, bases within the halo) and the global high / low faces, on in-plane parts that keep (h, w) on
    their own lattice; (name, m64, traits)."""
    parts = dict(lc.linear_parts()['rot345'])
    Ls = [('I', np.eye(3), 'identity'), ('r345_ax0', parts['r345_ax0'], 'rot345'), ('r345q_ax0', parts['r345q_ax0'], 'rot345'),
          ('sh1_12', np.array([[1.0, 0, 0], [0, 1, 1], [0, 0, 1]]), 'shear')]
    c = lc.centre_of((G, H, W), 'half')
    out = []

    def add(label, L, cls, t0, eps, group):
        m = np.eye(4)
        m[:3, :3] = L
        m[:3, 3] = c - L @ c
        m[0, 3] = t0 + eps
        grid = m[:3, 3] * 2.0 ** 41
        t = dict(index=len(out), group=group, cls=cls, family='axis0', f32=False, eps=(eps, 0.0, 0.0), eps_sign=int(np.sign(eps)),
                 exact=lc.is_dyadic(L) and bool(np.all(grid == np.round(grid))))
        out.append((f'slab{len(out):02d}_{label}_t{t0:+g}{eps:+.3g}', m, t))

    for n, eps in enumerate(lc.EPS):
        label, L, cls = Ls[n % len(Ls)]
        add(label, L, cls, float((0, 1, -1)[n % 3]), eps, 'lattice')
    for n, eps in enumerate(lc.FACE_EPS * 2):
        label, L, cls = Ls[n % len(Ls)]
        # output plane G - 1 - k exactly on the high face (outside), plane k exactly on the low face (inside)
        add(label, L, cls, (0.5, 1.5)[n % 2], eps, 'face_chain' if cls == 'rot345' else 'face_exact')
        add(label, L, cls, (-0.5, -1.5)[n % 2], eps, 'face_chain' if cls == 'rot345' else 'face_exact')
    return out


@pytest.mark.parametrize('interp', SLAB_INTERPS)
def test_slab_handles_on_axis0_lattice_and_face_offsets(interp):
    """Slab handles with plane0 != 0 and out_plane0 != 0 (raw vt_volume_create_slab, float64 entry): the inside test is on the GLOBAL
    coordinate, the taps on the window's.  Each slab against the oracle on its own window."""
    from voltools_amd.distributed import plan_halo_exchange, slab_bounds, stencil_halo
    node(f'slab-{interp}')
    lib = N.load()
    counts = [30, 36, 30]
    G, H, W = sum(counts), 40, 46
    vol = rand_vol((G, H, W), 11)
    filt = interp.startswith('filt')
    src = oracle.prefilter(vol) if filt else vol
    kind = 'bspline' if filt else interp
    halo = stencil_halo(interp) + 2
    fails = Failures()
    info = N.VolumeInfo()
    for r, (g0, g1) in enumerate(slab_bounds(counts)):
        (w0, w1), _, _ = plan_halo_exchange(counts, r, halo)
        win = np.ascontiguousarray(vol[w0:w1])
        cflags = (N.SLAB_LO_INTERIOR if w0 > 0 else 0) | (N.SLAB_HI_INTERIOR if w1 < G else 0)
        h = ctypes.c_void_p()
        N.check(lib.vt_volume_create_slab(0, w1 - w0, H, W, N.INTERP_CODES[interp], win.ctypes.data, cflags, w0, G, g0, g1 - g0, ctypes.byref(h)),
                'vt_volume_create_slab')
        oshape = (g1 - g0, H, W)
        init = (rand_vol(oshape, 12) + np.float32(2.0)).astype(np.float32)
        try:
            for name, m64, t in slab_cases(G, H, W):
                want, inside, want_keep = oracle_pair(np.ascontiguousarray(src[w0:w1]), m64, kind, oshape, init, plane0=w0, global_depth=G, out_plane0=g0)
                m = np.ascontiguousarray(m64)
                for flags, keep in ((FT, False), (FT, True), (FT | N.NO_ZSEP, False), (N.FORCE_DIRECT, False), (N.FORCE_DIRECT, True), (0, False)):
                    out = init.copy()
                    N.check(lib.vt_volume_affine_f64(h, m.ctypes.data, out.ctypes.data, flags | (N.KEEP_OUTSIDE if keep else 0)), 'vt_volume_affine_f64')
                    N.check(lib.vt_volume_info(h, ctypes.byref(info)), 'vt_volume_info')
                    err = float(np.abs(out - (want_keep if keep else want)).max())
                    note(info.last_kernel, interp, t, m64, err)
                    fails.check(err <= TOL[interp], name, 'slab', r, flags, keep, 'kernel', info.last_kernel, 'err', err)
                    if keep:
                        fails.check(np.array_equal(out == init, ~inside), name, 'slab', r, flags, 'inside mask differs')
        finally:
            lib.vt_volume_destroy(h)
    fails.done()


SCIPY_SHAPES = ((33, 47, 50), (70, 66, 72))
for _si in range(len(SCIPY_SHAPES)):
    for _interp in SLAB_INTERPS:
        NODES_ALL.add(f'scipy-{_si}-{_interp}')


@pytest.mark.parametrize('interp', SLAB_INTERPS)
@pytest.mark.parametrize('si', range(len(SCIPY_SHAPES)), ids=['x'.join(map(str, s)) for s in SCIPY_SHAPES])
def test_edge_scipy_handles_on_chain_exact_lattice_and_face_cases(si, interp):
    """edge='scipy': the cut moves to s = 0 and s = dim - 1 (both inside).  Chain-exact cases only -- scipy forms its coordinates in another
    order, so on the 3-4-5 parts the side of the cut is not defined between the two -- against device='cpu' on the whole volume, at the
    tolerances of tests/test_gpu_edge_scipy.py."""
    node(f'scipy-{si}-{interp}')
    shape = SCIPY_SHAPES[si]
    ii = SLAB_INTERPS.index(interp)
    vol = rand_vol(shape, 5)
    stride = (2, 5)[si]
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    fails = Failures()
    n = 0
    try:
        for j, (name, m64, t) in enumerate(c for c in lc.cases(shape, ('lattice', 'f32twin', 'face_scipy')) if c[2]['exact']):
            if (j + ii) % stride:
                continue
            n += 1
            m = matrix_for(m64, t)
            want = vt.affine(vol, m64, interpolation=interp, device='cpu')
            for flags in (0, FT, FT | N.NO_ZSEP, N.FORCE_DIRECT):
                got = sv.affine(m, _flags=flags)
                err = float(np.abs(got - want).max())
                fails.check(err <= TOL_SCIPY[interp], name, flags, 'kernel', sv.info().last_kernel, 'err', err)
    finally:
        sv.close()
    assert n >= 15
    fails.done()


def test_axis0_separable_cases_on_the_families_of_the_test_build():
    """The axis-0-separable groups (directly, or after an axis exchange) under VT_NO_QUAD / VT_NO_ZPAIR / VT_NO_MARCH: in the test build
    (tests/test_gpu_legacy.py runs this node there) these reach round 1's kernels 5 / 4, 4 and 3; in the product build the general kernels
    serve them.  Same cases, same oracle, same tolerances."""
    shape = SHAPES[0]
    kernels = collections.Counter()
    fails = Failures()
    for interp in ('linear', 'filt_bspline'):
        vol = rand_vol(shape, 31)
        filt = interp.startswith('filt')
        src = oracle.prefilter(vol) if filt else vol
        kind = 'bspline' if filt else interp
        init = (rand_vol(shape, 32) + np.float32(2.0)).astype(np.float32)
        sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
        try:
            for j, (name, m64, t) in enumerate(c for c in lc.cases(shape, TEXTURE_GROUPS) if c[2]['family'] != 'general'):
                if j % 3:
                    continue
                m = matrix_for(m64, t)
                want, inside, want_keep = oracle_pair(src, m64, kind, shape, init)
                for flags in LEGACY_SETS:
                    out = init.copy()
                    sv.affine(m, output=out, keep_outside=True, _flags=flags)
                    k = sv.info().last_kernel
                    kernels[(k, t['group'])] += 1
                    err = float(np.abs(out - want_keep).max())
                    fails.check(err <= TOL[interp] and np.array_equal(out == init, ~inside), name, interp, flags, 'kernel', k, 'err', err)
        finally:
            sv.close()
    if LEGACY:
        for k in (3, 4, 5):
            for g in TEXTURE_GROUPS:
                assert kernels[(k, g)] > 0, (k, g, dict(kernels))
    fails.done()


def ledger_report():
    lines = ['coverage ledger: launches per (kernel, class) x (group, sign of eps)']
    cols = [(g, s) for g in TEXTURE_GROUPS for s in (0, 1, -1)]
    lines.append('%-14s' % 'kernel' + ''.join('%16s' % f'{g}{"0+-"[s]}' for g, s in cols))
    for k in sorted({key[0] for key in LEDGER}):
        for c in ('linear', 'cubic'):
            lines.append('%-14s' % f'{k} {c}' + ''.join('%16d' % LEDGER[(k, c, g, s)] for g, s in cols))
    lines.append('plane-quad forms (orientation, axis-0 split, class): ' + ', '.join(f'{k}: {v}' for k, v in sorted(QUAD_FORMS.items())))
    lines.append('bit identities compared: ' + ', '.join(f'{k}: {v}' for k, v in sorted(IDENTITIES.items())))
    lines.append('largest |got - oracle| per (kernel, interpolation): ' + ', '.join(f'{k}: {v:.3e}' for k, v in sorted(WORST.items())))
    return '\n'.join(lines)


def test_zz_coverage_ledger():
    """Every product family -- 1, 2, 6, 8, 9, 10 and the fused projection 7 -- served, for trilinear and for cubic (9: cubic only, the
    planner never picks it for trilinear), at least one case of every group: lattice with eps of either sign, float32 twin, face-exact,
    face-chain-dependent; and the plane-quad kernel was reached in the three forms the planner distinguishes on the axis-0 offset
    (fz == 0, fz tiny, fz == 1.0f) on the plain and on both exchanged orientations.  Last in the file; skips itself when only a selection
    of the file ran (-k, single nodes)."""
    print('\n' + ledger_report())
    if NODES_RUN != NODES_ALL:
        pytest.skip(f'only {len(NODES_RUN)} of {len(NODES_ALL)} nodes ran: the ledger describes a selection')
    missing = []
    for k in (1, 2, 6, 8, 9, 10, 7):
        for c in ('linear', 'cubic'):
            if k == 9 and c == 'linear':
                continue
            for g, s in (('lattice', 1), ('lattice', -1), ('f32twin', None), ('face_exact', None), ('face_chain', None)):
                n = sum(v for (kk, cc, gg, ss), v in LEDGER.items() if kk == k and cc == c and gg == g and (s is None or ss == s))
                if n == 0:
                    missing.append((k, c, g, s))
    for ori in ('plain', 'axis1', 'axis2'):
        for form in ('zero', 'tiny', 'one'):
            for c in ('linear', 'cubic'):
                if QUAD_FORMS[(ori, form, c)] == 0:
                    missing.append(('kind 8', ori, form, c))
    assert not missing, missing
