"""-m gpu: StaticVolume.warp_stack_sum (vt_volume_warp_stack_sum, kernel 26): the images warp_stack would write, summed under weight columns
without being written.  Two bit identities carry most of the file (compared as uint32, so the sign of a zero counts):

  1. column c == float32 of the host loop  acc = b; acc = acc + W[i, c] * double(S_i)  over S = warp_stack(..., weights=None) from the same
     handle with the same flags -- all five interpolations, both tiles, both routes;
  2. a one-hot column holds warp_stack's image k under that weight.

Parity with the float64 model (tests/warp_stack_sum_model.py) is held to TOL[interp] * sum_i |W[i, c]| per column: each term carries
warp_stack's bound TOL * |w_i| (tests/test_gpu_warp_stack.py), and the float64 additions are some 2^-29 below it.  The parity cases have
no pixel within SKIRT_EPS of a skirt face (tests/test_warp_stack_sum_host.py), so every pixel is compared.

Cases and shapes are tests/warp_stack_cases.py's: stack (6, 40, 52), output (37, 45) on the (1, 16, 16) tile with cut tiles, (61, 59) on
the (1, 32, 32) tile, n = 10; the weight columns are tests/warp_stack_sum_cases.py's."""
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, rand_vol

import warp_stack_cases as wc
import warp_stack_model as wsm
import warp_stack_sum_cases as sc
import warp_stack_sum_model as ssm
from warp_stack_cases import STACK, OUT, OUT32, TILE, PLANES, OUTSIDE

pytestmark = pytest.mark.gpu

VT_EUNSUPPORTED = 10004
FLAGS = (0, _native.FORCE_DIRECT)
GRID_SHAPES = ((2, 2), (3, 5), (1, 4), (1, 1), 'dense')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def data(seed=41, shape=STACK):
    s = rand_vol(shape, seed)
    s.setflags(write=False)
    return s


def handle(interp, src=None):
    return vt.StaticVolume(data() if src is None else src, interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))


def host_loop(S, W, start=None):
    """float32(acc) of acc = b; acc = acc + W[i, c] * double(S_i), i ascending: (G, Ho, Wo)."""
    return ssm.two_rounding_sum(S.astype(np.float64), W, start).astype(np.float32)


def check_info(sv, ms, g, n, out, interp, flags, G):
    info = sv.info()
    p = ssm.plan(ms, g, n, out, interp, G, force_direct=bool(flags))
    assert info.last_kernel == 26 and tuple(info.last_tile) == (1,) + tuple(p.tile), (info.last_kernel, tuple(info.last_tile))
    assert out not in TILE or tuple(info.last_tile) == TILE[out]
    assert info.last_grid == p.sum_grid, (info.last_grid, p.sum_grid)
    assert tuple(info.last_lds_dims) == tuple(p.sum_lds_dims) and info.last_lds_bytes == p.sum_lds_bytes, \
        (tuple(info.last_lds_dims), p.sum_lds_dims, info.last_lds_bytes, p.sum_lds_bytes)
    return p


# ---- 1. the host loop over warp_stack's images ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('out', [OUT, OUT32], ids=['16x16', '32x32'])
def test_column_is_the_host_loop_over_warp_stack_images(out, interp):
    names, W = sc.first(9)
    sv = handle(interp)
    try:
        for gs in GRID_SHAPES:
            for amp in wc.AMPLITUDES:
                own = wc.grids(gs, amp, out)
                for g in (own, own[4]):
                    for mats in (wc.batch(out), wc.batch(out).astype(np.float32)):
                        for flags in FLAGS:
                            S = sv.warp_stack(g, mats, out, planes=PLANES, _flags=flags).copy()
                            got = sv.warp_stack_sum(g, mats, out, W, planes=PLANES, _flags=flags)
                            check_info(sv, mats, g, 10, out, interp, flags, 9)
                            want = host_loop(S, W)
                            assert want[0].any() and same_bits(got, want), \
                                (interp, out, gs, amp, g.ndim, mats.dtype, flags, int((bits(got) != bits(want)).sum()))
        # matrices=None: the identity for the T images
        g = wc.grids((3, 5), 1.5, out, STACK[0], 9)
        for flags in FLAGS:
            S = sv.warp_stack(g, None, out, _flags=flags).copy()
            got = sv.warp_stack_sum(g, None, out, W[:STACK[0]], _flags=flags)
            assert same_bits(got, host_loop(S, W[:STACK[0]])), (interp, out, flags)
            none = sv.warp_stack_sum(g, None, out, _flags=flags)
            assert none.shape == out and same_bits(none, host_loop(S, None)[0])
    finally:
        sv.close()


# ---- 2. one-hot columns ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_one_hot_columns_are_warp_stack_images(interp):
    names, W = sc.first(9)
    sv = handle(interp)
    try:
        for out in (OUT, OUT32):
            for gs, amp in (((3, 5), 1.5), ('dense', 12.0)):
                g = wc.grids(gs, amp, out)
                for flags in FLAGS:
                    got = sv.warp_stack_sum(g, wc.batch(out), out, W, planes=PLANES, _flags=flags).copy()
                    for name, k in (('hot_inside', sc.INSIDE), ('hot_outside', OUTSIDE), ('hot_last', sc.LAST)):
                        img = sv.warp_stack(g, wc.batch(out), out, sc.COLUMNS[name], planes=PLANES, _flags=flags)
                        assert same_bits(got[names.index(name)], img[k]), (interp, out, gs, flags, name)
                        assert not bits(np.delete(img, k, axis=0)).any()
                    assert got[names.index('hot_inside')].any() and got[names.index('hot_last')].any()
                    assert not bits(got[names.index('zero')]).any() and not bits(got[names.index('hot_outside')]).any()      # +0 bits
    finally:
        sv.close()


# ---- 3. parity with the model --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('out', [OUT, OUT32], ids=['16x16', '32x32'])
def test_parity_against_the_model(out, interp):
    names, W = sc.first(9)
    sv = handle(interp)
    try:
        for name, o, ms, g in wc.parity_cases():
            if o != out:
                continue
            n = len(g)
            planes = PLANES if ms is not None else None
            Wn = W[:n]
            want, kept = ssm.warp_stack_sum(data(), ms, g, planes, out, interp, Wn)
            assert kept.mean() >= 0.999
            bound = TOL[interp] * np.abs(Wn).sum(axis=0)
            for flags in FLAGS:
                got = sv.warp_stack_sum(g, ms, out, Wn, planes=planes, _flags=flags)
                assert got.dtype == np.float32 and got.shape == want.shape
                for c in range(9):
                    err = float(np.abs(got[c].astype(np.float64) - want[c])[kept].max())
                    print(f'{interp} {name} flags={flags} column {names[c]}: max|hip - model| {err:.3e}  bound {bound[c]:.3e}')
                    assert err <= bound[c], (interp, name, flags, names[c], err, bound[c])
    finally:
        sv.close()


# ---- 4. independence -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_a_column_does_not_depend_on_g_or_its_place(interp):
    ms = wc.batch()
    g = wc.grids((3, 5), 12.0)
    sv = handle(interp)
    try:
        for flags in FLAGS:
            alone = {k: sv.warp_stack_sum(g, ms, OUT, sc.COLUMNS[k], planes=PLANES, _flags=flags).copy() for k in sc.NAMES}
            assert sv.info().last_grid == 9                                                      # G = 1: one chunk x 3 x 3 tiles
            assert alone['ones'].any() and alone['ramp'].any()
            for G in sc.G_VALUES:
                names, W = sc.first(G)
                got = sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES, _flags=flags)
                assert got.shape == (G,) + OUT and sv.info().last_grid == 9 * -(-G // sc.GC)
                for c, k in enumerate(names):
                    assert same_bits(got[c], alone[k]), (interp, flags, G, k)
            for names, W in sc.placements():
                got = sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES, _flags=flags)
                for c, k in enumerate(names):
                    assert same_bits(got[c], alone[k]), (interp, flags, names, k)
            # (n,) and (n, 1) differ in shape only
            col = sv.warp_stack_sum(g, ms, OUT, sc.COLUMNS['mixed'][:, None], planes=PLANES, _flags=flags)
            assert col.shape == (1,) + OUT and same_bits(col[0], alone['mixed'])
            # a shared grid against n copies of it
            names, W = sc.first(5)
            for gs, amp in (((3, 5), 1.5), ('dense', 12.0), ((1, 1), 1.5)):
                G1 = wc.grids(gs, amp)[4]
                a = sv.warp_stack_sum(G1, ms, OUT, W, planes=PLANES, _flags=flags).copy()
                b = sv.warp_stack_sum(np.tile(G1[None], (10, 1, 1, 1)), ms, OUT, W, planes=PLANES, _flags=flags)
                assert a.any() and same_bits(a, b), (interp, gs, flags)
    finally:
        sv.close()


def test_output_kinds_earlier_calls_and_recycled_memory():
    ms = wc.batch()
    g = wc.grids((3, 5), 1.5)
    names, W = sc.first(5)
    shape = (5,) + OUT
    for interp in ('linear', 'filt_bspline'):
        sv = handle(interp)
        fresh = sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES).copy()
        host = np.full(shape, 5, np.float32)
        assert sv.warp_stack_sum(g, ms, OUT, W, output=host, planes=PLANES) is None and same_bits(host, fresh)
        dev = vt.empty(shape, device='gpu:0')
        dev.set(np.full(shape, 5, np.float32))
        assert sv.warp_stack_sum(g, ms, OUT, W, output=dev, planes=PLANES) is None
        sv.synchronize()
        assert same_bits(dev.get(), fresh)
        assert (sv.info().out_depth, sv.info().out_height, sv.info().out_width) == STACK          # the handle's own output shape is untouched
        # earlier calls of other entry points share the table buffers
        vol = (12, 20, 24)
        sv.backproject(vt.utils.backproject_matrices(np.linspace(-50.0, 50.0, 6), 1, vol, STACK), vol)
        assert same_bits(sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES), fresh)
        sv.warp_stack(wc.grids('dense', 12.0, OUT32), wc.batch(OUT32), OUT32, planes=PLANES)
        assert same_bits(sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES), fresh)
        sv.warp_stack_sum(wc.grids('dense', 12.0, OUT32), wc.batch(OUT32), OUT32, sc.first(9)[1], planes=PLANES)
        assert same_bits(sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES), fresh)
        sv.close()
        # a handle whose resident buffer is the recycled allocation of one that held 1e3
        big = vt.StaticVolume(np.full(STACK, 1e3, np.float32), interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))
        big.warp_stack_sum(g, ms, OUT, W, planes=PLANES)
        big.close()
        other = handle(interp)
        assert same_bits(other.warp_stack_sum(g, ms, OUT, W, planes=PLANES), fresh)
        other.close()


# ---- 5. accumulate -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_accumulate_continues_the_host_loop(interp):
    ms = wc.batch()
    g = wc.grids((3, 5), 1.5)
    names, W = sc.first(5)
    sv = handle(interp)
    try:
        for flags in FLAGS:
            S = sv.warp_stack(g, ms, OUT, planes=PLANES, _flags=flags).copy()
            out = np.full((5,) + OUT, 7, np.float32)
            assert sv.warp_stack_sum(g[:5], ms[:5], OUT, W[:5], output=out, planes=PLANES[:5], _flags=flags) is None
            first = out.copy()
            assert same_bits(first, host_loop(S[:5], W[:5]))
            assert sv.warp_stack_sum(g[5:], ms[5:], OUT, W[5:], output=out, planes=PLANES[5:], accumulate=True, _flags=flags) is None
            want = host_loop(S[5:], W[5:], start=first.astype(np.float64))
            # up to the sign of a zero found in `out`: compare values, and bits where the start is not a zero
            assert np.array_equal(out, want) and np.array_equal(bits(out)[first != 0], bits(want)[first != 0]), (interp, flags)
            # device output
            dev = vt.empty((5,) + OUT, device='gpu:0')
            dev.set(first)
            sv.warp_stack_sum(g[5:], ms[5:], OUT, W[5:], output=dev, planes=PLANES[5:], accumulate=True, _flags=flags)
            sv.synchronize()
            assert same_bits(dev.get(), out)
        # tiles that no entry reaches keep what was there, a NaN included
        m1, g1, p1, w1 = wc.pushed_out_case()
        what = wsm.tile_outcome(wsm.plan(m1, g1, 1, OUT, interp), m1, STACK[1:])
        assert (what[0, :, 2] == 'zero').all()
        for flags in FLAGS:
            out = np.full(OUT, 5.0, np.float32)
            out[3, 40] = np.nan
            out[20, 33] = -0.0
            before = out.copy()
            sv.warp_stack_sum(g1, m1, OUT, w1, output=out, planes=p1, accumulate=True, _flags=flags)
            assert np.array_equal(bits(out[:, 32:]), bits(before[:, 32:])), (interp, flags)
            S = sv.warp_stack(g1, m1, OUT, planes=p1, _flags=flags)
            assert same_bits(out[:, :32], host_loop(S, w1, start=before.astype(np.float64)[None])[0][:, :32])
            assert (out[:, :20] != 5.0).any()
    finally:
        sv.close()


# ---- 6. the routes, read from info() against plan() --------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_routes(interp):
    sv = handle(interp)
    try:
        for key, (ms, g, planes, w) in wc.route_cases().items():
            n = len(ms)
            W = np.stack([w, np.ones(n), -0.5 * w], axis=1)
            for flags in FLAGS:
                S = sv.warp_stack(g, ms, OUT, planes=planes, _flags=flags).copy()
                got = sv.warp_stack_sum(g, ms, OUT, W, planes=planes, _flags=flags)
                p = check_info(sv, ms, g, n, OUT, interp, flags, 3)
                if flags:
                    assert tuple(sv.info().last_lds_dims) == (0, 0, 0)
                assert (S.any() or key == 'hull') and same_bits(got, host_loop(S, W)), (interp, key, flags)      # (hull: every pixel is pushed out)
            p = ssm.plan(ms, g, n, OUT, interp, 3)
            if key == 'spike':                       # calm entries stage, the spiked one gathers, inside one workgroup's walk
                assert p.sum_lds_dims == (2,) + wsm.CAP_DIMS[1:] and p.staged[0].all() and p.staged[2].all() and not p.staged[1].any()
            elif key == 'hull':
                assert p.flag.all() and not p.hull.any()
            else:
                assert not p.flag.any() and p.sum_lds_dims == (0, 0, 0), key
    finally:
        sv.close()


# ---- 7. small and odd shapes -----------------------------------------------------------------------------------------------------------
SMALL_CASES = wc.SMALL_CASES


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
@pytest.mark.parametrize('shape,out,gs', SMALL_CASES, ids=[f'{"x".join(map(str, s))}-{"x".join(map(str, o))}-{"x".join(map(str, g))}'
                                                          for s, o, g in SMALL_CASES])
def test_small_and_odd_shapes(shape, out, gs, interp):
    src = data(47, shape)
    ms, g, planes, w = wc.small_case(shape, out, gs)
    W = np.stack([w, np.ones(3), np.array([0.0, 2.0, 0.0]), -w, np.array([1.0, 0.0, 0.0])], axis=1)       # T = 1 included; G = GC + 1
    sv = handle(interp, src)
    try:
        for flags in FLAGS:
            S = sv.warp_stack(g, ms, out, planes=planes, _flags=flags).copy()
            got = sv.warp_stack_sum(g, ms, out, W, planes=planes, _flags=flags)
            check_info(sv, ms, g, 3, out, interp, flags, 5)
            assert S.any() and same_bits(got, host_loop(S, W)), (interp, shape, out, gs, flags)
    finally:
        sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_pushed_out_tiles(interp):
    ms, g, planes, w = wc.pushed_out_case()
    sv = handle(interp)
    try:
        for flags in FLAGS:
            S = sv.warp_stack(g, ms, OUT, planes=planes, _flags=flags).copy()
            got = sv.warp_stack_sum(g, ms, OUT, np.stack([w, -w], axis=1), planes=planes, _flags=flags)
            assert same_bits(got, host_loop(S, np.stack([w, -w], axis=1))) and got[0][:, :20].any()
            assert not bits(got[:, :, 32:]).any()                                               # +0, not -0
    finally:
        sv.close()


# ---- 8. non-finite data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_non_finite_pixels_reach_their_stencils_only(interp):
    """test_gpu_warp_stack's construction (no coordinate within 1e-3 of an integer, so every tap of a stencil has a non-zero weight).  A
    column is non-finite exactly where an entry with a non-zero weight in it has a non-finite sample.  The zero pattern is the same in
    every column of a chunk (columns 0-3: entry 2 is 0; column 4: only entry 2 counts), so no 0 x NaN is in question."""
    src = np.array(data())
    src[1, 17, 23] = np.nan
    src[1, 9, 40] = np.inf
    src[4, 0, 0] = np.inf
    src[4, 39, 51] = np.nan
    ms = np.zeros((4, 4, 4))
    ms[:, 0, 0] = ms[:, 3, 3] = 1
    ms[0, 1:3, 1:] = [(0.8, 0.1, 3.33), (0.1, 0.9, 5.47)]
    ms[1, 1:3, 1:] = [(1.2, -0.3, 2.25), (0.3, 1.1, 4.55)]
    ms[2, 1:3, 1:] = [(1.0, 0.0, -1.35), (0.0, 1.0, -2.65)]
    ms[3, 1:3, 1:] = [(0.9, 0.2, 5.15), (-0.2, 1.3, 9.75)]
    g = np.zeros((4, 2, 2, 2), np.float32)
    g[:] = np.array([(0.05, -0.02), (0.02, -0.02), (0.1, 0.2), (0.03, -0.03)], np.float32)[:, None, None, :]
    g[:, 0, 1] += np.float32(0.004)
    g[:, 1, 0] -= np.float32(0.004)
    planes = np.array([1, 1, 4, 4])
    W = np.array([[1.0, 0.5, -1.0, 2.0, 0.0], [-2.0, 1.0, 0.25, 1.0, 0.0], [0.0, 0.0, 0.0, 0.0, 2.0], [1.5, -1.0, 1.0, 0.5, 0.0]])
    y = np.stack([np.stack(wsm.coords(ms[i], g[i], OUT)) for i in range(4)])
    assert np.abs(y - np.round(y)).min() > 1e-3
    vols, masks, dist = wsm.warp_stack(src, ms, g, planes, OUT, interp)
    bad = ~np.isfinite(vols)
    assert all(b.any() for b in bad) and not bad.all()
    want_bad = np.stack([(bad & (W[:, c] != 0)[:, None, None]).any(axis=0) for c in range(5)])
    clean = np.where(bad, 0.0, vols)
    want = ssm.two_rounding_sum(clean, W)
    sv = handle(interp, src)
    try:
        for flags in FLAGS:
            got = sv.warp_stack_sum(g, ms, OUT, W, planes=planes, _flags=flags)
            assert np.array_equal(~np.isfinite(got), want_bad), (interp, flags, int((~np.isfinite(got) != want_bad).sum()))
            for c in range(5):
                ok = ~want_bad[c]
                err = np.abs(got[c].astype(np.float64) - want[c])[ok].max()
                assert err <= TOL[interp] * np.abs(W[:, c]).sum(), (interp, flags, c, err)
    finally:
        sv.close()


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    ms = wc.batch()
    m1 = np.ascontiguousarray(ms[:1], dtype=np.float32)
    g1 = np.ascontiguousarray(wc.grids((3, 5), 1.5)[:1])
    out = np.zeros((2,) + OUT, np.float32)
    p0 = np.zeros(1, np.int32)
    w2 = np.array([[1.0, -0.5]])

    def call(h, n=1, mat=m1, grids=g1, n_grids=1, gdims=(3, 5), planes=p0, G=2, w=w2, shape=OUT, flags=0, f64=False, o=out):
        fn = lib.vt_volume_warp_stack_sum_f64 if f64 else lib.vt_volume_warp_stack_sum
        mat = None if mat is None else np.ascontiguousarray(mat, dtype=np.float64 if f64 else np.float32)
        return fn(h, n, None if mat is None else mat.ctypes.data, None if grids is None else grids.ctypes.data, n_grids, *gdims,
                  None if planes is None else planes.ctypes.data, G, None if w is None else w.ctypes.data, *shape,
                  None if o is None else o.ctypes.data, flags)

    # filt_* without VT_STACK, in Python and by the library; VT_EDGE_SCIPY
    sv = vt.StaticVolume(data(), interpolation='filt_bspline', device='gpu:0')
    with pytest.raises(ValueError):
        sv.warp_stack_sum(g1[0], ms, OUT, planes=PLANES)
    assert call(sv._handle) == VT_EUNSUPPORTED and b'VT_STACK' in lib.vt_last_error()
    assert call(sv._handle, f64=True) == VT_EUNSUPPORTED
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()
    sv = vt.StaticVolume(data(), device='gpu:0', edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    with pytest.raises(RuntimeError, match=f'code {VT_EUNSUPPORTED}'):
        sv.warp_stack_sum(g1[0], ms, OUT, planes=PLANES)
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()

    sv = handle('bspline')
    hd = sv._handle
    want = sv.warp_stack_sum(g1, m1, OUT, w2, planes=[0]).copy()
    assert want.any()

    def good():
        out[...] = 3
        _native.check(call(hd), 'warp_stack_sum')
        assert same_bits(out, want)

    def refused(code, word, **kw):
        for f64 in (False, True):
            assert call(hd, f64=f64, **kw) == code and (word is None or word in lib.vt_last_error()), (kw, lib.vt_last_error())
        good()

    bad = m1.copy()
    bad[0, 1, 2] = np.nan
    refused(VT_EINVAL, b'finite', mat=bad)
    for p in ([STACK[0]], [-1]):
        refused(VT_EINVAL, b'plane', planes=np.array(p, np.int32))
    refused(VT_EINVAL, b'plane', planes=None)                                                   # n = 1 != T
    for v in (np.inf, np.nan):
        refused(VT_EINVAL, b'weight', w=np.array([[1.0, v]]))
    for shape in ((0, 45), (37, -1)):
        refused(VT_EINVAL, None, shape=shape)
    refused(VT_EINVAL, None, n=0)
    refused(VT_EINVAL, None, n=-2)
    # the refusals of this entry point
    for G in (0, -3):
        refused(VT_EINVAL, b'column', G=G)
    refused(VT_EINVAL, b'NULL weights', w=None)                                                 # without weights there is one column
    for ng in (0, 2, -1):
        refused(VT_EINVAL, b'grids', n_grids=ng)
    for gd in ((0, 5), (3, 0), (3, 46), (38, 5), (-1, 5)):
        refused(VT_EINVAL, b'grid dims', gdims=gd)
    for v in (np.nan, np.inf, -np.inf):
        gb = g1.copy()
        gb[0, 2, 4, 1] = v
        refused(VT_EINVAL, b'node', grids=gb)
    refused(VT_EINVAL, b'NULL', grids=None)
    refused(VT_EINVAL, None, o=None)
    # the bounds, decided before anything is read: 2^31 columns' worth of chunks x 9 tiles; 2^27 grids x 15 nodes x 2
    refused(VT_EUNSUPPORTED, b'grid too large', G=0x7fffffff)
    refused(VT_EUNSUPPORTED, b'grids too large', n=1 << 27, n_grids=1 << 27)
    # weights == NULL with one column is a column of ones; matrices == NULL is the identity; other flags are ignored
    _native.check(call(hd, G=1, w=None), 'warp_stack_sum, NULL weights')
    assert same_bits(out[0], sv.warp_stack_sum(g1, m1, OUT, planes=[0]))
    _native.check(call(hd, flags=_native.KEEP_OUTSIDE | _native.NO_MARCH), 'warp_stack_sum')
    assert same_bits(out, want)
    _native.check(call(hd, mat=None), 'warp_stack_sum, NULL matrices')
    assert same_bits(out, sv.warp_stack_sum(g1, np.eye(3)[None], OUT, w2, planes=[0]))
    sv.close()


# ---- 10. find_shifts -> motion_corrected_sum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_find_shifts_into_motion_corrected_sum(interp):
    """Six frames cut from one larger image at known integer offsets: find_shifts measures them on every patch of a 2 x 2 grid, and the
    sum through those displacements is six times the unshifted frame wherever all six frames hold the pixel -- to the interpolation's
    tolerance per frame on unit-range data (coordinates are integers: a linear sample is the pixel, an interpolating spline returns it
    within TOL).  The interior stays 16 pixels off the frames' borders, where what the in-plane prefilter makes of the zero boundary
    (it decays by 0.27 per pixel) is below 1e-9."""
    H, W, pad, margin = 64, 80, 4, 16
    big = np.random.RandomState(5).random_sample((H + 2 * pad, W + 2 * pad)).astype(np.float32)
    shifts = np.array([(0, 0), (1, -2), (-3, 1), (2, 2), (-1, -3), (3, 0)])
    base = big[pad:pad + H, pad:pad + W]
    movie = np.stack([big[pad - dy:pad - dy + H, pad - dx:pad - dx + W] for dy, dx in shifts])        # frame_i[y + d_i] = base[y]
    lin = vt.StaticVolume(movie, interpolation='linear', device='gpu:0')
    d = lin.find_shifts(base, (4, 4), (2, 2), subpixel=False, normalized=True)
    lin.close()
    assert d.shape == (6, 2, 2, 2)
    assert np.array_equal(d, np.broadcast_to(shifts[:, None, None, :].astype(np.float64), d.shape))
    sv = handle(interp, movie)
    try:
        got = sv.motion_corrected_sum(d, halves=True)
        assert sv.info().last_kernel == 26 and got.shape == (3, H, W)
        inner = (slice(margin, H - margin), slice(margin, W - margin))
        for c, k in enumerate((6, 3, 3)):
            err = float(np.abs(got[c][inner].astype(np.float64) - k * base[inner].astype(np.float64)).max())
            print(f'{interp} column {c}: max|sum - {k} x frame| {err:.3e}  bound {k * TOL[interp]:.3e}')
            assert err <= k * TOL[interp], (interp, c, err)
    finally:
        sv.close()
