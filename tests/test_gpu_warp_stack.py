"""-m gpu: StaticVolume.warp_stack (vt_volume_warp_stack, kernel 22): every image of a resident stack through its own 2-D displacement grid.
The definition is tests/warp_stack_model.py times the entry's weight; tolerances are TOL of tests/test_gpu_extract.py on unit-range data
times |w_i|.  Bit identities are compared as uint32, so the sign of a zero counts.  Pixels within SKIRT_EPS of a skirt face, where float64
rounding may decide the inside test either way, are left out of the comparisons with the model; tests/test_warp_stack_host.py holds
their share to 0.001 per case (the exact lattice case leaves none out).

The cases live in tests/warp_stack_cases.py.  The stack is (6, 40, 52); output (37, 45) takes the (1, 16, 16) tile with cut tiles on both
axes, (61, 59) the (1, 32, 32) tile."""
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, rand_vol
from test_gpu_box_lattice import positive

import warp_stack_cases as wc
import warp_stack_model as wsm
from warp_stack_cases import STACK, OUT, OUT32, TILE, PLANES, WEIGHTS, NONZERO, OUTSIDE

pytestmark = pytest.mark.gpu

VT_EUNSUPPORTED = 10004
FLAGS = (0, _native.FORCE_DIRECT)


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


def tiles_in(out, tile):
    return -(-out[0] // tile[1]) * -(-out[1] // tile[2])


def model(src, ms, g, planes, out, interp):
    """(B (n, Ho, Wo) float64, inside masks, kept: the pixels farther than SKIRT_EPS from every skirt face)."""
    vols, masks, dist = wsm.warp_stack(src, ms, g, planes, out, interp)
    with np.errstate(invalid='ignore'):
        kept = ~(dist <= wsm.SKIRT_EPS)
    assert kept.mean() >= 0.999
    return vols, masks, kept


def check_entries(got, vols, kept, w, tol, what):
    """Every kept pixel of every entry: |got_i - w_i B_i| <= |w_i| tol."""
    assert got.dtype == np.float32 and got.shape == vols.shape, what
    for i in range(len(vols)):
        err = float(np.abs(got[i].astype(np.float64) - w[i] * vols[i])[kept[i]].max()) if kept[i].any() else 0.0
        print(what, f'entry {i}: max|hip - model| {err:.3e}  bound {abs(w[i]) * tol:.3e}')
        assert err <= abs(w[i]) * tol, (what, i, err)


def check_info(sv, ms, g, n, out, interp, flags):
    info = sv.info()
    p = wsm.plan(ms, g, n, out, interp, force_direct=bool(flags))
    assert info.last_kernel == 22 and tuple(info.last_tile) == TILE.get(out, tuple(info.last_tile)), (info.last_kernel, tuple(info.last_tile))
    assert tuple(info.last_tile) == (1,) + tuple(p.tile) and info.last_grid == n * p.nT[0] * p.nT[1]
    assert tuple(info.last_lds_dims) == tuple(p.lds_dims) and info.last_lds_bytes == p.lds_bytes, \
        (tuple(info.last_lds_dims), p.lds_dims, info.last_lds_bytes, p.lds_bytes)
    if flags:
        assert tuple(info.last_lds_dims) == (0, 0, 0)
    return p


# ---- 1. parity, and the two routes against each other ------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('out', [OUT, OUT32], ids=['16x16', '32x32'])
def test_parity_against_the_model(out, interp):
    sv = handle(interp)
    try:
        for name, o, ms, g in wc.parity_cases():
            if o != out:
                continue
            n = len(g)
            planes, w = (PLANES, WEIGHTS) if ms is not None else (None, None)
            for f32 in ((False, True) if ms is not None else (False,)):
                mats = ms.astype(np.float32) if f32 else ms
                vols, masks, kept = model(data(), None if ms is None else mats.astype(np.float64), g, planes, out, interp)
                if ms is not None and not name.endswith('12.0'):
                    assert not masks[OUTSIDE].any() and all(masks[i].any() for i in range(10) if i != OUTSIDE)
                got = {}
                for flags in FLAGS:
                    got[flags] = sv.warp_stack(g, mats, out, w, planes=planes, _flags=flags)
                    check_info(sv, mats, g, n, out, interp, flags)
                    check_entries(got[flags], vols, kept, np.ones(n) if w is None else w, TOL[interp], (interp, name, f32, flags))
                    if ms is not None:
                        assert not bits(got[flags][OUTSIDE]).any() and not bits(got[flags][3]).any()      # all outside, weight 0: +0
                if interp == 'linear':                                                  # the same taps and arithmetic on both routes
                    assert same_bits(got[0], got[FLAGS[1]]), (name, f32)
                else:
                    err = np.abs(got[0].astype(np.float64) - got[FLAGS[1]])
                    for i in range(n):
                        assert float(err[i].max()) <= abs(1.0 if w is None else w[i]) * TOL[interp], (interp, name, i)
    finally:
        sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
@pytest.mark.parametrize('out', [OUT, OUT32], ids=['16x16', '32x32'])
def test_inside_mask_pixel_for_pixel(out, interp):
    """Data in [1, 2) and weights without a zero: inside the skirt the smallest weight on a real tap is positive, so `got != 0` is the
    model's mask on the kept pixels."""
    src = positive(data())
    sv = handle(interp, src)
    try:
        for gs, amp in (((3, 5), 12.0), ('dense', 1.5), ((1, 4), 12.0)):
            g = wc.grids(gs, amp, out)
            _, masks, kept = model(src, wc.batch(out), g, PLANES, out, interp)
            for flags in FLAGS:
                got = sv.warp_stack(g, wc.batch(out), out, NONZERO, planes=PLANES, _flags=flags)
                for i in range(10):
                    differs = int((((got[i] != 0) != masks[i]) & kept[i]).sum())
                    assert differs == 0, (interp, out, gs, flags, i, differs)
                    assert not bits(got[i][~masks[i] & kept[i]]).any()                  # outside: +0, not -0
    finally:
        sv.close()


# ---- 2. bit identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_zero_grid_gives_affine_stack_bits(interp):
    sv = handle(interp)
    try:
        for out in (OUT, OUT32):
            for ms in (wc.batch(out), wc.batch(out).astype(np.float32)):
                for flags in FLAGS:
                    want = sv.affine_stack(ms, out, WEIGHTS, planes=PLANES, _flags=flags).copy()
                    assert sv.info().last_kernel == 21
                    for g in (np.zeros((2, 2, 2)), np.zeros((10, 3, 5, 2)), np.zeros((1, 1, 2)), np.zeros((10,) + out + (2,)), np.zeros((1, 4, 2))):
                        got = sv.warp_stack(g, ms, out, WEIGHTS, planes=PLANES, _flags=flags)
                        assert sv.info().last_kernel == 22
                        assert same_bits(got, want), (interp, out, ms.dtype, flags, g.shape, int((bits(got) != bits(want)).sum()))
    finally:
        sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_shared_grid_is_n_copies(interp):
    sv = handle(interp)
    try:
        for out in (OUT, OUT32):
            for gs, amp in (((3, 5), 1.5), ('dense', 12.0), ((1, 1), 1.5)):
                G = wc.grids(gs, amp, out)[4]
                for flags in FLAGS:
                    a = sv.warp_stack(G, wc.batch(out), out, WEIGHTS, planes=PLANES, _flags=flags).copy()
                    b = sv.warp_stack(np.tile(G[None], (10, 1, 1, 1)), wc.batch(out), out, WEIGHTS, planes=PLANES, _flags=flags)
                    assert a.any() and same_bits(a, b), (interp, out, gs, flags)
    finally:
        sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_dyadic_constant_grid_folds_into_the_translation(interp):
    """Integer shifts and a dyadic constant grid: the chain and the lerps are exact, so warp_stack writes affine_stack's bits for the
    matrices with the constant added to the translation -- every pixel, those exactly on the lattice and on the skirt faces included."""
    ms, g, folded, planes = wc.lattice_case()
    w = np.array([1.0, -0.5, 2.0, 0.75, 1.5, -1.25])
    sv = handle(interp)
    try:
        for out in (OUT, OUT32, STACK[1:]):
            for flags in FLAGS:
                want = sv.affine_stack(folded, out, w, planes=planes, _flags=flags).copy()
                got = sv.warp_stack(g, ms, out, w, planes=planes, _flags=flags)
                assert want.any() and same_bits(got, want), (interp, out, flags, int((bits(got) != bits(want)).sum()))
    finally:
        sv.close()


def test_one_entry_against_warp():
    """Linear only, to TOL: the route of the parent commit -- warp on the same handle with output (1, Ho, Wo), row 0 = (0, 0, 0, plane) and
    component 0 of the grid zero."""
    sv = handle('linear')
    try:
        for out in (OUT, OUT32):
            for gs, amp in (((3, 5), 1.5), ((2, 2), 12.0), ('dense', 1.5), ((1, 4), 12.0)):
                g = wc.grids(gs, amp, out)
                for i in (1, 5, 9):
                    got = sv.warp_stack(g[i:i + 1], wc.batch(out)[i:i + 1], out, planes=PLANES[i:i + 1])[0].copy()
                    m = np.array(wc.batch(out)[i])
                    m[0] = (0, 0, 0, PLANES[i])
                    m[1:3, 0] = 0
                    g3 = np.zeros((1,) + g.shape[1:3] + (3,), np.float32)
                    g3[0, ..., 1:] = g[i]
                    want = sv.warp(g3, m, (1,) + out)[0]
                    assert sv.info().last_kernel == 20
                    err = float(np.abs(got.astype(np.float64) - want).max())
                    assert got.any() and err <= TOL['linear'], (out, gs, i, err)
    finally:
        sv.close()


# ---- 3. independence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_an_image_does_not_depend_on_the_batch(interp):
    ms = wc.batch()
    g = wc.grids((3, 5), 12.0)
    sv = handle(interp)
    try:
        for flags in FLAGS:
            full = sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES, _flags=flags).copy()
            assert full.any()
            assert same_bits(sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES, _flags=flags), full)           # repeated
            for perm in (np.arange(10)[::-1], np.array([4, 0, 6, 2, 9, 5, 1, 8, 3, 7])):
                got = sv.warp_stack(g[perm], ms[perm], OUT, WEIGHTS[perm], planes=PLANES[perm], _flags=flags)
                assert same_bits(got, full[perm]), (interp, flags, perm)
            for i in range(10):
                got = sv.warp_stack(g[i:i + 1], ms[i:i + 1], OUT, WEIGHTS[i:i + 1], planes=PLANES[i:i + 1], _flags=flags)
                assert sv.info().last_grid == tiles_in(OUT, TILE[OUT]) and same_bits(got[0], full[i]), (interp, flags, i)
            many = sv.warp_stack(np.tile(g, (31, 1, 1, 1)), np.tile(ms, (31, 1, 1)), OUT, np.tile(WEIGHTS, 31), planes=np.tile(PLANES, 31),
                                 _flags=flags)
            assert sv.info().last_grid == 310 * tiles_in(OUT, TILE[OUT])
            assert same_bits(many, np.tile(full, (31, 1, 1))), (interp, flags)
        # a neighbour with a 200-pixel spike: its own tiles gather, the calm entries stage, and write what they write alone
        sm, sg, sp, sw = wc.spike_case()
        got = sv.warp_stack(sg, sm, OUT, sw, planes=sp).copy()
        p = check_info(sv, sm, sg, 3, OUT, interp, 0)
        assert p.staged[0].all() and p.staged[2].all() and not p.staged[1].any()
        vols, _, kept = model(data(), sm, sg, sp, OUT, interp)
        check_entries(got, vols, kept, sw, TOL[interp], (interp, 'spike'))
        for i in (0, 2):
            alone = sv.warp_stack(sg[i:i + 1], sm[i:i + 1], OUT, sw[i:i + 1], planes=sp[i:i + 1])
            assert tuple(sv.info().last_lds_dims) != wsm.CAP_DIMS and same_bits(alone[0], got[i]), (interp, i)
    finally:
        sv.close()


def test_output_kinds_earlier_calls_and_recycled_memory():
    ms = wc.batch()
    g = wc.grids((3, 5), 1.5)
    shape = (10,) + OUT
    for interp in ('linear', 'filt_bspline'):
        sv = handle(interp)
        fresh = sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES).copy()
        host = np.full(shape, 5, np.float32)
        assert sv.warp_stack(g, ms, OUT, WEIGHTS, output=host, planes=PLANES) is None and same_bits(host, fresh)
        dev = vt.empty(shape, device='gpu:0')
        dev.set(np.full(shape, 5, np.float32))
        assert sv.warp_stack(g, ms, OUT, WEIGHTS, output=dev, planes=PLANES) is None
        sv.synchronize()
        assert same_bits(dev.get(), fresh)
        assert (sv.info().out_depth, sv.info().out_height, sv.info().out_width) == STACK          # the handle's own output shape is untouched
        # earlier calls of other entry points share the table buffers
        vol = (12, 20, 24)
        sv.backproject(vt.utils.backproject_matrices(np.linspace(-50.0, 50.0, 6), 1, vol, STACK), vol)
        assert same_bits(sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES), fresh)
        sv.affine_stack(ms[:6][::-1], OUT32)
        assert same_bits(sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES), fresh)
        if interp == 'linear':
            sv.warp(np.ones((2, 2, 2, 3), np.float32))
            assert sv.info().last_kernel == 20
            assert same_bits(sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES), fresh)
        sv.close()
        # a handle whose resident buffer is the recycled allocation of one that held 1e3
        big = vt.StaticVolume(np.full(STACK, 1e3, np.float32), interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))
        big.warp_stack(g, ms, OUT, planes=PLANES)
        big.close()
        other = handle(interp)
        assert same_bits(other.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES), fresh)
        other.close()


def test_torch_output():
    torch = pytest.importorskip('torch')
    ms = wc.batch()
    g = wc.grids((3, 5), 1.5)
    sv = handle('bspline')
    fresh = sv.warp_stack(g, ms, OUT, WEIGHTS, planes=PLANES).copy()
    tens = torch.full((10,) + OUT, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.warp_stack(g, ms, OUT, WEIGHTS, output=tens, planes=PLANES) is None
    sv.synchronize()
    assert same_bits(tens.cpu().numpy(), fresh)
    sv.close()


# ---- 4. the routes, read from info() against plan() --------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_routes(interp):
    sv = handle(interp)
    try:
        for key, (ms, g, planes, w) in wc.route_cases().items():
            n = len(ms)
            vols, masks, kept = model(data(), ms, g, planes, OUT, interp)
            got = {}
            for flags in FLAGS:
                got[flags] = sv.warp_stack(g, ms, OUT, w, planes=planes, _flags=flags).copy()
                p = check_info(sv, ms, g, n, OUT, interp, flags)
                check_entries(got[flags], vols, kept, w, TOL[interp], (interp, key, flags))
            p = wsm.plan(ms, g, n, OUT, interp)
            if key == 'spike':
                assert p.lds_dims == wsm.CAP_DIMS and p.staged[0].all() and not p.staged[1].any()
            elif key == 'hull':
                assert p.flag.all() and not p.hull.any() and p.lds_dims == wsm.CAP_DIMS
            else:
                assert not p.flag.any() and p.lds_dims == (0, 0, 0) and masks.any(), key
            if interp == 'linear':
                assert same_bits(got[0], got[FLAGS[1]]), key
        # a pushed-out grid column: the tiles that see pushed-out nodes only are classified wholly outside and store +0
        ms, g, planes, w = wc.pushed_out_case()
        vols, masks, kept = model(data(), ms, g, planes, OUT, interp)
        what = wsm.tile_outcome(wsm.plan(ms, g, 1, OUT, interp), ms, STACK[1:])
        assert (what[0, :, 2] == 'zero').all() and masks[0][:, :20].any() and not masks[0][:, 32:].any()
        for flags in FLAGS:
            got = sv.warp_stack(g, ms, OUT, w, planes=planes, _flags=flags)
            check_entries(got, vols, kept, w, TOL[interp], (interp, 'pushed out', flags))
            assert not bits(got[0][:, 32:]).any()
    finally:
        sv.close()


# ---- 5. small and odd shapes -----------------------------------------------------------------------------------------------------------
SMALL_CASES = wc.SMALL_CASES


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
@pytest.mark.parametrize('shape,out,gs', SMALL_CASES, ids=[f'{"x".join(map(str, s))}-{"x".join(map(str, o))}-{"x".join(map(str, g))}'
                                                          for s, o, g in SMALL_CASES])
def test_small_and_odd_shapes(shape, out, gs, interp):
    src = data(47, shape)
    ms, g, planes, w = wc.small_case(shape, out, gs)
    vols, masks, kept = model(src, ms, g, planes, out, interp)
    assert masks.any()
    sv = handle(interp, src)
    try:
        for flags in FLAGS:
            got = sv.warp_stack(g, ms, out, w, planes=planes, _flags=flags)
            check_info(sv, ms, g, 3, out, interp, flags)
            check_entries(got, vols, kept, w, TOL[interp], (interp, shape, out, gs, flags))
    finally:
        sv.close()


# ---- 6. non-finite data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_non_finite_pixels_reach_their_stencils_only(interp):
    """Coordinates on the lattice (multiples of 0.1) + an offset + a displacement within 0.004 of a constant: nowhere within 1e-3 of an integer,
    so every tap of a stencil has a non-zero weight and the model's set of non-finite outputs is exact."""
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
    g[:, 0, 1] += np.float32(0.004)                                                      # a field that varies, by less than the clearance
    g[:, 1, 0] -= np.float32(0.004)
    planes = np.array([1, 1, 4, 4])
    w = np.array([1.0, -2.0, 0.5, 1.5])
    y = np.stack([np.stack(wsm.coords(ms[i], g[i], OUT)) for i in range(4)])
    assert np.abs(y - np.round(y)).min() > 1e-3
    vols, masks, kept = model(src, ms, g, planes, OUT, interp)
    bad = ~np.isfinite(vols)
    assert all(b.any() for b in bad) and not bad.all() and kept.all()
    sv = handle(interp, src)
    try:
        for flags in FLAGS:
            got = sv.warp_stack(g, ms, OUT, w, planes=planes, _flags=flags)
            assert np.array_equal(~np.isfinite(got), bad), (interp, flags, int((~np.isfinite(got) != bad).sum()))
            ok = ~bad
            err = np.abs(got.astype(np.float64) - w[:, None, None] * vols)[ok].max()
            assert err <= 2.0 * TOL[interp]                                              # max |w| = 2
    finally:
        sv.close()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    ms = wc.batch()
    m1 = np.ascontiguousarray(ms[:1], dtype=np.float32)
    g1 = np.ascontiguousarray(wc.grids((3, 5), 1.5)[:1])
    out = np.zeros((1,) + OUT, np.float32)
    p0 = np.zeros(1, np.int32)

    def call(h, n=1, mat=m1, grids=g1, n_grids=1, gdims=(3, 5), planes=p0, w=None, shape=OUT, flags=0, f64=False, o=out):
        fn = lib.vt_volume_warp_stack_f64 if f64 else lib.vt_volume_warp_stack
        mat = None if mat is None else np.ascontiguousarray(mat, dtype=np.float64 if f64 else np.float32)
        return fn(h, n, None if mat is None else mat.ctypes.data, None if grids is None else grids.ctypes.data, n_grids, *gdims,
                  None if planes is None else planes.ctypes.data, None if w is None else w.ctypes.data, *shape,
                  None if o is None else o.ctypes.data, flags)

    # filt_* without VT_STACK, in Python and by the library; VT_EDGE_SCIPY
    sv = vt.StaticVolume(data(), interpolation='filt_bspline', device='gpu:0')
    with pytest.raises(ValueError):
        sv.warp_stack(g1[0], ms, OUT, planes=PLANES)
    assert call(sv._handle) == VT_EUNSUPPORTED and b'VT_STACK' in lib.vt_last_error()
    assert call(sv._handle, f64=True) == VT_EUNSUPPORTED
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()
    sv = vt.StaticVolume(data(), device='gpu:0', edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    with pytest.raises(RuntimeError, match=f'code {VT_EUNSUPPORTED}'):
        sv.warp_stack(g1[0], ms, OUT, planes=PLANES)
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()

    sv = handle('bspline')
    hd = sv._handle
    want = sv.warp_stack(g1, m1, OUT, planes=[0]).copy()
    assert want.any()
    bad = m1.copy()
    bad[0, 1, 2] = np.nan
    assert call(hd, mat=bad) == VT_EINVAL and b'finite' in lib.vt_last_error()
    assert call(hd, mat=bad, f64=True) == VT_EINVAL
    for p in ([STACK[0]], [-1]):
        assert call(hd, planes=np.array(p, np.int32)) == VT_EINVAL and b'plane' in lib.vt_last_error()
    assert call(hd, planes=None) == VT_EINVAL and b'plane' in lib.vt_last_error()           # n = 1 != T
    assert call(hd, w=np.array([np.inf])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    for shape in ((0, 45), (37, -1)):
        assert call(hd, shape=shape) == VT_EINVAL
    assert call(hd, n=0) == VT_EINVAL and call(hd, n=-2) == VT_EINVAL
    # the refusals of this entry point
    for ng in (0, 2, -1):
        assert call(hd, n_grids=ng) == VT_EINVAL and b'grids' in lib.vt_last_error()
    for gd in ((0, 5), (3, 0), (3, 46), (38, 5), (-1, 5)):
        assert call(hd, gdims=gd) == VT_EINVAL and b'grid dims' in lib.vt_last_error(), gd
    for v in (np.nan, np.inf, -np.inf):
        gb = g1.copy()
        gb[0, 2, 4, 1] = v
        assert call(hd, grids=gb) == VT_EINVAL and b'node' in lib.vt_last_error()
        assert call(hd, grids=gb, f64=True) == VT_EINVAL
    assert call(hd, grids=None) == VT_EINVAL and b'NULL' in lib.vt_last_error()
    assert call(hd, o=None) == VT_EINVAL
    # the bounds, decided before anything is read: 2^29 images x 9 tiles; 2^27 grids x 15 nodes x 2
    assert call(hd, n=1 << 29) == VT_EUNSUPPORTED and b'grid too large' in lib.vt_last_error()
    assert call(hd, n=1 << 29, f64=True) == VT_EUNSUPPORTED
    assert call(hd, n=1 << 27, n_grids=1 << 27) == VT_EUNSUPPORTED and b'grids too large' in lib.vt_last_error()
    # the handle still answers; matrices == NULL is the identity; flags other than the routes' and VT_OUT_DEVICE are ignored
    _native.check(call(hd, flags=_native.KEEP_OUTSIDE | _native.ACCUMULATE), 'warp_stack')
    assert same_bits(out, want)
    _native.check(call(hd, f64=True), 'warp_stack_f64')
    assert same_bits(out, want)
    _native.check(call(hd, mat=None), 'warp_stack, NULL matrices')
    assert same_bits(out, sv.warp_stack(g1, np.eye(3)[None], OUT, planes=[0]))
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_chain_into_backprojection_stays_on_the_device(interp):
    """warp_stack -> a new handle on the device result -> backproject: the aligned series never visits the host."""
    sv = handle(interp)
    g = wc.grids((3, 5), 1.5, STACK[1:], STACK[0], 13)
    want = sv.warp_stack(g).copy()
    dev = vt.empty(STACK, device='gpu:0')
    assert sv.warp_stack(g, output=dev) is None
    sv.synchronize()
    sv.close()
    vol = (12, 20, 24)
    bp = vt.utils.backproject_matrices(np.linspace(-50.0, 50.0, 6), 1, vol, STACK)
    a = vt.StaticVolume(dev, interpolation='linear', device='gpu:0')
    b = vt.StaticVolume(want, interpolation='linear', device='gpu:0')
    assert same_bits(a.backproject(bp, vol), b.backproject(bp, vol))
    a.close()
    b.close()
