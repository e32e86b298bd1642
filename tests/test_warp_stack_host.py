"""StaticVolume.warp_stack without a GPU: the device='cpu' path against the float64 model of tests/warp_stack_model.py, the zero grid
against affine_stack, the model held to the cases of the GPU tests (tests/warp_stack_cases.py: the skirt condition, the plan
properties), utils.stack_grid_nodes, argument errors, library codes and symbols."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import backproject_model as bm
import warp_stack_cases as wc
import warp_stack_model as wsm
from test_stack_affine_host import MARGIN, INTERPS, STACK, OUT, PLANES, WTS, N, VT_EINVAL, cpu_bound, embed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = ((2, 2), (3, 5), (1, 4), 'dense')
AMP = 1.5


@pytest.fixture(scope='module')
def stack():
    s = np.random.RandomState(11).random_sample(STACK).astype(np.float32)
    s.setflags(write=False)
    return s


def batch():
    """Ten float64 (3, 3) matrices onto OUT whose footprints, grown by the 1.5 pixels a grid can add, stay MARGIN['filt_bspline'] = 14
    pixels inside the (64, 72) images but for their corners: the output centre goes to the image centre plus a shift of at most 2 pixels,
    turned by at most 8 degrees and never magnified (scale >= 1 shrinks the footprint)."""
    return vt.utils.stack_matrices(shifts=[[0.5, -1.25], [0.0, 2.0], [1.0, -2.0], [0.375, 0.625], [0.0, 0.0], [-1.5, 0.25], [2.0, 1.0], [-1.0, 0.5],
                                           [0.0, -1.5], [1.25, 1.25]],
                                   rotations=[8.0, -6.0, 0.0, 0.0, 3.0, 0.0, -4.5, 5.0, -8.0, 7.5],
                                   scales=[1.0, 1.1, 1.0, 1.0, 1.05, 1.0, 1.2, 1.0, 1.15, 1.0], image_shape=STACK, output_shape=OUT)


def host_grids(gs, shared, seed=3):
    g = OUT if gs == 'dense' else gs
    rs = np.random.RandomState(seed)
    a = ((rs.random_sample((N,) + g + (2,)) * 2.0 - 1.0) * AMP).astype(np.float32)
    return a[0] if shared else a


def model_m4(m3):
    m4 = np.zeros((len(m3), 4, 4))
    m4[:, 0, 0] = 1
    m4[:, 1:, 1:] = np.asarray(m3, np.float64)
    return m4


# ---- the CPU device path against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
def test_cpu_device_path_against_the_model(interp, stack):
    ms = batch()
    H, W = STACK[1:]
    k = MARGIN[interp]
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    for gs in GRIDS:
        for shared in (False, True):
            g = host_grids(gs, shared)
            assert np.abs(g).max() <= AMP
            for mats in (ms, ms.astype(np.float32)):
                m4 = model_m4(mats)
                vols, _, _ = wsm.warp_stack(stack, m4, g, PLANES, OUT, interp)
                got = sv.warp_stack(g, mats, OUT, WTS, planes=PLANES)
                assert got.dtype == np.float32 and got.shape == (N,) + OUT
                kept = 0
                for i in range(N):
                    y, x = wsm.coords(m4[i], wsm.grid_of(g, i), OUT)
                    keep = (y >= k) & (y <= H - 1 - k) & (x >= k) & (x <= W - 1 - k)
                    kept += int(keep.sum())
                    err = float(np.abs(got[i].astype(np.float64) - WTS[i] * vols[i])[keep].max()) if keep.any() else 0.0
                    bound = cpu_bound(interp, WTS[i], stack)
                    print(f'{interp} {gs} shared={shared} {mats.dtype} entry {i}: kept {int(keep.sum())}/{keep.size}  '
                          f'max|cpu - model| {err:.3e}  bound {bound:.3e}')
                    assert err <= bound, (interp, gs, shared, i, err, bound)
                assert kept >= 0.9 * N * OUT[0] * OUT[1], (gs, shared, kept)
    # the (n, 4, 4) form with junk in row 0 and column 0 gives the same bits; a shared grid is n copies of it
    g = host_grids((3, 5), False)
    assert np.array_equal(sv.warp_stack(g, embed(ms), OUT, WTS, planes=PLANES), sv.warp_stack(g, ms, OUT, WTS, planes=PLANES))
    assert np.array_equal(sv.warp_stack(g[0], ms, OUT, WTS, planes=PLANES), sv.warp_stack(np.tile(g[:1], (N, 1, 1, 1)), ms, OUT, WTS, planes=PLANES))
    # n from the grids, then from T; output=; the default output shape
    assert sv.warp_stack(g[:5], output_shape=OUT).shape == (5,) + OUT
    assert sv.warp_stack(g[0]).shape == STACK
    out = np.full((N,) + OUT, 7, np.float32)
    assert sv.warp_stack(g, ms, OUT, WTS, output=out, planes=PLANES) is out
    assert np.array_equal(out, sv.warp_stack(g, ms, OUT, WTS, planes=PLANES))


@pytest.mark.parametrize('interp', INTERPS)
def test_zero_grid_is_affine_stack(interp, stack):
    ms = batch()
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    want = sv.affine_stack(ms, OUT, WTS, planes=PLANES)
    for g in (np.zeros((2, 2, 2)), np.zeros((N, 3, 5, 2)), np.zeros((1, 1, 2)), np.zeros(OUT + (2,))):
        got = sv.warp_stack(g, ms, OUT, WTS, planes=PLANES)
        assert float(np.abs(got.astype(np.float64) - want).max()) <= 1e-6
    ident = sv.warp_stack(np.zeros((2, 2, 2)))
    assert float(np.abs(ident.astype(np.float64) - sv.affine_stack(np.tile(np.eye(3), (STACK[0], 1, 1)))).max()) <= 1e-6


# ---- the model on the cases of the GPU tests ---------------------------------------------------------------------------------------
def all_gpu_cases():
    for name, out, ms, g in wc.parity_cases():
        yield name, out, ms, g, (wc.PLANES if ms is not None else None)
    for name, (ms, g, planes, _) in wc.route_cases().items():
        yield name, wc.OUT, ms, g, planes
    ms, g, planes, _ = wc.pushed_out_case()
    yield 'pushed out', wc.OUT, ms, g, planes
    for shape, out, gs in wc.SMALL_CASES:
        ms, g, planes, _ = wc.small_case(shape, out, gs)
        yield f'small {shape} {out} {gs}', out, ms, g, planes, shape


def test_skirt_condition_of_the_gpu_cases():
    """Within SKIRT_EPS of a skirt face float64 rounding may decide a pixel's inside test either way; the GPU tests leave those pixels
    out, and this holds their share to 0.001 per case before any GPU run.  The exact lattice case leaves none out."""
    for name, out, ms, g, planes, *shape in all_gpu_cases():
        src = np.zeros(shape[0] if shape else wc.STACK, np.float32)
        for f32 in (False, True):
            mm = ms if ms is None or not f32 else ms.astype(np.float32).astype(np.float64)
            _, _, dist = wsm.warp_stack(src, mm, g, planes, out, 'linear')
            share = wsm.skirt_share(dist)
            print(f'{name} f32={f32}: share within {wsm.SKIRT_EPS} of a face {share:.5f}')
            assert share <= 0.001, (name, f32, share)
    ms, g, folded, planes = wc.lattice_case()
    for out in (wc.OUT, wc.OUT32):
        y, x = zip(*[wsm.coords(ms[i], g[i], out) for i in range(len(ms))])
        fy, fx = zip(*[wsm.affine_coords(folded[i], out) for i in range(len(ms))])
        assert np.array_equal(np.stack(y), np.stack(fy)) and np.array_equal(np.stack(x), np.stack(fx))      # exact: nothing to leave out
        on_face = (np.stack(y) == -0.5) | (np.stack(y) == wc.STACK[1] - 0.5) | (np.stack(x) == -0.5) | (np.stack(x) == wc.STACK[2] - 0.5)
        on_lattice = (np.stack(y) == np.floor(np.stack(y))) & (np.stack(x) == np.floor(np.stack(x)))
        assert on_face.any() and on_lattice.any()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_plan_properties(interp):
    for name, out, ms, g, planes, *shape in all_gpu_cases():
        n = len(ms) if ms is not None else len(g)
        p = wsm.plan(ms, g, n, out, interp)
        T = p.tile
        assert out not in wc.TILE or (1,) + tuple(T) == wc.TILE[out], (name, T)
        assert (p.nodes[..., 0] * p.nodes[..., 1]).max() <= (T[0] + 1) * (T[1] + 1) and 4 * p.node_floats <= 8720
        # a tile that passes the cap fits the allocation
        bytes_ = 4 * p.dims[..., 0] * p.dims[..., 1]
        assert bytes_.max() <= p.patch_bytes <= wsm.PATCH_CAP, (name, int(bytes_.max()), p.patch_bytes)
        assert p.lds_bytes == 128 + 4 * p.node_floats + p.patch_bytes
        # every tap of a staged tile lies in its patch
        assert wsm.violations(p, ms, g, out, interp) == [], name
        d = wsm.plan(ms, g, n, out, interp, force_direct=True)
        assert not d.staged.any() and d.lds_dims == (0, 0, 0) and d.lds_bytes == 128 + 4 * d.node_floats
    routes = wc.route_cases()
    ms, g, planes, _ = routes['spike']
    p = wsm.plan(ms, g, 3, wc.OUT, interp)
    assert p.staged[0].all() and p.staged[2].all() and p.flag.all()
    assert not p.staged[1].any() and p.hull[1].all()                       # the spike's tiles exceed the cap, not the hull limit
    assert p.lds_dims == wsm.CAP_DIMS and p.patch_bytes == wsm.PATCH_CAP
    ms, g, planes, _ = routes['hull']
    p = wsm.plan(ms, g, 1, wc.OUT, interp)
    assert p.flag.all() and not p.hull.any() and not p.staged.any()
    for key in ('extent', 'chain'):
        ms, g, planes, _ = routes[key]
        p = wsm.plan(ms, g, 1, wc.OUT, interp)
        assert not p.flag.any() and not p.staged.any() and p.lds_dims == (0, 0, 0) and p.patch_bytes == 0, key
    ms, g, planes, _ = wc.pushed_out_case()
    p = wsm.plan(ms, g, 1, wc.OUT, interp)
    what = wsm.tile_outcome(p, ms, wc.STACK[1:])
    assert (what[0, :, 2] == 'zero').all() and (what[0, :, 0] != 'zero').all(), what


# ---- stack_grid_nodes ------------------------------------------------------------------------------------------------------------
def test_stack_grid_nodes_by_definition():
    nodes = vt.utils.stack_grid_nodes((3, 5), (37, 45))
    assert nodes.shape == (3, 5, 2) and nodes.dtype == np.float64
    for j in range(3):
        for k in range(5):
            assert np.array_equal(nodes[j, k], [j * 36 / 2, k * 44 / 4])
    assert np.array_equal(nodes[0, 0], [0, 0]) and np.array_equal(nodes[-1, -1], [36, 44])
    one = vt.utils.stack_grid_nodes((1, 4), (37, 45))
    assert one.shape == (1, 4, 2) and np.array_equal(one[0, :, 0], [18.0] * 4) and np.array_equal(one[0, :, 1], np.arange(4) * 44 / 3)
    assert np.array_equal(vt.utils.stack_grid_nodes((1, 1), (1, 1)), np.zeros((1, 1, 2)))
    assert np.array_equal(vt.utils.stack_grid_nodes((37, 45), (37, 45))[..., 1], np.broadcast_to(np.arange(45.0), (37, 45)))
    assert np.array_equal(nodes, vt.utils.grid_nodes((1, 3, 5), (1, 37, 45))[0, :, :, 1:])
    for bad in (((3, 5, 2), (37, 45)), ((3,), (37, 45)), ((3, 46), (37, 45)), ((0, 5), (37, 45)), (5, (37, 45)), ((3, 5), (37, 45, 1)),
                ((3.0, 5), (37, 45))):
        with pytest.raises(ValueError):
            vt.utils.stack_grid_nodes(*bad)


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors(stack):
    sv = vt.StaticVolume(stack, device='cpu')
    ms = batch()
    g = host_grids((3, 5), False)
    for bad in (np.zeros((3, 5)), np.zeros((3, 5, 3)), np.zeros((N, 3, 5, 3)), np.zeros((2, N, 3, 5, 2)), np.zeros((N, 0, 5, 2)),
                np.zeros((N, 3, 25, 2)), np.zeros((N, 21, 5, 2)), np.zeros((4, 3, 5, 2))):
        with pytest.raises(ValueError):
            sv.warp_stack(bad, ms, OUT, planes=PLANES)
    for bad in (np.nan, np.inf):
        gg = g.copy()
        gg[3, 1, 2, 0] = bad
        with pytest.raises(ValueError):
            sv.warp_stack(gg, ms, OUT, planes=PLANES)
        w = WTS.copy()
        w[2] = bad
        with pytest.raises(ValueError):
            sv.warp_stack(g, ms, OUT, w, planes=PLANES)
    for bad in (np.eye(3), np.zeros((0, 3, 3)), np.zeros((2, 3, 4)), np.zeros((2, 5, 5))):
        with pytest.raises(ValueError):
            sv.warp_stack(g[0], bad, OUT, planes=[0] * len(bad))
    with pytest.raises(ValueError):
        sv.warp_stack(g, ms, OUT, WTS[:4], planes=PLANES)
    with pytest.raises(ValueError):
        sv.warp_stack(g, ms, OUT)                                                           # planes=None with n = 10 != T = 5
    with pytest.raises(ValueError):
        sv.warp_stack(g, None, OUT)                                                         # n from the grids: 10 != T
    for bad in ([0, 1, 2, 3, 4, 5, 0, 0, 0, 0], [0, 1, 2, 3, 4, -1, 0, 0, 0, 0], [0, 1, 2, 3], [[0, 1, 2, 3, 4, 0, 0, 0, 0, 0]]):
        with pytest.raises(ValueError):
            sv.warp_stack(g, ms, OUT, planes=bad)
    for bad in (np.zeros((N, 20, 25), np.float32), np.zeros((5,) + OUT, np.float32), np.zeros(OUT, np.float32)):
        with pytest.raises(ValueError):
            sv.warp_stack(g, ms, OUT, output=bad, planes=PLANES)
    for shape in ((0, 12), (6, 8, 12), (6, 8.0), (6,), 5):
        with pytest.raises(ValueError):
            sv.warp_stack(g[0, :1, :1], ms, shape, planes=PLANES)
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, 'filt_bspline', 'cpu').warp_stack(g, ms, OUT, planes=PLANES)


# ---- the library without a GPU ---------------------------------------------------------------------------------------------------
def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    g = np.zeros((1, 2, 2, 2), np.float32)
    w = np.ones(1)
    pl = np.zeros(1, np.int32)
    out = np.zeros((1, 4, 4), np.float32)
    assert lib.vt_volume_warp_stack(None, 1, m32.ctypes.data, g.ctypes.data, 1, 2, 2, pl.ctypes.data, w.ctypes.data, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_warp_stack_f64(None, 1, m64.ctypes.data, g.ctypes.data, 1, 2, 2, pl.ctypes.data, w.ctypes.data, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_warp_stack_f64(None, 1, None, g.ctypes.data, 1, 2, 2, None, None, 4, 4, out.ctypes.data, _native.FORCE_DIRECT) == VT_EINVAL
    assert b'NULL' in lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_warp_stack', 'vt_volume_warp_stack_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 13
    assert '22 per-image displacement grids of a stack' in header                  # the last_kernel comment names the new kernel
    assert 'stack_grid_nodes' in dir(vt.utils)
