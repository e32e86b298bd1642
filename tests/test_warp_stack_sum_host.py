"""StaticVolume.warp_stack_sum / motion_corrected_sum without a GPU: the device='cpu' path against the float64 ascending sum of its own
warp_stack(weights=None) images (bit for bit, every pixel), the forms of `weights`, halves, shifts, accumulate, argument errors, the
model of tests/warp_stack_sum_model.py held to the cases of the GPU tests (plan properties, the skirt condition), library codes and
symbols."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import warp_stack_cases as wc
import warp_stack_model as wsm
import warp_stack_sum_cases as sc
import warp_stack_sum_model as ssm
from test_stack_affine_host import INTERPS, STACK, OUT, PLANES, N, VT_EINVAL
from test_warp_stack_host import batch, host_grids, all_gpu_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def stack():
    s = np.random.RandomState(11).random_sample(STACK).astype(np.float32)
    s.setflags(write=False)
    return s


def host_loop(images, W, start=None):
    """float32(acc) of acc = b; acc = acc + W[i, c] * double(S_i), i ascending."""
    return ssm.two_rounding_sum(images.astype(np.float64), W, start).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the CPU path is the float64 ascending sum of its own images -------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
def test_cpu_path_is_the_ascending_sum_of_its_own_images(interp, stack):
    assert N == sc.N
    ms = batch()
    names, W = sc.first(9)
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    for gs in ((3, 5), 'dense'):
        for shared in (False, True):
            g = host_grids(gs, shared)
            for mats in (ms, ms.astype(np.float32)):
                S = sv.warp_stack(g, mats, OUT, planes=PLANES)
                assert S.any()
                got = sv.warp_stack_sum(g, mats, OUT, W, planes=PLANES)
                assert got.dtype == np.float32 and got.shape == (9,) + OUT
                want = host_loop(S, W)
                assert np.array_equal(bits(got), bits(want)), (interp, gs, shared, mats.dtype, int((bits(got) != bits(want)).sum()))
                assert not bits(got[names.index('zero')]).any()
    # matrices=None: n from the grids, then from T
    g = host_grids((3, 5), False)[:STACK[0]]
    assert np.array_equal(sv.warp_stack_sum(g), host_loop(sv.warp_stack(g), None)[0])
    assert np.array_equal(sv.warp_stack_sum(g[0]), host_loop(sv.warp_stack(g[0]), None)[0])


def test_forms_of_weights(stack):
    ms = batch()
    g = host_grids((3, 5), False)
    sv = vt.StaticVolume(stack, device='cpu')
    none = sv.warp_stack_sum(g, ms, OUT, planes=PLANES)
    assert none.shape == OUT
    assert np.array_equal(bits(none), bits(sv.warp_stack_sum(g, ms, OUT, np.ones(N), planes=PLANES)))
    w = np.array(wc.WEIGHTS)
    flat = sv.warp_stack_sum(g, ms, OUT, w, planes=PLANES)
    col = sv.warp_stack_sum(g, ms, OUT, w[:, None], planes=PLANES)
    assert flat.shape == OUT and col.shape == (1,) + OUT and np.array_equal(bits(flat), bits(col[0]))
    # a column does not depend on the others
    for names, W in sc.placements():
        got = sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES)
        alone = sv.warp_stack_sum(g, ms, OUT, sc.COLUMNS[names[1]], planes=PLANES)
        assert np.array_equal(bits(got[1]), bits(alone)), names
        if 'mixed' in names:
            assert np.array_equal(bits(got[names.index('mixed')]), bits(flat)), names


def test_halves_and_shifts(stack):
    T = STACK[0]
    g = host_grids((3, 5), False)[:T]
    sv = vt.StaticVolume(stack, device='cpu')
    h = sv.motion_corrected_sum(g, halves=True)
    assert h.shape == (3,) + STACK[1:]
    even, odd = np.zeros(T), np.zeros(T)
    even[0::2] = 1
    odd[1::2] = 1
    for c, w in enumerate((np.ones(T), even, odd)):
        assert np.array_equal(bits(h[c]), bits(sv.warp_stack_sum(g, weights=w))), c
    assert np.array_equal(bits(sv.motion_corrected_sum(g)), bits(h[0]))
    # whole-frame shifts: the matrices align_stack builds
    shifts = np.array([[0.5, -1.25], [0.0, 2.0], [1.0, -2.0], [0.375, 0.625], [-1.5, 0.25]])[:T]
    ms = vt.utils.stack_matrices(shifts, None, None, STACK[1:], OUT)
    got = sv.motion_corrected_sum(g, shifts, output_shape=OUT)
    assert got.shape == OUT and got.any()
    assert np.array_equal(bits(got), bits(sv.warp_stack_sum(g, ms, OUT)))
    # no local motion: one zero node, the sum of align_stack's images
    plain = sv.motion_corrected_sum(shifts=shifts, output_shape=OUT)
    want = host_loop(sv.align_stack(shifts, output_shape=OUT), None)[0]
    assert float(np.abs(plain.astype(np.float64) - want).max()) <= 1e-5
    with pytest.raises(ValueError):
        sv.motion_corrected_sum(g, weights=np.ones(T))
    assert sv.motion_corrected_sum(g).shape == STACK[1:]


def test_accumulate_on_the_cpu_path(stack):
    ms = batch()
    g = host_grids((3, 5), False)
    names, W = sc.first(5)
    sv = vt.StaticVolume(stack, device='cpu')
    S = sv.warp_stack(g, ms, OUT, planes=PLANES)
    out = sv.warp_stack_sum(g[:5], ms[:5], OUT, W[:5], planes=PLANES[:5])
    first = out.copy()
    assert sv.warp_stack_sum(g[5:], ms[5:], OUT, W[5:], output=out, planes=PLANES[5:], accumulate=True) is out
    want = host_loop(S[5:], W[5:], start=first.astype(np.float64))
    assert np.array_equal(bits(out), bits(want))
    with pytest.raises(ValueError):
        sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES, accumulate=True)                    # nothing to add into


# ---- argument errors, each followed by a good call ------------------------------------------------------------------------------------
def test_argument_errors_each_followed_by_a_good_call(stack):
    sv = vt.StaticVolume(stack, device='cpu')
    ms = batch()
    g = host_grids((3, 5), False)
    names, W = sc.first(5)
    want = sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES)

    def refused(*a, **kw):
        with pytest.raises(ValueError):
            sv.warp_stack_sum(*a, **kw)
        assert np.array_equal(bits(sv.warp_stack_sum(g, ms, OUT, W, planes=PLANES)), bits(want))

    for bad in (np.zeros((3, 5)), np.zeros((3, 5, 3)), np.zeros((N, 3, 5, 3)), np.zeros((N, 0, 5, 2)), np.zeros((N, 3, 25, 2)),
                np.zeros((4, 3, 5, 2))):
        refused(bad, ms, OUT, W, planes=PLANES)
    for bad in (np.nan, np.inf):
        gg = g.copy()
        gg[3, 1, 2, 0] = bad
        refused(gg, ms, OUT, W, planes=PLANES)
        w = W.copy()
        w[2, 3] = bad
        refused(g, ms, OUT, w, planes=PLANES)
    for bad in (np.eye(3), np.zeros((0, 3, 3)), np.zeros((2, 3, 4))):
        refused(g[0], bad, OUT, planes=[0] * len(bad))
    for bad in (W[:4], W.T, np.ones((N, 0)), np.ones((N, 2, 2)), np.ones(N - 1), np.float64(1.0)):
        refused(g, ms, OUT, bad, planes=PLANES)
    refused(g, ms, OUT, W)                                                                   # planes=None with n = 10 != T
    for bad in ([0, 1, 2, 3, 4, 5, 0, 0, 0, 0], [0, 1, 2, 3, 4, -1, 0, 0, 0, 0], [0, 1, 2, 3]):
        refused(g, ms, OUT, W, planes=bad)
    for bad in (np.zeros((N,) + OUT, np.float32), np.zeros(OUT, np.float32), np.zeros((4,) + OUT, np.float32)):
        refused(g, ms, OUT, W, output=bad, planes=PLANES)
    refused(g, ms, OUT, np.ones(N), output=np.zeros((1,) + OUT, np.float32), planes=PLANES)   # (n,) weights: the result is (Ho, Wo)
    for shape in ((0, 12), (6, 8, 12), (6, 8.0), 5):
        refused(g[0, :1, :1], ms, shape, W, planes=PLANES)
    refused(g, ms, OUT, W, planes=PLANES, accumulate=True)
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, 'filt_bspline', 'cpu').warp_stack_sum(g, ms, OUT, W, planes=PLANES)


# ---- the model on the cases of the GPU tests ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_plan_properties(interp):
    for name, out, ms, g, planes, *shape in all_gpu_cases():
        n = len(ms) if ms is not None else len(g)
        for grids in (g, g[0]):
            for G in sc.G_VALUES:
                p = ssm.plan(ms, grids, n, out, interp, G)
                # the allocation holds every tile's patch, twice; the launch stays within what a workgroup may have
                bytes_ = 4 * p.dims[..., 0] * p.dims[..., 1]
                assert bytes_.max() <= p.patch_bytes <= wsm.PATCH_CAP, (name, int(bytes_.max()), p.patch_bytes)
                assert p.node_blocks == (1 if grids.ndim == 3 or n == 1 else 3)
                assert p.sum_lds_bytes == 4 * p.node_blocks * p.node_floats + 2 * p.patch_bytes <= ssm.LDS_LIMIT, (name, p.sum_lds_bytes)
                assert p.sum_grid == -(-G // sc.GC) * p.nT[0] * p.nT[1]
                assert p.sum_lds_dims == ((2,) + tuple(p.lds_dims[1:]) if p.patch_bytes else (0, 0, 0))
        d = ssm.plan(ms, g, n, out, interp, 3, force_direct=True)
        assert not d.staged.any() and d.sum_lds_dims == (0, 0, 0) and d.sum_lds_bytes == 4 * d.node_blocks * d.node_floats
    # the largest launch there can be: a dense grid on the 32 x 32 tile, the allocation at the cap
    assert 4 * 3 * ((2 * 33 * 33 + 3) & ~3) + 2 * wsm.PATCH_CAP <= ssm.LDS_LIMIT


def test_passed_over_entries():
    names, W = sc.first(9)
    po = ssm.passed_over(W, sc.N)
    assert po.shape == (3, sc.N)
    # chunk 0 = (ones, mixed, zero, hot_inside): nothing is passed over; chunk 1 = (hot_outside, hot_last, even, odd): nothing either
    assert not po[0].any() and not po[1].any() and not po[2].any()
    only = ssm.passed_over(sc.matrix(('zero', 'hot_inside', 'hot_last')), sc.N)
    assert only.shape == (1, sc.N) and [i for i in range(sc.N) if not only[0, i]] == [sc.INSIDE, sc.LAST]
    assert ssm.passed_over(sc.matrix(('zero',)), sc.N).all()
    assert not ssm.passed_over(None, 3).any()


def test_skirt_condition_of_the_parity_cases():
    """No output pixel of the parity cases lies within SKIRT_EPS of a skirt face in any entry, so the GPU parity test compares every
    pixel of a sum (it asserts a kept share of at least 0.999)."""
    from test_gpu_extract import rand_vol
    src = rand_vol(wc.STACK, 41)
    for name, out, ms, g in wc.parity_cases():
        planes = wc.PLANES if ms is not None else None
        for f32 in (False, True):
            mm = ms if ms is None or not f32 else ms.astype(np.float32).astype(np.float64)
            _, kept = ssm.warp_stack_sum(src, mm, g, planes, out, 'linear')
            share = 1.0 - float(kept.mean())
            print(f'{name} f32={f32}: share of output pixels within {wsm.SKIRT_EPS} of a face in some entry {share:.5f}')
            assert share == 0.0, (name, f32, share)


# ---- the library without a GPU ---------------------------------------------------------------------------------------------------
def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    g = np.zeros((1, 2, 2, 2), np.float32)
    w = np.ones(2)
    pl = np.zeros(1, np.int32)
    out = np.zeros((2, 4, 4), np.float32)
    assert lib.vt_volume_warp_stack_sum(None, 1, m32.ctypes.data, g.ctypes.data, 1, 2, 2, pl.ctypes.data, 2, w.ctypes.data, 4, 4,
                                        out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_warp_stack_sum_f64(None, 1, m64.ctypes.data, g.ctypes.data, 1, 2, 2, pl.ctypes.data, 2, w.ctypes.data, 4, 4,
                                            out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_warp_stack_sum_f64(None, 1, None, g.ctypes.data, 1, 2, 2, None, 1, None, 4, 4, out.ctypes.data,
                                            _native.FORCE_DIRECT) == VT_EINVAL
    assert b'NULL' in lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_warp_stack_sum', 'vt_volume_warp_stack_sum_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 14
    assert '26 the images of kind 22 summed' in header                             # the last_kernel comment names the new kernel
    assert callable(vt.StaticVolume.warp_stack_sum) and callable(vt.StaticVolume.motion_corrected_sum)
