"""-m gpu: StaticVolume.warp (vt_volume_warp, kernel 20).  Affine fields against the oracle of `extract` on every voxel; fields that are
not affine against the float64 model of tests/warp_model.py, its plan included; the two routes of a tile against each other; independence
of output kind, history and handle; edge='scipy' against scipy's map_coordinates; refusals."""
import ctypes

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle

import warp_cases as wc
import warp_model as wm
from test_gpu_extract import TOL
from test_gpu_edge_scipy import TOL as TOL_EDGE

pytestmark = pytest.mark.gpu

VT_EINVAL, VT_EUNSUPPORTED = 10001, 10004
SKIRT_EPS = 1e-9
NON_NEGATIVE = ('linear', 'bspline', 'bspline_simple')


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits_up_to_zero_sign(a, b):
    return np.array_equal(a, b) and bool(((bits(a) == bits(b)) | ((a == 0) & (b == 0))).all())


@pytest.fixture(scope='module')
def volumes():
    """One handle per interpolation for the whole file (the source never changes)."""
    svs = {interp: vt.StaticVolume(wc.source_volume(), interpolation=interp, device='gpu:0') for interp in wc.INTERPS}
    yield svs
    for sv in svs.values():
        sv.close()


# ---- oracle: affine fields ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', wc.INTERPS)
@pytest.mark.parametrize('case', wc.affine_field_cases(), ids=lambda c: c[0])
def test_affine_fields_against_the_oracle(case, interp, volumes):
    name, out_shape, grid, B, c = case
    sv = volumes[interp]
    vol = wc.source_volume()
    src = oracle.prefilter(vol) if interp.startswith('filt') else vol
    okind = interp[5:] if interp.startswith('filt') else interp
    m64 = wc.rotated(out_shape)
    for m in (m64, m64.astype(np.float32)):
        total = wc.combined(m.astype(np.float64), B, c)
        dist = float(wm.skirt_distance(wm.affine_coords(total, out_shape), wc.SRC).min())
        assert dist > SKIRT_EPS, (name, dist)                                # no voxel to leave out, by construction
        want = oracle.affine_ex(src, total, okind, out_shape)
        assert want.any()
        routes = {}
        for flags in (0, _native.FORCE_DIRECT):
            got = routes[flags] = sv.warp(grid, m, out_shape, _flags=flags)
            info = sv.info()
            assert info.last_kernel == 20 and got.shape == out_shape and got.dtype == np.float32
            err = float(np.abs(got.astype(np.float64) - want).max())
            print(name, interp, m.dtype, flags, 'max|hip - oracle|', err)
            assert np.isfinite(got).all() and err <= TOL[interp], (name, interp, m.dtype, flags, err)
        if interp == 'linear':
            assert same_bits_up_to_zero_sign(routes[0], routes[_native.FORCE_DIRECT]), (name, m.dtype)


# ---- model: fields that are not affine ------------------------------------------------------------------------------------------
def compare_with_model(got, name, interp, what):
    vals, ins, s, _ = wc.model_result(name, interp)
    keep = wm.skirt_distance(s, wc.SRC) > SKIRT_EPS
    assert (~keep).sum() <= 0.001 * keep.size, (what, int((~keep).sum()))
    err = float(np.abs(got.astype(np.float64) - vals)[keep].max())
    print(what, 'max|hip - model|', err, 'left out', int((~keep).sum()), 'inside', int(ins.sum()))
    assert np.isfinite(got).all() and err <= TOL[interp], (what, err)
    outside = keep & ~ins
    assert np.array_equal(bits(got)[outside], np.zeros(int(outside.sum()), np.uint32)), what       # exact +0
    if interp in NON_NEGATIVE:
        assert np.array_equal((got != 0)[keep], ins[keep]), what


@pytest.mark.parametrize('interp', wc.INTERPS)
@pytest.mark.parametrize('name', list(wc.field_cases()))
def test_fields_against_the_model_on_both_routes(name, interp, volumes):
    out_shape, grid, m = wc.field_cases()[name]
    p = wc.model_result(name, interp)[3]
    sv = volumes[interp]
    got = sv.warp(grid, m, out_shape)
    info = sv.info()
    assert info.last_kernel == 20 and info.last_grid == int(np.prod(p.nT)) and tuple(info.last_tile) == tuple(p.tile)
    assert tuple(info.last_lds_dims) == tuple(p.lds_dims) and info.last_lds_bytes == p.lds_bytes <= 160 * 1024
    compare_with_model(got, name, interp, (name, interp, 'default'))
    direct = sv.warp(grid, m, out_shape, _flags=_native.FORCE_DIRECT)
    info = sv.info()
    assert info.last_kernel == 20 and tuple(info.last_lds_dims) == (0, 0, 0) and info.last_lds_bytes <= 160 * 1024
    if interp == 'linear':
        assert same_bits_up_to_zero_sign(got, direct), name
    else:
        compare_with_model(direct, name, interp, (name, interp, 'direct'))
    assert np.array_equal(bits(got), bits(sv.warp(grid, m, out_shape, _flags=_native.FORCE_TILED)))      # no effect beyond the default
    what = wm.tile_outcome(p, m, wc.SRC)
    if name == 'spike200':
        assert (what == 'direct').any() and (what == 'stage').any()
    if name == 'pushed_out':
        assert (what == 'zero').any() and not got[:, :, :8].any()


# ---- independence ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_output_kind_history_and_handle_do_not_show(interp, volumes):
    out_shape, grid, m = wc.field_cases()['g467_a12']
    sv = volumes[interp]
    fresh = sv.warp(grid, m, out_shape)
    assert np.array_equal(bits(fresh), bits(sv.warp(grid, m, out_shape)))                    # a repeated call
    host = np.full(out_shape, 5, np.float32)
    assert sv.warp(grid, m, out_shape, output=host) is None
    dev = vt.empty(out_shape, device='gpu:0')
    assert sv.warp(grid, m, out_shape, output=dev) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(host)) and np.array_equal(bits(fresh), bits(dev.get()))
    torch = pytest.importorskip('torch')
    tens = torch.full(out_shape, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.warp(grid, m, out_shape, output=tens) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    # the scratch of the batched calls is shared: other entry points in between
    ms = np.stack([wc.rotated((8, 8, 8)), wc.rotated((8, 8, 8), (30.0, 1.0, 2.0))])
    sv.extract(ms, (8, 8, 8))
    sv.place(ms, (12, 12, 12))
    sv.projection_batch(np.stack([wc.rotated(wc.SRC)] * 2))
    assert np.array_equal(bits(fresh), bits(sv.warp(grid, m, out_shape)))
    other = vt.StaticVolume(wc.source_volume(), interpolation=interp, device='gpu:0')           # a fresh handle
    assert np.array_equal(bits(fresh), bits(other.warp(grid, m, out_shape)))
    # a float64 grid is rounded once on the host; the default shape is the volume's, the default matrix the identity
    assert np.array_equal(bits(fresh), bits(other.warp(grid.astype(np.float64), m, out_shape)))
    zero = np.zeros((1, 1, 1, 3), np.float32)
    assert np.array_equal(bits(other.warp(zero)), bits(other.warp(zero, np.eye(4), wc.SRC)))
    if interp == 'linear':
        assert np.array_equal(other.warp(zero), wc.source_volume())
    other.close()


# ---- edge='scipy' ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_edge_scipy_handle_equals_the_cpu_path(interp):
    out_shape = wc.OUT_C
    n = wc.nodes((5, 6, 7), out_shape) / np.asarray(out_shape, np.float64)
    grid = (3.0 * np.stack([np.sin(2.0 * n[..., 1] + n[..., 2]), np.cos(3.0 * n[..., 0] - n[..., 2]), np.sin(1.0 + 2.5 * n[..., 0] * n[..., 1])],
                           axis=-1)).astype(np.float32)
    assert 2.0 < np.abs(grid).max() <= 3.0
    m = wc.rotated(out_shape, (6.0, -9.0, 4.0), scale=1.3)                    # the output reaches past the volume's faces
    vol = wc.source_volume()
    want = vt.StaticVolume(vol, interpolation=interp, device='cpu').warp(grid, m, out_shape)
    assert want.any() and not want.all()
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', edge='scipy')
    for flags in (0, _native.FORCE_DIRECT):
        got = sv.warp(grid, m, out_shape, _flags=flags)
        err = float(np.abs(got.astype(np.float64) - want).max())
        print(interp, flags, 'max|hip(edge=scipy) - cpu|', err)
        assert sv.info().last_kernel == 20 and err <= TOL_EDGE[interp], (interp, flags, err)
    sv.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(volumes):
    sv = volumes['linear']
    lib = _native.load()
    out_shape, grid, m = wc.field_cases()['g222_a1.5']
    good = sv.warp(grid, m, out_shape)
    out = np.zeros(out_shape, np.float32)
    m64 = np.ascontiguousarray(m)

    def call(g, gd, mat=m64, o=out):
        return lib.vt_volume_warp_f64(sv._handle, mat.ctypes.data, g.ctypes.data, *gd, *out_shape, o.ctypes.data, 0)

    def still_good():
        assert np.array_equal(bits(good), bits(sv.warp(grid, m, out_shape)))

    big = np.zeros((11, 2, 2, 3), np.float32)
    assert call(big, (11, 2, 2)) == VT_EINVAL and b'grid dims' in lib.vt_last_error()         # g_k > o_k
    still_good()
    assert call(grid, (2, 0, 2)) == VT_EINVAL and b'grid dims' in lib.vt_last_error()         # g_k == 0
    still_good()
    with pytest.raises(ValueError):
        sv.warp(big, m, out_shape)
    nan_grid = grid.copy()
    nan_grid[1, 0, 1, 2] = np.nan
    assert call(nan_grid, (2, 2, 2)) == VT_EINVAL and b'not finite' in lib.vt_last_error()
    with pytest.raises(RuntimeError):
        sv.warp(nan_grid, m, out_shape)
    still_good()
    nan_m = m64.copy()
    nan_m[1, 2] = np.inf
    assert call(grid, (2, 2, 2), mat=nan_m) == VT_EINVAL and b'not finite' in lib.vt_last_error()
    still_good()
    with pytest.raises(ValueError):
        sv.warp(grid, m, out_shape, output=np.zeros((10, 18, 19), np.float32))
    still_good()
    assert lib.vt_volume_warp_f64(sv._handle, m64.ctypes.data, grid.ctypes.data, 2, 2, 2, 10, 0, 18, out.ctypes.data, 0) == VT_EINVAL
    still_good()
    # a stack handle holds in-plane coefficients
    stack = vt.StaticVolume(wc.source_volume(), interpolation='filt_bspline', device='gpu:0', stack=True)
    with pytest.raises(RuntimeError, match='in-plane'):
        stack.warp(grid, m, out_shape)
    assert lib.vt_volume_warp_f64(stack._handle, m64.ctypes.data, grid.ctypes.data, 2, 2, 2, *out_shape, out.ctypes.data, 0) == VT_EUNSUPPORTED
    stack.close()
    still_good()


def test_slab_and_unfinalized_handles_are_refused():
    lib = _native.load()
    vol = np.ascontiguousarray(wc.source_volume()[:20, :24, :28])
    grid = np.zeros((1, 1, 1, 3), np.float32)
    out = np.zeros((8, 8, 8), np.float32)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert lib.vt_volume_warp(h, None, grid.ctypes.data, 1, 1, 1, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    assert b'slab' in lib.vt_last_error()
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert lib.vt_volume_warp(h, None, grid.ctypes.data, 1, 1, 1, 8, 8, 8, out.ctypes.data, 0) == VT_EINVAL
    assert b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    _native.check(lib.vt_volume_warp(h, None, grid.ctypes.data, 1, 1, 1, 8, 8, 8, out.ctypes.data, 0), 'warp')
    assert np.array_equal(out, vol[:8, :8, :8])
    lib.vt_volume_destroy(h)
