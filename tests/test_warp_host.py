"""StaticVolume.warp without a GPU: the model's coordinates on affine fields, the staging safety invariant of the planning rule on
every case the GPU file uses, the device='cpu' path (scipy's map_coordinates) against the model, utils.grid_nodes, argument errors."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import warp_cases as wc
import warp_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
TOL_CPU = {'linear': 1e-6, 'bspline': 1e-6, 'bspline_simple': 1e-6, 'filt_bspline': 3e-6, 'filt_bspline_simple': 3e-6}


@pytest.mark.parametrize('case', wc.affine_field_cases(), ids=lambda c: c[0])
def test_affine_fields_reproduce_the_affine_chain(case):
    name, out_shape, grid, B, c = case
    for m in (None, wc.rotated(out_shape)):
        s = wm.coords(m, grid, out_shape)
        want = wm.affine_coords(wc.combined(np.eye(4) if m is None else m, B, c), out_shape)
        err = float(np.abs(s - want).max())
        print(name, 'identity' if m is None else 'rotated', 'max|s - chain|', err)
        assert err <= 1e-11


def _every_plan():
    for name, (out_shape, grid, m) in wc.field_cases().items():
        yield name, out_shape, grid, m
    for name, out_shape, grid, B, c in wc.affine_field_cases():
        yield 'affine_' + name, out_shape, grid, wc.rotated(out_shape)


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_staging_safety_invariant(interp):
    """In every tile the model marks staged, every tap index of every voxel lies in [0, L) of that tile's box on all three axes."""
    staged = direct = 0
    for name, out_shape, grid, m in _every_plan():
        p = wm.plan(m, grid, out_shape, interp)
        s = wm.coords(m, grid, out_shape)
        assert wm.violations(p, s, out_shape, interp) == [], name
        assert p.lds_bytes <= 160 * 1024, name
        assert (p.nodes <= np.asarray(p.tile) + 1).all(), name            # at most floor((T - 1) r) + 2 nodes per axis
        staged += int(p.staged.sum())
        direct += int((~p.staged).sum())
    assert staged > 0 and direct > 0


def test_the_spike_splits_the_tiles_and_the_push_empties_some():
    out_shape, grid, m = wc.field_cases()['spike200']
    for interp in ('linear', 'bspline'):
        what = wm.tile_outcome(wm.plan(m, grid, out_shape, interp), m, wc.SRC)
        assert (what == 'direct').any() and (what == 'stage').any(), interp
    out_shape, grid, m = wc.field_cases()['pushed_out']
    what = wm.tile_outcome(wm.plan(m, grid, out_shape, 'linear'), m, wc.SRC)
    assert (what == 'zero').any() and (what == 'stage').any()
    ins = wc.model_result('pushed_out', 'linear')[1]
    assert not ins[:, :, :8].any() and ins[:, :, 24:].any()               # a face region is outside


@pytest.mark.parametrize('interp', wc.INTERPS)
@pytest.mark.parametrize('name', ['g345_a12', 'dense_a1.5', 'pushed_out'])
def test_cpu_path_against_the_model(name, interp):
    """filt_*: the CPU path's coefficients are scipy's (spline_filter, mode='constant'), the library's and prefilter_f64's start the
    recursion differently and differ from them by up to 1e-2 near a face (tests/test_backproject_host.py: cpu_bound).  What this test
    holds the CPU path to is its coordinates and its sampling, so the model samples the coefficients the CPU path defines."""
    out_shape, grid, m = wc.field_cases()[name]
    vals, ins, s, _ = wc.model_result(name, interp)
    if interp in wm.FILTERED:
        from scipy.ndimage import spline_filter
        vals = wm.sample(spline_filter(wc.source_volume().astype(np.float64), 3, output=np.float64, mode='constant'), s, interp)
    got = vt.StaticVolume(wc.source_volume(), interpolation=interp, device='cpu').warp(grid, m, out_shape)
    assert got.shape == out_shape and got.dtype == np.float32
    full = wm.taps_inside(s, wc.SRC, interp)
    assert full.sum() > 0.2 * full.size or name == 'pushed_out'
    err = float(np.abs(got.astype(np.float64) - vals)[full].max())
    print(name, interp, 'max|cpu - model| where every tap is inside', err, 'voxels', int(full.sum()))
    assert err <= TOL_CPU[interp]
    # scipy's constant mode: a coordinate outside [0, dim - 1] gives exactly 0
    outside = np.zeros(out_shape, bool)
    for r in range(3):
        outside |= (s[r] < -1e-9) | (s[r] > wc.SRC[r] - 1 + 1e-9)
    assert outside.any() or name != 'pushed_out'
    assert not got[outside].any()


def test_cpu_defaults_and_output_argument():
    vol = wc.source_volume()
    sv = vt.StaticVolume(vol, device='cpu')
    zero = np.zeros((1, 1, 1, 3))
    assert np.array_equal(sv.warp(zero), vol)                             # identity matrix, the volume's shape, no displacement
    out = np.empty(wc.OUT_A, np.float32)
    grid = wc.field_cases()['g222_a1.5'][1]
    assert sv.warp(grid, wc.rotated(wc.OUT_A), wc.OUT_A, output=out) is out
    assert np.array_equal(out, sv.warp(grid.astype(np.float64), wc.rotated(wc.OUT_A), wc.OUT_A))


def test_grid_nodes_formula():
    got = vt.utils.grid_nodes((3, 1, 5), (9, 17, 19))
    assert got.shape == (3, 1, 5, 3) and got.dtype == np.float64
    for i in range(3):
        for k in range(5):
            assert np.array_equal(got[i, 0, k], [i * 8 / 2, 8.0, k * 18 / 4])
    assert np.array_equal(vt.utils.grid_nodes((4, 6, 7), wc.OUT_C), wc.nodes((4, 6, 7), wc.OUT_C))
    dense = vt.utils.grid_nodes(wc.OUT_A, wc.OUT_A)
    assert np.array_equal(dense[..., 0], np.broadcast_to(np.arange(10.0)[:, None, None], wc.OUT_A))
    for bad in ((3, 5), (0, 2, 2), (2, 2, 20), (2.0, 2, 2)):
        with pytest.raises(ValueError):
            vt.utils.grid_nodes(bad, wc.OUT_A)
    with pytest.raises(ValueError):
        vt.utils.grid_nodes((2, 2, 2), (10, 18))


def test_argument_errors():
    sv = vt.StaticVolume(wc.source_volume(), device='cpu')
    good = np.zeros((2, 2, 2, 3), np.float32)
    for bad in (np.zeros((2, 2, 2)), np.zeros((2, 2, 2, 2)), np.zeros((2, 2, 3)), np.zeros((0, 2, 2, 3)), np.zeros((2, 2, 19, 3)),
                np.zeros((11, 2, 2, 3))):
        with pytest.raises(ValueError):
            sv.warp(bad, None, wc.OUT_A)
    for bad_m in (np.eye(3), np.zeros((2, 4, 4))):
        with pytest.raises(ValueError):
            sv.warp(good, bad_m, wc.OUT_A)
    for bad_shape in ((10, 18), (10, 18, 0), (10.0, 18, 18)):
        with pytest.raises(ValueError):
            sv.warp(good, None, bad_shape)
    with pytest.raises(ValueError):
        sv.warp(good, None, wc.OUT_A, output=np.zeros((10, 18, 19), np.float32))


def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    grid = np.zeros((2, 2, 2, 3), np.float32)
    out = np.zeros((4, 4, 4), np.float32)
    m32, m64 = np.eye(4, dtype=np.float32), np.eye(4)
    assert lib.vt_volume_warp(None, m32.ctypes.data, grid.ctypes.data, 2, 2, 2, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_warp_f64(None, m64.ctypes.data, grid.ctypes.data, 2, 2, 2, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_warp(None, None, grid.ctypes.data, 2, 2, 2, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert b'NULL' in lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_warp', 'vt_volume_warp_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 11
    assert '20 resampling through a displacement grid' in header         # the last_kernel comment names the new kernel
    assert 'grid_nodes' in dir(vt.utils)
