"""Every prefilter kernel form and dispatch branch against the float64 recursion (tests/prefilter_model.py).

The case lists below are routed through the host model of the dispatch by tests/test_prefilter_model.py (CPU), which fails when a
(form, template parameter) pair or one of the listed branches is reached by no case.  Distances are in u = 2^-23 * max|c64|:

  * against `prefilter_f64`: max|hip - c64| <= 2 * R_REF * u.  R_REF is the float32 oracle's own distance from float64 over this
    case list (measured on the CPU by test_prefilter_model.py::test_oracle_distance, never on the kernels).  The kernels re-associate the
    same recursion (wave scans, carries through LDS, fma), which reorders roundings and adds none of consequence: twice the sequential
    float32 recursion's distance allows for that;
  * against the float32 oracle on unit-range data: the suite's 5e-6, as tests/test_gpu_parity.py has it.

Every case prints its figures (pytest -s shows them) before it is judged; a family reports all of its failing cases at once.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle
import prefilter_model as pm

pytestmark = pytest.mark.gpu

R_REF = 3.6                   # largest oracle distance over CASES x KINDS in u (test_prefilter_model.py::test_oracle_distance), rounded up
F64_FACTOR = 2.0              # kernels: at most F64_FACTOR * R_REF * u from float64
ORACLE_TOL = 5e-6             # unit-range data against the float32 oracle
TOL_FILT = 3e-6               # tests/test_gpu_parity.py TOL['filt_bspline'] (unit-range data: max|c64| about 7.5)
KINDS = ('unit', 'signed')
SHIFT = (0.25, -0.5, 0.125)   # sub-voxel shift: every coefficient and the pad columns take part

# ---------------------------------------------------------------------------------------------------
# the cases: (D, H, W) through vt_prefilter_inplace (pitch = W)
# ---------------------------------------------------------------------------------------------------
CHUNK_N = (1, 2, 11, 12, 13, 32, 33, 63, 64, 65, 80, 255, 256, 257, 260, 389)
BLOCK_N = (40, 255, 256, 257, 271, 272, 273, 288, 530)
DENSE = {
    # widths that are no multiple of 4 take prefilter_x_scan<1..32> (first, middle, last width of each); the others x_scan4
    'x_scan': [(2, 3, w) for w in (1, 5, 63, 64, 65, 101, 127, 128, 129, 201, 255, 257, 301, 511, 512, 513, 700, 701, 1023, 1025, 1027,
                                  1501, 2047)],
    'x_scan4': [(2, 3, w) for w in (4, 64, 252, 256, 260, 512, 516, 1024, 1028, 2048)],
    # W > 2048: the chunked form along x, lanes along y (3 lanes of one wave; 70 lanes in two waves)
    'x_wide': [(2, h, w) for h in (3, 70) for w in (2049, 2100, 2500)],
    # odd widths: the chunked form on axes 0 (67 columns: two lane blocks) and 1
    'chunked': [(n, 3, 67) for n in CHUNK_N] + [(2, n, 5) for n in CHUNK_N],
    # rows of whole vectors: the block form on axes 0 and 1; one and two column blocks
    'block': [(n, 2, w) for w in (4, 8, 260) for n in BLOCK_N] + [(2, n, w) for w in (4, 8, 260) for n in BLOCK_N],
    # rows of whole 8-sample lanes, >= 40 rows: X and Y fused ((260, 64): a last row segment of 4 rows, shorter than the warm-up)
    'xy': [(2, h, w) for h, w in ((40, 64), (160, 64), (161, 72), (260, 64), (288, 64), (289, 72), (40, 512), (41, 520), (40, 960),
                                  (40, 968), (45, 1000))],
}
CASES = [(fam, shape) for fam, shapes in DENSE.items() for shape in shapes]

CHUNK_KNOB_SHAPES = [(300, 3, 67), (2, 100, 7), (2, 3, 2100)]
CHUNK_KNOB_VALUES = ('32', '64', '128')

# one impulse volume per form: impulses on both sides of every cut the model reports
IMPULSE_SHAPES = [(2, 3, 101), (2, 3, 255), (2, 3, 301), (2, 3, 701), (2, 3, 2047), (2, 3, 512), (2, 3, 1024), (2, 3, 2048),
                  (2, 3, 2100), (389, 3, 67), (2, 80, 5), (530, 2, 260), (2, 530, 8), (2, 273, 4), (2, 289, 72), (2, 45, 1000)]

# resident handles (pitch = resident_pitch(W)); the last six: the block form on axis 0 / axis 1 with W % 4 = 1, 2, 3
RESIDENT = [(3, 20, 600), (3, 20, 1500), (2, 24, 1100), (2, 3, 2100), (24, 36, 50), (36, 24, 50), (33, 41, 67),
            (257, 2, 5), (40, 2, 6), (273, 2, 7), (2, 257, 5), (2, 40, 6), (2, 273, 7)]
RECYCLED = (41, 44, 50)

# slab windows of a (SLAB_LO + depth, 40, 46) volume: planes [SLAB_LO, SLAB_LO + depth), low end interior
SLAB_H, SLAB_W, SLAB_LO = 40, 46, 10
SLAB_DEPTHS = (24, 36, 48)
SLAB_INSIDE = 19              # output planes whose taps stay >= 18 planes inside the window's low end

# the one-shot pipeline tests of tests/test_gpu_parity.py (shape, axis-0-separable matrices among the cases)
ONESHOT_SHAPES = [((256, 192, 320), True), ((40, 512, 520), True), ((100, 300, 290), True), ((150, 700, 650), False)]

# static knobs: one fresh process each (read once per process); tests/prefilter_knob_child.py runs KNOB_SHAPES
KNOBS = [{'VT_PF_NO_XY': '1'}, {'VT_PF_NO_BLOCK': '1'}, {'VT_PF_BLOCK': '1'}, {'VT_PF_BLOCK': '2'}]
KNOB_SHAPES = [(300, 3, 67), (2, 273, 260), (273, 2, 8), (2, 161, 72)]
KNOB_TIMEOUT = 120


# ---------------------------------------------------------------------------------------------------
# data and references (computed once per (shape, kind), never written to)
# ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def make_vol(shape, kind):
    r = np.random.RandomState(shape[0] * 1000003 + shape[1] * 1009 + shape[2]).random_sample(shape)
    if kind == 'signed':
        r = (r - 0.5) * 2000.0
    v = r.astype(np.float32)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def reference(shape, kind):
    c = pm.prefilter_f64(make_vol(shape, kind))
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def impulse_vol(shape):
    v = np.zeros(shape, np.float32)
    for idx in pm.impulse_positions(pm.route_dense(shape), shape):
        v[idx] = 1.0
    v.setflags(write=False)
    return v


def form_names(r):
    return ' '.join(f'{f}<{p}>' for f, p in pm.forms(r))


def run_dense(vol):
    lib = _native.load()
    d = _native.DeviceArray.from_numpy(np.ascontiguousarray(vol), 0)
    try:
        _native.check(lib.vt_prefilter_inplace(0, d.ptr, *vol.shape), 'vt_prefilter_inplace')
        return d.get()
    finally:
        d.free()


def judge_dense(tag, shape, kind, vol, c64, env=None, bad=None):
    """One dense case: prints the figures, appends to `bad` what misses its bound."""
    r = pm.route_dense(shape, env=env)
    got = run_dense(vol)
    u = pm.unit(c64)
    r_gpu = float(np.abs(got - c64).max()) / u
    line = f'PFR {tag} {shape} {kind} [{form_names(r)}] r_gpu={r_gpu:.2f}'
    if r_gpu > F64_FACTOR * R_REF:
        bad.append(f'{shape} {kind}: {r_gpu:.2f} u from float64 (bound {F64_FACTOR * R_REF})')
    if kind == 'unit':
        d_or = float(np.abs(got - oracle.prefilter(vol)).max())
        line += f' oracle={d_or:.2e}'
        if d_or > ORACLE_TOL:
            bad.append(f'{shape} {kind}: {d_or:.2e} from the float32 oracle (bound {ORACLE_TOL})')
    print(line)


# ---------------------------------------------------------------------------------------------------
# dense
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('family', list(DENSE))
def test_dense_forms_against_float64(family, kind):
    """Every dense case of a family, both data kinds: <= 2 R_REF u from float64, and <= 5e-6 from the float32 oracle on unit data."""
    bad = []
    for shape in DENSE[family]:
        judge_dense(family, shape, kind, make_vol(shape, kind), reference(shape, kind), bad=bad)
    assert not bad, '\n'.join(bad)


@pytest.mark.parametrize('value', CHUNK_KNOB_VALUES)
def test_chunk_size_knob(value, monkeypatch):
    """VT_PF_CHUNK (read on every call) selects prefilter_chunked<32 | 64 | 128> on three chunked shapes."""
    monkeypatch.setenv('VT_PF_CHUNK', value)
    bad = []
    for shape in CHUNK_KNOB_SHAPES:
        assert ('chunked', int(value)) in pm.forms(pm.route_dense(shape, env={'VT_PF_CHUNK': value}))
        for kind in KINDS:
            judge_dense(f'chunk{value}', shape, kind, make_vol(shape, kind), reference(shape, kind), env={'VT_PF_CHUNK': value}, bad=bad)
    assert not bad, '\n'.join(bad)


def test_unit_impulses_on_both_sides_of_every_cut():
    """A unit impulse on either side of every segment, chunk and wave-share boundary the model reports: the float64 response decays as
    z^|i - p|, so a carry applied to the wrong neighbour (or dropped) is an error of the size of the response itself."""
    bad = []
    for shape in IMPULSE_SHAPES:
        vol = impulse_vol(shape)
        c64 = pm.prefilter_f64(vol)
        r = pm.route_dense(shape)
        got = run_dense(vol)
        r_gpu = float(np.abs(got - c64).max()) / pm.unit(c64)
        print(f'PFR impulse {shape} impulse [{form_names(r)}] r_gpu={r_gpu:.2f} impulses={int(vol.sum())}')
        if r_gpu > F64_FACTOR * R_REF:
            bad.append(f'{shape}: {r_gpu:.2f} u from float64 (bound {F64_FACTOR * R_REF})')
    assert not bad, '\n'.join(bad)


# ---------------------------------------------------------------------------------------------------
# resident handles and slab windows
# ---------------------------------------------------------------------------------------------------
def shift_matrix():
    m = np.eye(4, dtype=np.float32)
    m[:3, 3] = SHIFT
    return m


def resident_tol(c64, kind):
    return TOL_FILT * (1.0 if kind == 'unit' else float(np.abs(c64).max()) / 7.5)


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', RESIDENT, ids=lambda s: 'x'.join(map(str, s)))
def test_resident_handles_against_float64_coefficients(shape, kind):
    """filt_bspline handles (pitched rows: x_scan4, xy and the block form on widths that are no multiple of 4): the shifted resampling
    against the oracle's resampling of the float64 coefficients, over the whole volume."""
    vol, c64 = make_vol(shape, kind), reference(shape, kind)
    m = shift_matrix()
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    try:
        got = sv.affine(m)
    finally:
        sv.close()
    want = oracle.affine_ex(c64.astype(np.float32), m, 'filt_bspline', shape)
    err, tol = float(np.abs(got - want).max()), resident_tol(c64, kind)
    print(f'PFR resident {shape} {kind} [{form_names(pm.route_resident(shape))}] err={err:.3e} tol={tol:.3e}')
    assert err <= tol, (shape, kind, err, tol)


def test_resident_handle_on_recycled_buffers():
    """Both buffers of the handle come back dirty from the allocation cache (a closed handle of the same size held 1e6 everywhere,
    coefficients up to 1e7): with W % 4 = 2 the voxels whose taps reach the pad columns must still match."""
    shape, kind = RECYCLED, 'unit'
    assert shape[2] % 4 and pm.route_resident(shape).passes[-1].form == 'block'
    vt.StaticVolume(np.full(shape, 1.0e6, np.float32), interpolation='filt_bspline', device='gpu:0').close()
    vol, c64 = make_vol(shape, kind), reference(shape, kind)
    m = shift_matrix()
    sv = vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0')
    try:
        got = sv.affine(m)
    finally:
        sv.close()
    want = oracle.affine_ex(c64.astype(np.float32), m, 'filt_bspline', shape)
    err = np.abs(got - want)
    print(f'PFR recycled {shape} {kind} err={float(err.max()):.3e} at the pad columns={float(err[:, :, -3:].max()):.3e}')
    assert float(err[:, :, -3:].max()) <= TOL_FILT          # taps of the last columns read the pad columns
    assert float(err.max()) <= TOL_FILT


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('depth', SLAB_DEPTHS)
def test_slab_windows_with_an_interior_low_end(depth, kind):
    """vt_volume_create_slab with SLAB_LO_INTERIOR: the steady-state causal start on axis 0 through the chunked form in place
    (24 planes), out of place (36) and the block form (48).  Output planes whose taps stay 18 planes inside the window's low end
    against the whole volume's float64 coefficients; every output plane against the float64 recursion with the same start."""
    import ctypes
    lib = _native.load()
    G = SLAB_LO + depth
    shape = (G, SLAB_H, SLAB_W)
    vol, c64 = make_vol(shape, kind), reference(shape, kind)
    win = np.ascontiguousarray(vol[SLAB_LO:])
    m = shift_matrix()
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, depth, SLAB_H, SLAB_W, _native.INTERP_CODES['filt_bspline'], win.ctypes.data,
                                            _native.SLAB_LO_INTERIOR, SLAB_LO, G, SLAB_LO, depth, ctypes.byref(h)), 'vt_volume_create_slab')
    try:
        got = np.empty((depth, SLAB_H, SLAB_W), np.float32)
        _native.check(lib.vt_volume_affine(h, m.ctypes.data, got.ctypes.data, 0), 'vt_volume_affine')
    finally:
        lib.vt_volume_destroy(h)
    tol = resident_tol(c64, kind)
    whole = oracle.affine_ex(c64.astype(np.float32), m, 'filt_bspline', (depth - SLAB_INSIDE, SLAB_H, SLAB_W), 0, G, SLAB_LO + SLAB_INSIDE)
    err_whole = float(np.abs(got[SLAB_INSIDE:] - whole).max())
    cwin = pm.prefilter_f64(win, lo_interior_axis0=True)
    # (from the third plane on: no tap of those leaves the window)
    same = oracle.affine_ex(cwin.astype(np.float32), m, 'filt_bspline', (depth - 2, SLAB_H, SLAB_W), SLAB_LO, G, SLAB_LO + 2)
    err_same = float(np.abs(got[2:] - same).max())
    print(f'PFR slab depth={depth} {kind} [{form_names(pm.route_resident((depth, SLAB_H, SLAB_W), lo_interior=True))}] '
          f'whole={err_whole:.3e} same_start={err_same:.3e} tol={tol:.3e}')
    assert err_whole <= tol, (depth, kind, err_whole, tol)
    assert err_same <= tol, (depth, kind, err_same, tol)


# ---------------------------------------------------------------------------------------------------
# static knobs: one fresh process per setting
# ---------------------------------------------------------------------------------------------------
def test_static_knobs_in_fresh_processes():
    """VT_PF_NO_XY, VT_PF_NO_BLOCK, VT_PF_BLOCK=1|2 are read once per process: one child each, one after the other, each with its own
    time limit; the first child that fails ends the test and no further child is started."""
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'prefilter_knob_child.py')
    for knob in KNOBS:
        env = dict(os.environ)
        for name in ('VT_PF_NO_XY', 'VT_PF_NO_BLOCK', 'VT_PF_BLOCK', 'VT_PF_CHUNK'):
            env.pop(name, None)
        env.update(knob)
        try:
            p = subprocess.run([sys.executable, child], env=env, capture_output=True, text=True, timeout=KNOB_TIMEOUT)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f'{knob}: no result within {KNOB_TIMEOUT} s\n{e.stdout}\n{e.stderr}')
        print(p.stdout, end='')
        assert p.returncode == 0, f'{knob}: exit status {p.returncode}\n{p.stdout}\n{p.stderr}'
        assert p.stdout.count('PFR knob') == len(KNOB_SHAPES) * len(KINDS), p.stdout
