"""-m gpu: the three general-matrix kernels -- affine_tiled (kind 2), the lane-block kernel (9), the packed-footprint kernel (6) -- held to
their staged boxes: the host model of their tap indices (tests/affine_index_model.py) pinned to what the library reports, a poisoned
neighbour at the source voxels a tap below the box would read, and signed data on the lattice tables.

Flag sets as tests/test_gpu_lattice.py forces the families.  Trilinear handles are made under VT_BLOCK_LINEAR=1 and VT_SPAN=0, so that the
lane-block kernel and the kernel of vt_kernels_packed.hip serve trilinear launches too (by default the planner gives those to the
packed-span kernel, which has its own origin margin and is not modelled here).

Poisoned neighbour.  Before kBoxMargin reached these kernels, a voxel whose coordinate is exactly floor(lo) of its tile could arrive with
box index -1 and fraction 1.0f; its zero-weight tap then read the neighbouring row of the box.  affine_index_model.POISON_CASES names, per
(kernel, interpolation class), cases where that wrapped read lands inside the allocation on a source voxel inside the volume; NaN (and in
a second pass +inf) is written at exactly those source voxels of a standard_normal volume.  The listed output voxels must be finite and
equal the oracle on the clean volume; any other output may be non-finite only if a poisoned voxel lies within its stencil WIDENED BY ONE
VOXEL PER AXIS ON THE LOW SIDE (the fixed-point drift may put a zero-weight tap at floor(s) - 1: the kernels' documented contract).  The
drift goes either way (vt_device.h, struct Fx): a coordinate within 2^-24 BELOW an integer may arrive on it with fraction 0, and its
zero-weight tap is then the one ABOVE the stencil, which that rule cannot judge; affine_index_model.poison_plan therefore places no
poisoned voxel on those taps, and the rule is decidable on every output voxel (the CPU test holds the two-sided contract on the model).  The
lane-block kernel's cubic form has no such case -- a wrapped read of its trimmed, stride-padded image lands on a slot the tile did not
stage, neither in the tables nor among the dedicated lead rows (affine_index_model.lead_cases) -- so (9, cubic) has no poisoned node; the
model's sweep (tests/test_affine_index_model.py) is its guard.
"""
import collections

import numpy as np
import pytest

import affine_index_model as am
import lattice_cases as lc
import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle
from test_gpu_lattice import SHAPES as LATTICE_SHAPES, TOL, matrix_for

pytestmark = pytest.mark.gpu

N = _native
FT = N.FORCE_TILED
FLAGS = {2: FT | N.NO_ZSEP | N.NO_BLOCK | N.NO_PACKED, 9: FT | N.NO_ZSEP, 6: FT | N.NO_ZSEP | N.FORCE_PACKED}
SHAPES = LATTICE_SHAPES[:2]
assert SHAPES == ((70, 66, 72), (33, 47, 50))
NODES = [(0, 'linear'), (0, 'bspline'), (1, 'linear'), (1, 'bspline'), (1, 'filt_bspline')]
SIGNED_STRIDE = 12          # a signed-data node takes every 12th case, shifted from node to node (the oracle costs ~0.1 s per case), and every poisoned case

_PLANS = {}


def handle(vol, interp, monkeypatch):
    """A handle on which all three families can serve this interpolation (the knobs are read when a handle is created)."""
    if interp == 'linear':
        monkeypatch.setenv('VT_BLOCK_LINEAR', '1')
        monkeypatch.setenv('VT_SPAN', '0')
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    if interp == 'linear':
        monkeypatch.delenv('VT_BLOCK_LINEAR')
        monkeypatch.delenv('VT_SPAN')
    return sv


def expected_plan(kind, m, shape, interp):
    """The model's plan of the launch: of the axis-permuted matrix where try_general_reorient exchanges the copy, else of the matrix as
    given.  The plan depends on the linear part and the interpolation class alone."""
    m = np.asarray(m, np.float64)
    mr, _, pi = am.reoriented(m, shape)
    key = (kind, am.is_cubic(interp), mr[:3, :3].tobytes(), m[:3, :3].tobytes())
    if key not in _PLANS:
        plan = am.PLANNERS[kind](mr, am.is_cubic(interp))
        if plan is None and pi != (0, 1, 2):
            plan = am.PLANNERS[kind](m, am.is_cubic(interp))
        _PLANS[key] = plan
    return _PLANS[key]


def case_matrix(si, name):
    shape = SHAPES[si]
    for n, m64, t in lc.cases(shape):
        if n == name:
            return m64, matrix_for(m64, t)
    m = dict(am.lead_cases(shape))[name]
    return m, np.ascontiguousarray(m)


@pytest.mark.parametrize('si,interp', NODES, ids=[f'{"x".join(map(str, SHAPES[s]))}-{i}' for s, i in NODES])
def test_model_matches_the_library(si, interp, monkeypatch):
    """Every case of the tables under each family's flag set: wherever last_kernel is the family asked for, vt_volume_info's last_tile,
    last_lds_dims and last_lds_bytes equal the model's.  Every family must have been reached."""
    shape = SHAPES[si]
    vol = np.random.RandomState(17 + si).standard_normal(shape).astype(np.float32)
    sv = handle(vol, interp, monkeypatch)
    reached = collections.Counter()
    bad = []
    try:
        for name, m64, t in lc.cases(shape):
            m = matrix_for(m64, t)
            for kind, flags in FLAGS.items():
                sv.affine(m, _flags=flags)
                info = sv.info()
                if info.last_kernel != kind:
                    continue
                reached[kind] += 1
                plan = expected_plan(kind, m, shape, interp)
                got = (tuple(info.last_tile), tuple(info.last_lds_dims), int(info.last_lds_bytes))
                want = None if plan is None else (tuple(plan['tile']), tuple(plan['reported']), int(plan['lds_bytes']))
                if got != want:
                    bad.append((name, kind, got, want))
    finally:
        sv.close()
    print(f'\n{shape} {interp}: launches per family {dict(sorted(reached.items()))} of {len(list(lc.cases(shape)))} cases each')
    assert not bad, (len(bad), bad[:6])
    assert all(reached[k] > 0 for k in FLAGS), dict(reached)


POISON_NODES = sorted(am.POISON_CASES)


@pytest.mark.parametrize('kind,icls', POISON_NODES, ids=[f'kind{k}-{c}' for k, c in POISON_NODES])
def test_poisoned_neighbour(kind, icls, monkeypatch):
    interp = 'linear' if icls == 'linear' else 'bspline'
    fails = []
    ran = 0
    for si, name in am.POISON_CASES[(kind, icls)]:
        shape = SHAPES[si]
        m64, m = case_matrix(si, name)
        pp = am.poison_plan(kind, np.asarray(m, np.float64), shape, interp)
        listed, poison, allowed = pp['listed'], pp['poison'], pp['allowed']
        assert len(listed) and len(poison), (name, 'the before-model lists no wrapped in-allocation read: POISON_CASES is out of date')
        clean = np.random.RandomState(29 + si).standard_normal(shape).astype(np.float32)
        want = oracle.affine_ex(clean, m64, interp, shape)
        tol = TOL[interp] * float(np.abs(clean).max())
        li = tuple(listed.T)
        for badval in (np.nan, np.inf):
            vol = clean.copy()
            vol[tuple(poison.T)] = badval
            sv = handle(vol, interp, monkeypatch)
            try:
                got = sv.affine(m, _flags=FLAGS[kind])
                k = int(sv.info().last_kernel)
            finally:
                sv.close()
            assert k == kind, (name, 'family not reached', k)
            ran += 1
            at = got[li]
            nonfinite = int((~np.isfinite(at)).sum())
            err = float(np.abs(np.where(np.isfinite(at), at, 0.0) - want[li]).max())
            stray = ~np.isfinite(got) & ~allowed
            ok = np.isfinite(got)
            err_all = float(np.abs(got[ok] - want[ok]).max())
            print(f'kind {kind} {interp} {name} poison {badval}: {len(poison)} source voxels, {len(listed)} listed outputs: {nonfinite} non-finite, '
                  f'max err {err:.3e} (tol {tol:.3e}); non-finite outside the widened stencils: {int(stray.sum())}; max err elsewhere {err_all:.3e}')
            if nonfinite or err > tol:
                fails.append((name, str(badval), 'listed voxels', nonfinite, err))
            if stray.any():
                fails.append((name, str(badval), 'non-finite outside the widened stencils', int(stray.sum())))
            if err_all > tol:
                fails.append((name, str(badval), 'finite voxels off the oracle', err_all))
    assert ran >= 2
    assert not fails, fails


SIGNED_NODES = [(si, interp, scale) for si, interp in NODES for scale in (1.0, 1e3)]


@pytest.mark.parametrize('si,interp,scale', SIGNED_NODES, ids=[f'{"x".join(map(str, SHAPES[s]))}-{i}-{sc:g}' for s, i, sc in SIGNED_NODES])
def test_signed_data_on_lattice_coordinates(si, interp, scale, monkeypatch):
    """standard_normal x {1, 1e3} data (the tables have only ever met random_sample) against the oracle, tolerance relative to max|volume|
    as tests/test_gpu_ranges.py has it; every family, every voxel."""
    shape = SHAPES[si]
    node = SIGNED_NODES.index((si, interp, scale))
    vol = (np.random.RandomState(41 + si).standard_normal(shape) * scale).astype(np.float32)
    filt = interp.startswith('filt')
    src = oracle.prefilter(vol) if filt else vol
    tol = TOL[interp] * float(np.abs(vol).max())
    poisoned = {name for lst in am.POISON_CASES.values() for s, name in lst if s == si}
    picked = [(name, m64, matrix_for(m64, t)) for j, (name, m64, t) in enumerate(lc.cases(shape)) if (j + node) % SIGNED_STRIDE == 0 or name in poisoned]
    picked += [(name, m, np.ascontiguousarray(m)) for name, m in am.lead_cases(shape) if name in poisoned]
    sv = handle(vol, interp, monkeypatch)
    reached = collections.Counter()
    worst = collections.defaultdict(float)
    fails = []
    try:
        for name, m64, m in picked:
            want = oracle.affine_ex(src, m64, 'bspline' if filt else interp, shape)
            for kind, flags in FLAGS.items():
                got = sv.affine(m, _flags=flags)
                k = int(sv.info().last_kernel)
                reached[k] += 1
                err = float(np.abs(got - want).max())
                worst[k] = max(worst[k], err)
                if not err <= tol:
                    fails.append((name, kind, k, err))
    finally:
        sv.close()
    print(f'\n{shape} {interp} x {scale:g}: {len(picked)} cases, launches per kernel {dict(sorted(reached.items()))}, largest |got - oracle| per kernel '
          f'{ {k: f"{v:.3e}" for k, v in sorted(worst.items())} } (tol {tol:.3e})')
    assert not fails, (len(fails), fails[:6])
    assert all(reached[k] > 0 for k in FLAGS), dict(reached)
