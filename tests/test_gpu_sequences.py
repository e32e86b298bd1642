"""-m gpu: long mixed call sequences on one handle (tests/handle_sequences.py) against the stateless model.

The per-call suites hold every kernel family to the oracle; nothing else holds the state a handle carries BETWEEN calls: the launch
counter of the plane-quad ping-pong, the request counters of the reorientation copies, the lazy copy table under a budget, the tile counters
the three persistent kernel families share (zeroed once, left zero by every launch for the next, which may be another family with another
grid), the staging plans and their epoch, the cached plane sum of the projection helper, staging buffers sized by the largest call so far,
the output shape, and underneath the handles the per-device recycler.  Every transforming op of every sequence is held to
  1. the oracle on every voxel, at the tolerances of tests/test_gpu_parity.py (x output depth for projections) and, for the edge='scipy'
     family, scipy itself at those of tests/test_gpu_edge_scipy.py; keep_outside ops also compare the set of untouched voxels;
  2. (families P, E) the same op executed alone on a newly created handle with the same environment and output shape: last_kernel,
     last_tile and last_grid EQUAL, the output bit-identical;
  3. (families P, S) twin handles that run the same sequence in lockstep under each setting the library documents as result-neutral
     (VT_NO_PROJ_CACHE=1, VT_QUAD_PINGPONG=0 / 2, VT_NO_PLANSHARE on every affine; S also a twin without any budget / release / trim op,
     compared bit for bit wherever last_kernel and last_tile agree);
  4. invariants of vt_volume_info after every op.
A failing op reports (family, sequence, op index, op, last_kernel, error) and ends its sequence; handles are closed in `finally`.
test_zz_sequence_ledger asserts at the end that the sequences reached what they are for.

One finding is written into the checks rather than skipped: `resident_bytes` right after create is not the floor of a handle for ever --
the first fused projection adds the projection helper (3 x H x W, counted by the budget, never released).  The invariant "after
release_copies / set_max_resident(plain) the handle is back at its floor" uses create's value plus the helper once it exists, and the
helper's size is taken from the one op that creates it (resident_bytes may grow by nothing else during a fused projection).
"""
import collections
import contextlib
import ctypes
import types

import numpy as np
import pytest

import handle_sequences as hs
from voltools_amd import _native

pytestmark = pytest.mark.gpu

N = _native
GARBAGE = np.float32(12345.0)           # pre-fill of outputs that must be overwritten completely

LEDGER = dict(kernels=collections.Counter(), evictions=0, reorient_builds=0, quad_parity=collections.Counter(), recreate_same=0,
              twin_bits=collections.Counter(), twin_ops=0, queue_used=collections.Counter(), transitions=collections.Counter(),
              ops=collections.Counter(), worst={})
RAN = set()
ALL = set()


@contextlib.contextmanager
def environment(monkeypatch, env):
    """Knobs are read when a handle is created: set for the create call only."""
    with monkeypatch.context() as mp:
        for k in ('VT_REORIENT', 'VT_BLOCK_MIN', 'VT_BLOCK_LINEAR', 'VT_NO_PROJ_CACHE', 'VT_QUAD_PINGPONG', 'VT_MAX_RESIDENT_GB'):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        yield


def snapshot(lib, h):
    info = N.VolumeInfo()
    N.check(lib.vt_volume_info(h, ctypes.byref(info)), 'vt_volume_info')
    return types.SimpleNamespace(kernel=int(info.last_kernel), tile=tuple(info.last_tile), grid=int(info.last_grid), out=(info.out_depth, info.out_height, info.out_width),
                                 resident=int(info.resident_bytes), built=int(info.copies_built), evicted=int(info.copies_evicted), budget=int(info.max_resident_bytes))


class Handle:
    """One vt_volume and what the model knows about it."""

    def __init__(self, lib, monkeypatch, env, vol, interp, edge='texture', window=None):
        self.lib, self.vol, self.interp, self.edge, self.window = lib, vol, interp, edge, window
        data = vol.make()
        self.h = ctypes.c_void_p()
        with environment(monkeypatch, env):
            if window:
                w0, w1, G, g0, g1 = window
                win = np.ascontiguousarray(data[w0:w1])
                N.check(lib.vt_volume_create_slab(0, w1 - w0, vol.shape[1], vol.shape[2], N.INTERP_CODES[interp], win.ctypes.data,
                                                  N.SLAB_LO_INTERIOR | N.SLAB_HI_INTERIOR, w0, G, g0, g1 - g0, ctypes.byref(self.h)), 'vt_volume_create_slab')
                self.out = (g1 - g0, vol.shape[1], vol.shape[2])
            else:
                N.check(lib.vt_volume_create(0, *vol.shape, N.INTERP_CODES[interp], data.ctypes.data, N.EDGE_SCIPY if edge == 'scipy' else 0,
                                             ctypes.byref(self.h)), 'vt_volume_create')
                self.out = tuple(vol.shape)
        s = self.info()
        self.floor = s.resident             # the plain copy; plus the projection helper once a fused projection has made it
        self.created_resident = s.resident
        self.has_helper = False
        self.budget = 0
        self.built, self.evicted = s.built, s.evicted
        self.quad_launches = 0
        self.asked = collections.Counter()
        assert s.out == self.out and s.budget == 0

    def info(self):
        return snapshot(self.lib, self.h)

    def close(self):
        if self.h:
            self.lib.vt_volume_destroy(self.h)
            self.h = None


class Runner:
    """Executes the ops of a sequence on its own handles (main / other), under its own create-time environment."""

    def __init__(self, seq, tag, monkeypatch, env_extra=None, flag_or=0, skip_policy=False):
        self.seq, self.tag, self.mp = seq, tag, monkeypatch
        self.env = dict(seq.env, **(env_extra or {}))
        self.flag_or, self.skip_policy = flag_or, skip_policy
        self.lib = N.load()
        self.handles = {}
        self.handles['main'] = Handle(self.lib, monkeypatch, self.env, seq.vol, seq.interp, seq.edge, seq.window)
        if seq.other_vol:
            self.handles['other'] = Handle(self.lib, monkeypatch, self.env, seq.other_vol, seq.other_interp)
        self.recreate_same = 0
        self.evicted_before = 0             # evictions of main handles that a recreate has destroyed since

    def close(self):
        for h in self.handles.values():
            h.close()

    # ---- one transforming call on a handle; returns the output as a host array ----
    def transform(self, H, op):
        lib = self.lib
        flags = op.flags | (N.KEEP_OUTSIDE if op.keep else 0) | (N.OUT_DEVICE if op.device_out else 0)
        if op.kind in ('affine', 'affine_batch'):
            flags |= self.flag_or
        n = len(op.m)
        dt = np.float64 if op.f64 else np.float32
        m = np.ascontiguousarray(np.asarray(op.m, np.float64).reshape(n, 16).astype(dt))
        if op.kind == 'affine':
            shape = H.out
        elif op.kind == 'affine_batch':
            shape = (n,) + tuple(H.out)
        elif op.kind == 'extract':
            shape = (n,) + tuple(op.out_shape)
        else:
            shape = tuple(H.out[1:])
        assert op.kind == 'extract' or tuple(op.out_shape) == tuple(H.out), ('model and handle disagree on the output shape', op.out_shape, H.out)
        host = np.full(shape, hs.SENTINEL if op.keep else GARBAGE, np.float32)
        dev = None
        if op.device_out:
            dev = N.DeviceArray.from_numpy(host)
            ptr = ctypes.c_void_p(dev.ptr)
        else:
            ptr = host.ctypes.data
        try:
            if op.kind == 'affine':
                fn = lib.vt_volume_affine_f64 if op.f64 else lib.vt_volume_affine
                N.check(fn(H.h, m.ctypes.data, ptr, flags), 'vt_volume_affine')
            elif op.kind == 'affine_batch':
                N.check(lib.vt_volume_affine_batch(H.h, n, m.ctypes.data, ptr, flags), 'vt_volume_affine_batch')
            elif op.kind == 'extract':
                fn = lib.vt_volume_extract_f64 if op.f64 else lib.vt_volume_extract
                N.check(fn(H.h, n, m.ctypes.data, *op.out_shape, ptr, flags), 'vt_volume_extract')
            else:
                fn = lib.vt_volume_project_f64 if op.f64 else lib.vt_volume_project
                N.check(fn(H.h, m.ctypes.data, ptr, flags), 'vt_volume_project')
            if dev is not None:
                N.check(lib.vt_volume_sync(H.h), 'vt_volume_sync')
                host = dev.get()
        finally:
            if dev is not None:
                dev.free()
        return host

    def run(self, op):
        """Execute one op; returns (output or None, info snapshot of the handle it ran on, info before)."""
        H = self.handles[op.handle]
        before = H.info()
        out = None
        if op.transforms:
            out = self.transform(H, op)
        elif op.kind == 'set_output_shape':
            N.check(self.lib.vt_volume_set_output_shape(H.h, *op.arg), 'vt_volume_set_output_shape')
            H.out = tuple(op.arg)
        elif op.kind == 'set_max_resident':
            H.budget = {'0': 0, 'plain': H.created_resident, '2.6': int(H.created_resident * 2.6)}[op.arg[0]]
            N.check(self.lib.vt_volume_set_max_resident(H.h, H.budget), 'vt_volume_set_max_resident')
        elif op.kind == 'release_copies':
            freed = ctypes.c_uint64(0)
            N.check(self.lib.vt_volume_release_copies(H.h, ctypes.byref(freed)), 'vt_volume_release_copies')
            assert freed.value == before.resident - H.floor, ('release_copies', freed.value, before.resident, H.floor)
        elif op.kind == 'device_trim':
            N.check(self.lib.vt_device_trim(0), 'vt_device_trim')
        elif op.kind == 'recreate':
            self.recreate(op)
            H = self.handles['main']
        else:
            raise KeyError(op.kind)
        after = H.info()
        self.invariants(H, op, before, after)
        return out, after, before

    def recreate(self, op):
        dirty_vol, new_vol = op.arg
        old = self.handles['main']
        old_bytes = old.created_resident
        self.evicted_before += old.info().evicted
        old.close()
        dirty = Handle(self.lib, self.mp, self.env, dirty_vol, self.seq.interp)
        try:
            same = dirty.created_resident == old_bytes
            # one transform into a host array of the next handle's output size: the recycled staging buffer holds 1e3 values too
            N.check(self.lib.vt_volume_set_output_shape(dirty.h, *new_vol.shape), 'vt_volume_set_output_shape')
            m = np.eye(4, dtype=np.float32)
            out = np.empty(new_vol.shape, np.float32)
            N.check(self.lib.vt_volume_affine(dirty.h, m.ctypes.data, out.ctypes.data, 0), 'vt_volume_affine')
            assert float(np.abs(out).max()) > 100.0          # (the outgoing values really are of magnitude 1e3)
        finally:
            dirty.close()
        self.handles['main'] = Handle(self.lib, self.mp, self.env, new_vol, self.seq.interp)
        if same and self.handles['main'].created_resident == old_bytes:
            self.recreate_same += 1

    def invariants(self, H, op, before, after):
        what = (self.seq.name, self.tag, op.kind, op.cls)
        assert after.out == H.out, what + ('output shape', after.out, H.out)
        if op.kind != 'recreate':
            assert after.built >= before.built and after.evicted >= before.evicted, what + ('counters went back',)
            if op.kind in ('extract', 'project'):
                assert after.out == before.out, what + ('output shape changed',)
        assert after.budget == H.budget, what + ('budget', after.budget, H.budget)
        if op.kind == 'project' and after.kernel == 7 and not H.has_helper:
            # the first fused projection makes the helper: nothing else may be added by this op
            assert after.built == before.built and before.resident < after.resident <= before.resident + H.created_resident, what + ('helper', before.resident, after.resident)
            H.floor += after.resident - before.resident
            H.has_helper = True
        if H.budget:
            assert after.resident <= max(H.budget, H.floor), what + ('over the budget', after.resident, H.budget)
        if op.kind == 'release_copies' or (op.kind == 'set_max_resident' and op.arg[0] == 'plain'):
            assert after.resident == H.floor, what + ('not back at the floor', after.resident, H.floor)
        assert after.resident >= H.floor, what + ('below the floor', after.resident, H.floor)


def describe(seq, i, op, info=None, err=None):
    return dict(family=seq.family, sequence=seq.name, seed=hs.SEED, index=i, kind=op.kind, handle=op.handle, cls=op.cls, flags=op.flags, f64=op.f64, keep=op.keep,
                device_out=op.device_out, out_shape=op.out_shape, last_kernel=None if info is None else info.kernel, err=err)


def check_against_model(seq, i, op, got, want, info):
    if op.kind == 'project':
        err = float(np.abs(got.astype(np.float64) - want).max())
    else:
        err = float(np.abs(got - want).max())
    key = (info.kernel, op.interp, op.edge)
    LEDGER['worst'][key] = max(LEDGER['worst'].get(key, 0.0), err / (op.out_shape[0] if op.kind == 'project' else 1))
    assert err <= hs.tolerance(op), describe(seq, i, op, info, err)
    if op.keep and op.kind in ('affine', 'affine_batch'):
        assert np.array_equal(got == hs.SENTINEL, want == hs.SENTINEL), describe(seq, i, op, info, 'the set of untouched voxels differs')
    else:
        assert not (got == GARBAGE).any(), describe(seq, i, op, info, 'voxels were not written')


def ntiles(info, out_shape):
    return int(np.prod([(s + t - 1) // t for s, t in zip(out_shape, info.tile)])) if all(info.tile) else 0


def note_main(seq, op, H, info, before, prev_fam):
    """The ledger's view of one transforming op of the main runner."""
    icls = 'linear' if op.interp == 'linear' else 'cubic'
    LEDGER['kernels'][info.kernel] += 1
    LEDGER['ops'][(seq.family, op.kind)] += 1
    if op.kind in ('affine', 'affine_batch') and info.kernel == 8:
        launches = len(op.m) if op.kind == 'affine_batch' else 1
        for _ in range(launches):
            LEDGER['quad_parity'][H.quad_launches & 1] += 1
            H.quad_launches += 1
    if seq.medium and op.handle == 'main' and op.kind == 'affine' and info.kernel in (6, 9):
        fam = 'block' if info.kernel == 9 else ('span' if icls == 'linear' else 'packed')
        if 0 < info.grid < ntiles(info, op.out_shape):
            LEDGER['queue_used'][fam] += 1
        if seq.family == 'P' and prev_fam and prev_fam != fam:
            LEDGER['transitions'][(prev_fam, fam)] += 1
    if seq.family == 'S' and op.cls.startswith('reorient') and op.handle == 'main':
        H.asked[op.cls] += 1
        if H.asked[op.cls] >= 4 and info.built > before.built:
            LEDGER['reorient_builds'] += 1


def queue_family(seq, op, info):
    if seq.medium and op.handle == 'main' and op.kind == 'affine' and info.kernel in (6, 9):
        return 'block' if info.kernel == 9 else ('span' if op.interp == 'linear' else 'packed')
    return None


def fresh_check(seq, i, op, main, got, info, monkeypatch):
    """The same op alone on a newly created handle with the same environment and output shape."""
    H = main.handles[op.handle]
    fresh = Runner.__new__(Runner)
    fresh.seq, fresh.tag, fresh.mp, fresh.env, fresh.flag_or, fresh.skip_policy, fresh.lib = seq, 'fresh', monkeypatch, main.env, 0, False, main.lib
    fh = Handle(main.lib, monkeypatch, main.env, H.vol, H.interp, H.edge, H.window)
    fresh.handles = {op.handle: fh}
    try:
        if fh.out != H.out:
            N.check(main.lib.vt_volume_set_output_shape(fh.h, *H.out), 'vt_volume_set_output_shape')
            fh.out = H.out
        alone, finfo, _ = fresh.run(op)
    finally:
        fh.close()
    assert (finfo.kernel, finfo.tile, finfo.grid) == (info.kernel, info.tile, info.grid), \
        describe(seq, i, op, info, ('route depends on history', (finfo.kernel, finfo.tile, finfo.grid), (info.kernel, info.tile, info.grid)))
    assert np.array_equal(alone, got), describe(seq, i, op, info, ('differs from a fresh handle by', float(np.abs(alone - got).max())))


def may_sample_a_reoriented_copy(op, info):
    """Finding of these sequences: last_kernel and last_tile do not identify the route of a general-matrix launch.  Where the output's w axis
    follows source axis 0 or 1 (handle_sequences.follows_axis) kinds 2 / 6 / 9 sample the axis-permuted copy if the handle holds it and the
    plain copy if not -- which the budget and the number of earlier requests decide -- with the taps added in another order: S-medium-linear,
    op `reorient1` after set_max_resident(plain), differed from its twin without policy ops by 1.8e-7 on the same kernel and tile.  Such
    launches are held to the oracle on both handles and compared bit for bit only under VT_NO_REORIENT."""
    if op.flags & N.NO_REORIENT or op.kind not in ('affine', 'affine_batch', 'project'):
        return False
    if op.kind != 'affine_batch' and info.kernel not in (2, 6, 9):       # (a queued batch reports the kernel of its last matrix only)
        return False
    return any(hs.follows_axis(m) != 2 for m in op.matrices())


SETTING_TWINS = (('VT_NO_PROJ_CACHE=1', {'VT_NO_PROJ_CACHE': '1'}, 0), ('VT_QUAD_PINGPONG=0', {'VT_QUAD_PINGPONG': '0'}, 0),
                 ('VT_QUAD_PINGPONG=2', {'VT_QUAD_PINGPONG': '2'}, 0), ('VT_NO_PLANSHARE', {}, N.NO_PLANSHARE))


def run_sequence(seq, monkeypatch, model, twins=False, fresh=False, policy_twin=False):
    RAN.add(seq.name)
    runners = []
    try:
        main = Runner(seq, 'main', monkeypatch)
        runners.append(main)
        if twins:
            for tag, env, flag_or in SETTING_TWINS:
                runners.append(Runner(seq, tag, monkeypatch, env_extra=env, flag_or=flag_or))
        if policy_twin:
            runners.append(Runner(seq, 'no policy ops', monkeypatch, skip_policy=True))
        prev_fam = None                     # queue family of the main handle's previous launch (ops that launch nothing on it keep it)
        for i, op in enumerate(seq.ops):
            got, info, before = main.run(op)
            if op.kind == 'recreate':
                prev_fam = None
            want = None
            if op.transforms:
                want = model.expected(op)
                check_against_model(seq, i, op, got, want, info)
                note_main(seq, op, main.handles[op.handle], info, before, prev_fam)
                if op.handle == 'main':
                    prev_fam = queue_family(seq, op, info)
                if fresh:
                    fresh_check(seq, i, op, main, got, info, monkeypatch)
            for r in runners[1:]:
                if r.skip_policy and op.kind in ('set_max_resident', 'release_copies', 'device_trim'):
                    continue
                tgot, tinfo, _ = r.run(op)
                if not op.transforms:
                    continue
                if r.skip_policy:
                    check_against_model(seq, i, op, tgot, want, tinfo)
                    LEDGER['twin_ops'] += 1
                    if (tinfo.kernel, tinfo.tile) == (info.kernel, info.tile) and not may_sample_a_reoriented_copy(op, info):
                        assert np.array_equal(tgot, got), describe(seq, i, op, info, ('differs from the twin without policy ops by', float(np.abs(tgot - got).max())))
                        LEDGER['twin_bits']['span' if (info.kernel == 6 and op.interp == 'linear') else info.kernel] += 1
                else:
                    assert np.array_equal(tgot, got), describe(seq, i, op, info, (r.tag, 'changes the result by', float(np.abs(tgot - got).max()), 'twin kernel', tinfo.kernel))
        if seq.family == 'S':
            LEDGER['evictions'] += main.evicted_before + main.handles['main'].info().evicted
        LEDGER['recreate_same'] += main.recreate_same
    finally:
        for r in runners:
            r.close()


@pytest.fixture(scope='module')
def model():
    return hs.Model()


def _ids(family):
    seqs = hs.sequences(family)
    for s in seqs:
        ALL.add(s.name)
    return seqs


@pytest.mark.parametrize('seq', _ids('P-small') + _ids('P-medium'), ids=lambda s: s.name)
def test_pure_sequences_match_the_oracle_a_fresh_handle_and_their_twins(seq, monkeypatch, model):
    run_sequence(seq, monkeypatch, model, twins=True, fresh=True)


@pytest.mark.parametrize('seq', _ids('S'), ids=lambda s: s.name)
def test_policy_sequences_match_the_oracle_and_their_twins(seq, monkeypatch, model):
    run_sequence(seq, monkeypatch, model, twins=True, policy_twin=True)


@pytest.mark.parametrize('seq', _ids('E'), ids=lambda s: s.name)
def test_edge_scipy_sequences_match_scipy_and_a_fresh_handle(seq, monkeypatch, model):
    run_sequence(seq, monkeypatch, model, fresh=True)


@pytest.mark.parametrize('seq', _ids('L'), ids=lambda s: s.name)
def test_slab_sequences_match_the_oracle(seq, monkeypatch, model):
    run_sequence(seq, monkeypatch, model)


def test_recycled_allocation_reads_zero_in_pad_columns_and_staging(monkeypatch, model):
    """The shortest form of `recreate`: a handle of 1e3 values is destroyed, the next handle of another shape and the same allocation size
    takes its buffers from the recycler (emptied first, so that they are the outgoing handle's own), and a transform whose last output
    column taps the first pad column must see 0 there."""
    for interp in ('linear', 'filt_bspline'):
        g = hs._gen('P', 'recycle-%s' % interp, interp, hs.Vol((41, 70, 133), 900))
        g.simple('device_trim')             # (the recycler holds nothing else: the first match IS the outgoing buffer)
        g.recreate()
        for flags in (hs.BOXES_FLAGS, hs.PACKED, hs.FT | N.NO_ZSEP, 0):       # boxes, packed footprints, lane blocks / boxes, default dispatch
            g.affine(cls='pad_probe', flags=flags, keep=False, device_out=False, f64=False)
        seq = g.finish(hs.P_ENV)
        ALL.add(seq.name)
        before = LEDGER['recreate_same']
        run_sequence(seq, monkeypatch, model, fresh=True)
        assert LEDGER['recreate_same'] == before + 1


def ledger_report():
    L = LEDGER
    lines = ['sequence ledger (main runners)',
             'ops per (family, kind): ' + ', '.join(f'{k[0]}/{k[1]}: {v}' for k, v in sorted(L['ops'].items())),
             'last_kernel counts: ' + ', '.join(f'{k}: {v}' for k, v in sorted(L['kernels'].items())),
             'plane-quad launches by parity of launch_no: ' + ', '.join(f'{"even" if k == 0 else "odd"}: {v}' for k, v in sorted(L['quad_parity'].items())),
             f'evictions in S: {L["evictions"]}; reorientation copies built at a fourth-or-later request in S: {L["reorient_builds"]}',
             f'recreates that took over an allocation of the same size: {L["recreate_same"]}',
             'medium handle, launches with fewer workgroups than tiles: ' + ', '.join(f'{k}: {v}' for k, v in sorted(L['queue_used'].items())),
             'medium handle (P), consecutive launches of different queue families: ' + ', '.join(f'{a}->{b}: {v}' for (a, b), v in sorted(L['transitions'].items())),
             f'S twin without policy ops: {L["twin_ops"]} ops, compared bit for bit per kernel: ' + ', '.join(f'{k}: {v}' for k, v in sorted(L['twin_bits'].items(), key=str)),
             'largest |got - expected| per (kernel, interpolation, edge), projections per plane: ' + ', '.join(f'{k}: {v:.2e}' for k, v in sorted(L['worst'].items()))]
    return '\n'.join(lines)


def test_zz_sequence_ledger():
    """The sequences did what they are for (summed over the main runners of the whole file).  Last in the file; skips itself when only a
    selection of the file ran."""
    print('\n' + ledger_report())
    if RAN != ALL:
        pytest.skip(f'only {len(RAN)} of {len(ALL)} sequences ran: the ledger describes a selection')
    L = LEDGER
    assert not {1, 2, 6, 7, 8, 9, 10, 11} - set(L['kernels']), sorted(L['kernels'])
    assert L['evictions'] > 0
    assert L['reorient_builds'] > 0
    assert L['quad_parity'][0] > 0 and L['quad_parity'][1] > 0
    assert L['recreate_same'] > 0
    # the persistent kernels' grids were smaller than their tile counts (the shared counters were really used), and every pair of
    # different families that one handle can run occurred back to back
    assert all(L['queue_used'][fam] > 0 for fam in ('block', 'span', 'packed')), dict(L['queue_used'])
    assert all(L['transitions'][pair] > 0 for pair in hs.QUEUE_PAIRS), dict(L['transitions'])
    # the twin of S without policy ops was compared bit for bit on the plane-quad, lane-block and packed-span kernels
    assert all(L['twin_bits'][k] > 0 for k in (8, 9, 'span')), dict(L['twin_bits'])
