"""Host side of the handle sequences (tests/handle_sequences.py): the coverage conditions the generator promises, and the stateless model.

No GPU.  What tests/test_gpu_sequences.py holds the library to is only worth something if the sequences really interleave every kind of
call, reach every flag set, never pass on zeros, and if the expected value of an op is a function of its record alone."""
import collections

import numpy as np
import pytest

import handle_sequences as hs
import voltools_amd as vt
from test_gpu_fuzz import FLAG_SETS as FUZZ_FLAG_SETS
from test_gpu_edge_scipy import TOL as TOL_SCIPY


def all_sequences():
    return [s for fam in ('P', 'S', 'E', 'L') for s in hs.sequences(fam)]


def test_generation_is_deterministic():
    first = {fam: hs.sequences(fam) for fam in ('P-small', 'P-medium', 'S', 'E', 'L')}
    hs._CACHE.clear()
    try:
        for fam in ('P-medium', 'E', 'L', 'S', 'P-small'):          # (another order: a sequence depends on its name alone)
            again = hs.sequences(fam)
            assert again == first[fam], fam
    finally:
        hs._CACHE.update(first)


def test_sequence_lengths_and_families():
    small, medium = hs.sequences('P-small'), hs.sequences('P-medium')
    assert {(s.vol.shape, s.interp) for s in small} == {(sh, i) for sh in hs.SMALL_SHAPES for i in hs.ALL_INTERPS}
    assert all(45 <= len(s.ops) <= 70 for s in small), [len(s.ops) for s in small]
    assert [s.interp for s in medium] == ['linear', 'bspline', 'filt_bspline'] and all(20 <= len(s.ops) <= 30 for s in medium)
    assert [s.interp for s in hs.sequences('S')] == ['linear', 'filt_bspline'] and all(35 <= len(s.ops) <= 45 for s in hs.sequences('S'))
    for s in small + medium:
        assert dict(s.env).get('VT_REORIENT') == '0' and not any(op.kind == 'set_max_resident' for op in s.ops), s.name
    for s in hs.sequences('S'):
        assert 'VT_REORIENT' not in dict(s.env)
        assert {op.cls for op in s.ops if op.kind == 'set_max_resident'} == {'0', 'plain', '2.6'}
        assert {'release_copies', 'device_trim', 'recreate', 'set_output_shape'} <= {op.kind for op in s.ops}
    assert all(s.edge == 'scipy' and {op.kind for op in s.ops} == set(hs.TRANSFORMS) for s in hs.sequences('E'))
    assert all(s.window and {op.kind for op in s.ops} == {'affine', 'project', 'set_output_shape'} for s in hs.sequences('L'))


def test_every_ordered_pair_of_op_kinds_is_consecutive_somewhere_in_family_p():
    seen = set()
    for s in hs.sequences('P'):
        kinds = [op.cov_kind for op in s.ops]
        seen.update(zip(kinds, kinds[1:]))
    want = {(a, b) for a in hs.P_KINDS for b in hs.P_KINDS} - set(hs.IMPOSSIBLE_KIND_PAIRS)
    assert not want - seen, sorted(want - seen)


def test_every_possible_pair_of_queue_families_is_consecutive_on_the_medium_handle():
    seen = set()
    for s in hs.sequences('P-medium'):
        assert dict(s.env).get('VT_BLOCK_MIN') and (s.interp != 'linear' or dict(s.env).get('VT_BLOCK_LINEAR') == '1')
        ops = [op for op in s.ops if op.handle == 'main']
        for a, b in zip(ops, ops[1:]):
            if a.qfam and b.qfam and a.qfam != b.qfam and a.vol == b.vol:
                seen.add((a.qfam, b.qfam))
    assert seen == set(hs.QUEUE_PAIRS), seen
    assert set(hs.QUEUE_PAIRS) | set(hs.IMPOSSIBLE_QUEUE_PAIRS) == {(a, b) for a in ('block', 'span', 'packed') for b in ('block', 'span', 'packed') if a != b}


def test_every_flag_set_and_argument_form_occurs():
    ops = [op for s in hs.sequences('P') for op in s.ops]
    aff = [op for op in ops if op.kind == 'affine']
    flags = {op.flags for op in aff}
    assert not {int(f) for f in FUZZ_FLAG_SETS} - flags
    assert not set(hs.PARITY_FLAG_SETS) - flags
    for bit in (hs.N.NO_PLANSHARE, hs.N.NO_ZFIR, hs.N.NO_ROWS, hs.N.NO_REORIENT):
        assert any(f & bit for f in flags), bit
    for field in ('f64', 'device_out', 'keep'):
        assert {getattr(op, field) for op in aff} == {False, True}, field
    classes = {op.cls.split(':')[0] for op in aff}
    assert {'parity', 'fuzz', 'lattice'} <= classes
    small = [op for s in hs.sequences('P-small') for op in s.ops]
    medium = [op for s in hs.sequences('P-medium') for op in s.ops]
    for group in (small, medium):
        assert {len(op.m) for op in group if op.kind == 'affine_batch'} == {1, 3, 7}
    assert all(np.prod(op.out_shape) > 96 ** 3 for op in medium if op.kind == 'affine_batch' and op.handle == 'main')
    assert any(np.prod(op.out_shape) <= 96 ** 3 for op in small if op.kind == 'affine_batch')
    ext = [op for op in ops if op.kind == 'extract']
    assert {len(op.m) for op in ext} == {1, 5} and {op.out_shape for op in ext} == set(hs.BOXES)
    assert {op.flags for op in ext} == {0, hs.N.FORCE_TILED, hs.N.FORCE_DIRECT} and {op.f64 for op in ext} == {False, True}
    assert {op.cls for op in ops if op.kind == 'project'} == {'proj_hit', 'proj_new_tz', 'proj_new_inplane', 'proj_general'}
    assert {op.cls for op in ops if op.kind == 'set_output_shape'} == {'larger', 'smaller', 'source'}


def test_projection_patterns_that_need_the_cache_key():
    """In every P sequence: a fused projection, a change of the output depth, and a fused projection with the SAME tz (the plane sum must
    be rebuilt: it covers other planes); and two fused projections in a row whose tz differ on one output depth."""
    for s in hs.sequences('P-small'):
        ops = [op for op in s.ops if op.handle == 'main' and op.kind in ('project', 'set_output_shape', 'recreate')]
        depth_change = tz_change = False
        for a, b, c in zip(ops, ops[1:], ops[2:]):
            if a.kind == c.kind == 'project' and b.kind == 'set_output_shape' and 'general' not in a.cls + c.cls:
                depth_change |= a.m[0][3] == c.m[0][3] and c.out_shape[0] < a.out_shape[0] and a.vol == c.vol
        for a, b in zip(ops, ops[1:]):
            if a.kind == b.kind == 'project' and 'general' not in a.cls + b.cls:
                tz_change |= a.m[0][3] != b.m[0][3] and a.out_shape == b.out_shape and a.vol == b.vol
        assert depth_change and tz_change, s.name


def test_recreate_reuses_the_allocation_by_the_rule_of_the_recycler():
    for shape in hs.SMALL_SHAPES + (hs.MEDIUM_SHAPE,):
        d = hs.dirty_shape(shape)
        assert d != shape and d[2] > shape[2] and hs.resident_bytes(d) == hs.resident_bytes(shape)
    for s in hs.sequences('P') + hs.sequences('S'):
        rec = [op for op in s.ops if op.kind == 'recreate']
        assert rec, s.name
        for op in rec:
            dirty, new = op.arg
            assert dirty.scale == 1.0e3 and new.scale == 1.0 and hs.resident_bytes(dirty.shape) == hs.resident_bytes(new.shape)
            i = s.ops.index(op)
            later = [j for j in range(i + 1, len(s.ops)) if s.ops[j].kind == 'recreate']
            nxt = s.ops[i + 1:later[0] if later else None]
            assert all(o.vol == new for o in nxt if o.handle == 'main')


def test_no_transforming_op_passes_on_zeros():
    worst = 1.0
    for s in all_sequences():
        for i, op in enumerate(s.ops):
            if not op.transforms or op.exempt:
                continue
            for m in op.matrices():
                if op.window:           # the slab's output planes against the global volume
                    m = m.copy()
                    m[:3, 3] += m[:3, 0] * op.window[3]
                share = hs.inside_share(m, op.out_shape, op.vol.shape)
                worst = min(worst, share)
                assert share >= 0.10, (s.name, i, op.kind, op.cls, share)
    assert worst >= 0.10


@pytest.fixture(scope='module')
def small_expected():
    """The expected values of the small-handle sequences of P and of E, in sequence order (computed once)."""
    model = hs.Model()
    return {s.name: [model.expected(op) if op.transforms else None for op in s.ops] for s in hs.sequences('P-small') + hs.sequences('E')}


def test_expected_values_do_not_depend_on_the_position_of_an_op(small_expected):
    rs = np.random.RandomState(hs.SEED)
    n = 0
    for s in hs.sequences('P-small') + hs.sequences('E'):
        model = hs.Model()                  # (a fresh one: nothing carried over from the in-order evaluation)
        for i in rs.permutation(len(s.ops)):
            op = s.ops[i]
            if op.transforms:
                n += 1
                assert np.array_equal(model.expected(op), small_expected[s.name][i]), (s.name, i, op.kind, op.cls)
    assert n > 300


def test_expected_values_are_not_trivial_and_keep_ops_hold_the_sentinel(small_expected):
    kept = collections.Counter()
    for s in hs.sequences('P-small'):
        for op, want in zip(s.ops, small_expected[s.name]):
            if want is None:
                continue
            assert np.isfinite(want).all()
            if not op.exempt:
                assert np.count_nonzero(want) >= 0.05 * want.size, (s.name, op.kind, op.cls)
            if op.keep:
                kept[bool((want == hs.SENTINEL).any())] += 1
    assert kept[True] > 0


def test_scipy_family_model_is_the_cpu_device(small_expected):
    n = 0
    for s in hs.sequences('E'):
        vol = s.vol.make()
        for op, want in zip(s.ops, small_expected[s.name]):
            if op.kind == 'affine':
                n += 1
                ref = vt.affine(vol, op.matrices()[0], interpolation=op.interp, device='cpu')
                assert np.abs(want - ref).max() <= TOL_SCIPY[op.interp], (s.name, op.cls)
            elif op.kind == 'project':
                ref = vt.affine(vol, op.matrices()[0], interpolation=op.interp, device='cpu').astype(np.float64).sum(axis=0)
                assert np.abs(want - ref).max() <= TOL_SCIPY[op.interp] * op.out_shape[0], (s.name, op.cls)
    assert n >= 8
