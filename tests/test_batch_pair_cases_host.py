"""No GPU: holds tests/batch_pair_cases.py to what tests/test_gpu_batch_pairs.py relies on, so that the GPU test cannot quietly cover
less than it claims -- the circuit visits every ordered pair of families, the seeded draw is deterministic and meets, as adjacencies, the
conditions under which one call could trip over what another left in the shared scratch (told from the case data: table lengths in
doubles, partial bytes from the plan modules), the pools hold the variants they promise, and every step of the `linear` walk is a valid
call: it runs on device='cpu'."""
import re

import numpy as np
import pytest

import voltools_amd as vt

import batch_pair_cases as bpc
import correlate_stack_model as csm
import moments_stack_model as msm

HANDLES = list(bpc.HANDLES)


def count_of(v):
    """The n of a variant (nb x n for backproject_boxes: the entries of its table), None for warp."""
    m = re.search(r'(\d+)x(\d+)', v.tag) if v.family == 'backproject_boxes' else re.search(r'n=(\d+)', v.tag)
    return None if m is None else int(np.prod([int(g) for g in m.groups()]))


# ---- the circuit -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('handle', HANDLES)
def test_the_circuit_visits_every_ordered_pair_once_and_is_deterministic(handle):
    h = bpc.HANDLES[handle]
    fams = bpc.circuit(h.families, h.seed)
    F = len(h.families)
    assert len(fams) == F * F + 1 and fams[0] == fams[-1]
    pairs = list(zip(fams, fams[1:]))
    assert len(set(pairs)) == F * F and set(pairs) == {(a, b) for a in h.families for b in h.families}
    assert fams == bpc.circuit(h.families, h.seed)
    assert fams != bpc.circuit(h.families, h.seed + 100)
    walk, again = bpc.steps(handle), bpc.steps.__wrapped__(handle)
    assert [v.name for v in walk] == [v.name for v in again] and all(a is b for a, b in zip(walk, again))
    assert len(walk) == F * F + 1 + len(bpc.REGRESSIONS[handle])
    assert [v.family for v in walk[len(bpc.REGRESSIONS[handle]):]] == fams


def test_the_four_handles_and_their_families():
    H = bpc.HANDLES
    assert HANDLES == ['linear', 'linear_split', 'filt_stack', 'filt_3d']
    assert len(bpc.FAMILIES) == 16 and H['linear'].families == bpc.FAMILIES == H['linear_split'].families
    assert (H['linear'].interpolation, H['linear'].stack, H['linear'].cap) == ('linear', False, 0)
    assert (H['linear_split'].interpolation, H['linear_split'].stack) == ('linear', False) and H['linear_split'].cap > 0
    assert (H['filt_stack'].interpolation, H['filt_stack'].stack) == ('filt_bspline', True)
    assert set(H['filt_stack'].families) == {'affine_stack', 'warp_stack', 'backproject', 'backproject_boxes', 'refused'}
    assert {v.tag.split(' ')[0] for v in bpc.all_pools()['refused']} == {'filter_stack', 'correlate_stack', 'moments_stack'}
    assert (H['filt_3d'].interpolation, H['filt_3d'].stack) == ('filt_bspline', False)
    assert set(H['filt_3d'].families) == {'affine_batch', 'extract', 'projection_batch', 'extract_sum', 'extract_dot', 'extract_dot_multi',
                                          'extract_sum_multi', 'place', 'warp'}


# ---- the adjacencies, from the case data ------------------------------------------------------------------------------------------------
def neighbours(handle):
    walk = bpc.steps(handle)
    return list(zip(walk, walk[1:]))


def holds(handle, what):
    assert any(what(a, b) for a, b in neighbours(handle)), handle


@pytest.mark.parametrize('handle', HANDLES)
def test_every_ordered_pair_of_families_is_adjacent(handle):
    h = bpc.HANDLES[handle]
    assert {(a.family, b.family) for a, b in neighbours(handle)} == {(a, b) for a in h.families for b in h.families}


@pytest.mark.parametrize('handle', HANDLES)
def test_tables_and_output_kinds_change_between_neighbours(handle):
    served = lambda a, b: not a.refusal and not b.refusal
    small, large = bpc.SMALL_TABLE, bpc.LARGE_TABLE
    assert small <= 2 * bpc.ENTRY and large >= 36 * (bpc.ENTRY + 1)
    holds(handle, lambda a, b: served(a, b) and a.table <= small and b.table >= large)
    holds(handle, lambda a, b: served(a, b) and a.table >= large and b.table <= small)
    holds(handle, lambda a, b: served(a, b) and a.device and not b.device)
    holds(handle, lambda a, b: served(a, b) and not a.device and b.device)
    holds(handle, lambda a, b: served(a, b) and not a.accumulate and b.accumulate)


@pytest.mark.parametrize('handle', ['linear', 'linear_split', 'filt_3d'])
def test_partials_and_result_types_change_between_neighbours(handle):
    h = bpc.HANDLES[handle]
    served = lambda a, b: not a.refusal and not b.refusal
    largest = max(h.partial_bytes(v) for v in bpc.steps(handle))
    assert largest >= 100 * 1024
    holds(handle, lambda a, b: served(a, b) and h.partial_bytes(a) == 0 and h.partial_bytes(b) == largest)
    holds(handle, lambda a, b: served(a, b) and h.partial_bytes(a) == largest and h.partial_bytes(b) == 0)
    holds(handle, lambda a, b: served(a, b) and not a.f64 and b.f64)
    holds(handle, lambda a, b: served(a, b) and a.f64 and not b.f64)


@pytest.mark.parametrize('handle', ['linear', 'linear_split'])
def test_odd_references_and_late_refusals_have_their_neighbours(handle):
    holds(handle, lambda a, b: b.family == 'correlate_stack' and b.odd_refs and a.table > b.table)
    for follower in ('correlate_stack', 'filter_stack', 'extract_dot'):
        holds(handle, lambda a, b: a.late_refusal and b.family == follower and not b.refusal)


def test_the_filt_stack_walk_interleaves_the_refused_calls():
    walk = bpc.steps('filt_stack')
    assert {v.name for v in walk if v.family == 'refused'} == {v.name for v in bpc.all_pools()['refused']}
    holds('filt_stack', lambda a, b: a.family == 'refused' and b.family == 'warp_stack' and not b.refusal)
    holds('filt_stack', lambda a, b: a.late_refusal and not b.refusal)
    for fam in bpc.BACK:
        holds('filt_stack', lambda a, b: a.family == 'refused' and b.family == fam)
        holds('filt_stack', lambda a, b: a.family == fam and b.family == 'refused')


@pytest.mark.parametrize('handle', HANDLES)
def test_the_generator_reports_the_conditions_it_was_asked_for(handle):
    found = bpc.adjacencies(handle, bpc.steps(handle))
    assert all(k in found for k in bpc.REQUIRED[handle]), [k for k in bpc.REQUIRED[handle] if k not in found]


def test_the_long_walks_use_every_variant():
    for handle in ('linear', 'linear_split'):
        used = {v.name for v in bpc.steps(handle)}
        assert used == {v.name for f in bpc.FAMILIES for v in bpc.all_pools()[f]}


# ---- the pools --------------------------------------------------------------------------------------------------------------------------
def test_pools_hold_both_table_sizes_both_outputs_and_accumulation():
    pools = bpc.all_pools()
    for fam in bpc.FAMILIES:
        pool = [v for v in pools[fam] if not v.refusal]
        assert 3 <= len(pool) <= 6, fam
        assert {v.device for v in pool} == {True, False}, fam
        assert all(v.f64 == (fam in ('extract_dot', 'extract_dot_multi', 'correlate_stack', 'moments_stack')) for v in pool), fam
        if fam in bpc.TAKES_N:
            counts = [count_of(v) for v in pool]
            assert min(counts) == 1 and max(counts) >= 40, (fam, counts)
    shapes = {tuple(int(g) for g in re.search(r'(\d+)x(\d+)', v.tag).groups()) for v in pools['backproject_boxes']}
    assert any(nb == 1 and n <= 4 for nb, n in shapes) and any(nb >= 3 and n >= 3 for nb, n in shapes)
    for fam in ('place', 'backproject', 'backproject_boxes'):
        assert {v.accumulate for v in pools[fam]} == {True, False}, fam
        assert {v.device for v in pools[fam] if v.accumulate} == {True, False}, fam


@pytest.mark.parametrize('cubic', [False, True])
def test_pools_hold_the_fewest_and_the_most_partials(cubic):
    pools = bpc.all_pools()
    for fam in bpc.USES_PARTIALS:
        sizes = sorted(v.partial_bytes(cubic) for v in pools[fam])
        assert sizes[-1] >= 30 * max(sizes[0], 16), (fam, sizes)
        if fam in ('extract_sum', 'extract_sum_multi', 'projection_batch', 'correlate_stack'):        # one segment, one piece: none at all
            assert sizes[0] == 0, (fam, sizes)
    for fam in bpc.FAMILIES:
        if fam not in bpc.USES_PARTIALS:
            assert all(v.partial_bytes(cubic) == 0 for v in pools[fam]), fam
    # a one-piece patch grid and the (1, 1) grid of 2 x 3 pieces under the window (2, 7)
    assert csm.plan(bpc.H, bpc.W, (1, 2), (3, 5))['pieces'] == 1 and csm.plan(bpc.H, bpc.W, (2, 7), (1, 1))['pieces'] == 6
    assert any('grid 3x5' in v.tag and v.partial_bytes() == 0 for v in pools['correlate_stack'])
    assert any('grid 1x1,window 2x7' in v.tag and v.partial_bytes() > 0 for v in pools['correlate_stack'])
    assert any('grid 1x1,window 2x7' in v.tag for v in pools['moments_stack']) and any('grid 3x5' in v.tag for v in pools['moments_stack'])


def test_pools_hold_the_table_layouts_of_the_stack_families():
    pools = bpc.all_pools()
    corr = pools['correlate_stack']
    odd = [v for v in corr if v.odd_refs]
    assert odd and all(v.ref_floats % 2 == 1 and 2 * (v.table - count_of(v)) == v.ref_floats + 1 for v in odd)
    assert any('planes' in v.tag and v.ref_floats == 0 for v in corr)
    assert (bpc.H * bpc.W) % 2 == 1 and {v.device for v in odd} == {True, False}
    filt = pools['filter_stack']
    assert {'axis1', 'axis2'} <= {t for v in filt for t in v.tag.split(',')}
    assert any('shared' in v.tag for v in filt) and any('rows' in v.tag for v in filt)
    assert (bpc.ZEROS9[1:-1] == 0).any() and bpc.ZEROS9[0] != 0 and bpc.ZEROS9[-1] != 0                  # interior zeros
    assert np.count_nonzero(bpc.ZEROS9) < bpc.ZEROS9.size
    ws = [v for v in pools['warp_stack'] if not v.refusal]
    assert all(count_of(v) % 2 == 1 for v in ws) and any('shared' in v.tag for v in ws) and any('own' in v.tag for v in ws)
    late = [v for v in pools['warp_stack'] if v.late_refusal]
    assert len(late) == 2 and all(v.refusal and v.table > 1000 for v in late)
    assert all(re.search(r'grid=\d+x\d+x\d+', v.tag) for v in pools['warp']) and 'warp' in bpc.HANDLES['linear'].families


def test_the_lowered_cap_splits_the_largest_correlate_and_moments_calls_three_ways():
    cap = bpc.HANDLES['linear_split'].cap
    assert 0 < cap < bpc.DEFAULT_CAP
    for fam, model in (('correlate_stack', csm), ('moments_stack', msm)):
        v = max(bpc.all_pools()[fam], key=lambda v: v.partial_bytes())
        shift, grid, n = v.launch_plan
        units = n * (grid[0] * grid[1] if fam == 'correlate_stack' else 1)
        per, last = model.launches(bpc.H, bpc.W, shift, grid, n, cap)
        assert -(-units // per) >= 3 and 1 <= last <= per, (fam, units, per)
        assert model.launches(bpc.H, bpc.W, shift, grid, n)[0] == units                                   # one launch under the default cap


# ---- every step of the linear walk is a valid call -------------------------------------------------------------------------------------
def test_every_step_of_the_linear_walk_runs_on_the_cpu():
    sv = vt.StaticVolume(bpc.volume(), interpolation='linear', device='cpu')
    seen = {}
    for v in bpc.steps('linear'):
        if v.name in seen:
            continue
        if v.refusal:
            seen[v.name] = v.refuse(sv)
            assert 'finite' in seen[v.name], v.name
            continue
        got = seen[v.name] = v.launch(sv, device=False)()
        assert got.shape == v.shape and got.dtype == (np.float64 if v.f64 else np.float32), v.name
        assert np.isfinite(got).all(), v.name
        if v.accumulate and 'outside' in v.tag:
            assert np.array_equal(got, v.base), v.name
        else:
            assert (got != bpc.PREFILL).any() and (got != 0).any(), v.name
            assert v.base is None or not np.array_equal(got, v.base), v.name
    assert len(seen) == len({v.name for f in bpc.FAMILIES for v in bpc.all_pools()[f]})
