"""-m gpu: every ordered pair of the batched entry points as neighbours on ONE handle (tests/batch_pair_cases.py: an Eulerian circuit
over the families, a seeded variant per step, the adjacencies that tests/test_batch_pair_cases_host.py holds it to).  The sixteen
families share the host staging vector, its device copy, the float64 partials and the result staging buffer; each reads the vector as
tables of its own, and what a call does not write keeps what the call before it left.  Per step of the walk:

  * the result equals the same call on a fresh handle bit for bit (uint8 views; the fresh result is computed once per variant), and so
    does the launch record of info(); a refusal gives the fresh handle's text and leaves the record as it was;
  * a device output is read only after the NEXT step has returned -- that call may regrow the device table or free and reallocate the
    partials while this one's reduction is still queued; the last step is read after synchronize();
  * info()'s output shape is what it was, and on the two linear handles every 16th step is followed by a plain affine() into a host
    array whose bits are a fresh handle's (the staging buffer shared through host_output_buffer);
  * the first occurrence of a variant of warp, affine_stack, warp_stack, filter_stack, correlate_stack and moments_stack is held to that
    family's float64 model with the tolerance of its own suite (TOL of tests/test_gpu_extract.py times |w|, the models' derived bounds),
    so that fresh and reused cannot be wrong together;
  * results are finite, and a call that does not accumulate overwrote its prefilled output.

A failure names the step and the pair: (#131 filter_stack[...] -> correlate_stack[...])."""
import numpy as np
import pytest

import batch_pair_cases as bpc
from test_gpu_batch_sequences import record
from test_gpu_extract import TOL

pytestmark = pytest.mark.gpu


def out_shape(sv):
    i = sv.info()
    return (i.out_depth, i.out_height, i.out_width)


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint8), want.view(np.uint8))


@pytest.mark.parametrize('handle', list(bpc.HANDLES))
def test_every_ordered_pair_of_batched_calls_on_one_handle(handle, monkeypatch):
    h = bpc.HANDLES[handle]
    walk, vol, tol = bpc.steps(handle), bpc.volume(), TOL[h.interpolation]
    create = lambda: h.create(monkeypatch.setenv, monkeypatch.delenv)
    fresh, checked = {}, set()

    def on_a_fresh_handle(v):
        """(result or refusal text, record) of the variant alone on a new handle, once."""
        if v.name not in fresh:
            one = create()
            try:
                before = record(one)
                res = v.step(one)
                fresh[v.name] = (res, before if v.refusal else record(one))
            finally:
                one.close()
        return fresh[v.name]

    def affine_into_host(sv):
        out = np.full(bpc.VOLUME, bpc.PREFILL, np.float32)
        sv.affine(bpc.affine_check_matrix(), output=out)
        return out

    def settle(label, v, fetch, rec, before):
        got = fetch()
        want, want_rec = on_a_fresh_handle(v)
        if v.refusal:
            assert got == want and rec == before, (label, got, want, rec, before)
            assert v.family == 'refused' or 'is not finite' in got, (label, got)
            return
        assert same_bits(got, want), (label, got.shape, want.shape, int((got.view(np.uint8) != want.view(np.uint8)).sum())
                                      if got.shape == want.shape and got.dtype == want.dtype else None)
        assert rec == want_rec, (label, rec, want_rec)
        assert np.isfinite(got).all(), label
        assert v.accumulate or (got != bpc.PREFILL).any(), label
        if v.truth is not None and v.name not in checked:
            checked.add(v.name)
            v.truth(got, vol, h.interpolation, tol)

    sv = create()
    try:
        shape0 = out_shape(sv)
        assert shape0 == bpc.VOLUME
        plain = h.interpolation == 'linear'
        if plain:
            one = create()
            try:
                affine_want = affine_into_host(one)
            finally:
                one.close()
            assert np.isfinite(affine_want).all() and (affine_want != 0).any() and (affine_want != bpc.PREFILL).all()
        pending, prev = None, None
        for i, v in enumerate(walk):
            label = f'(#{i} {prev.name if prev else "a new handle"} -> {v.name})'
            before = record(sv)
            fetch = v.launch(sv)
            rec = record(sv)
            assert out_shape(sv) == shape0, label
            if pending is not None:                          # the step before wrote a device array: read now that this call has returned
                settle(*pending)
                pending = None
            if v.device and not v.refusal:
                pending = (label, v, fetch, rec, before)
            else:
                settle(label, v, fetch, rec, before)
            if plain and i % 16 == 15:
                assert same_bits(affine_into_host(sv), affine_want), ('affine after', label)
                assert out_shape(sv) == shape0, label
            prev = v
        sv.synchronize()
        if pending is not None:
            settle(*pending)
        used = {v.name for v in walk}
        assert set(fresh) == used and checked == {v.name for v in walk if v.truth is not None}
    finally:
        sv.close()
