"""-m gpu: StaticVolume.correlate_stack (vt_volume_correlate_stack, kernel 24): shift scores of every image of a resident stack against
a reference, per patch of a grid.  The definition, the per-score bound (N + 2) 2^-53 sum |r s| and the kernel's plan are
tests/correlate_stack_model.py's, the cases tests/correlate_stack_cases.py's; every score is held to the bound.  Bit identities are
compared as uint64.

Out of reach of a test: the refusals for workgroups or partial sums of one patch at or above 2^31 and for more than 2^30 host
reference pixels need handles of several GiB; the output bound is reached through n alone."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import correlate_stack_model as csm
import correlate_stack_cases as csc

pytestmark = pytest.mark.gpu

VT_EINVAL, VT_EUNSUPPORTED = 10001, 10004


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def handle(src, interp='linear', **kw):
    return vt.StaticVolume(src, interpolation=interp, device='gpu:0', **kw)


@functools.lru_cache(maxsize=None)
def modelled(name, integers=False):
    c = next(c for c in csc.CASES if c['name'] == name)
    s, refs, kw = csc.arguments(c, integers)
    return csm.model(s, refs, c['max_shift'], c['grid'], kw['planes'], kw.get('reference_planes'))


def run(sv, c, integers=False, **more):
    s, refs, kw = csc.arguments(c, integers)
    return sv.correlate_stack(refs, c['max_shift'], c['grid'], **kw, **more)


# ---- 1. every case against the model, on random data within the bound and on small integers exactly ---------------------------------------
@pytest.mark.parametrize('stack_name', sorted(csc.SHAPES))
def test_cases_against_the_model(stack_name):
    for integers in (False, True):
        sv = handle(csc.stack(stack_name, integers))
        try:
            for c in csc.CASES:
                if c['stack'] != stack_name:
                    continue
                got = run(sv, c, integers)
                info = sv.info()
                assert info.last_kernel == 24
                vals, bounds = modelled(c['name'], integers)
                if integers:
                    # values in [-8, 8], at most 97 x 150 pixels per patch: every partial sum is an integer below 2^20, whatever the order
                    assert np.array_equal(got, vals), (c['name'], int((got != vals).sum()))
                else:
                    csm.check(got, vals, bounds, c['name'])
        finally:
            sv.close()


def test_sample_interpolations_and_stack_flag():
    c = next(c for c in csc.CASES if c['name'] == 'small-g35')
    want = None
    for interp in ('linear', 'bspline', 'bspline_simple'):
        for stack in (False, True):
            sv = handle(csc.stack('small'), interp, stack=stack)
            got = run(sv, c)
            sv.close()
            want = got if want is None else want
            assert same_bits(got, want), (interp, stack)
    csm.check(want, *modelled('small-g35'), 'interpolations')


def test_cross_check_against_extract_dot():
    """Independent device code on the same integer data: extract_dot with one integer translation per shift, a box (1, H, W) and the
    reference as template gives, in column 2, the (1, 1)-grid scores."""
    s = csc.stack('small', True)
    ref = csc.references('small', 1, True)[0]
    T, H, W = s.shape
    rh, rw = 2, 7
    sv = handle(s)
    try:
        got = sv.correlate_stack(ref, (rh, rw))
        ms = []
        for p in range(T):
            for u in range(2 * rh + 1):
                for v in range(2 * rw + 1):
                    m = np.eye(4)
                    m[:3, 3] = (p, u - rh, v - rw)
                    ms.append(m)
        dots = sv.extract_dot(np.array(ms), ref[None])
    finally:
        sv.close()
    assert np.array_equal(dots[:, 2].reshape(T, 1, 1, 2 * rh + 1, 2 * rw + 1), got)
    assert got.any()


# ---- 2. bit identities on random data -------------------------------------------------------------------------------------------------
def test_alone_in_a_batch_permuted_and_reference_routes():
    s = csc.stack('small')
    T, H, W = s.shape
    both = np.concatenate([s, csc.references('small', T)])                              # the references resident behind the images
    planes = np.array([3, 0, 4, 4, 1, 2, 0])
    n = len(planes)
    refs = both[T + planes % T]                                                         # entry i: reference planes[i]
    sv = handle(both)
    try:
        for shift, grid in (((2, 7), (1, 1)), ((3, 2), (3, 5)), ((1, 1), (19, 1))):
            whole = sv.correlate_stack(refs, shift, grid, planes=planes)
            csm.check(whole, *csm.model(both, refs, shift, grid, planes), ('batch', shift, grid))
            for i in range(n):                                                            # alone
                one = sv.correlate_stack(refs[i], shift, grid, planes=planes[i:i + 1])
                assert same_bits(one[0], whole[i]), (shift, grid, i)
            perm = np.random.default_rng(2).permutation(n)                                # permuted
            assert same_bits(sv.correlate_stack(refs[perm], shift, grid, planes=planes[perm]), whole[perm])
            # shared against per entry against resident, the same pixels
            shared = sv.correlate_stack(refs[1], shift, grid, planes=planes)
            own = sv.correlate_stack(np.stack([refs[1]] * n), shift, grid, planes=planes)
            res = sv.correlate_stack(max_shift=shift, patch_grid=grid, planes=planes, reference_planes=np.full(n, T + planes[1] % T))
            assert same_bits(shared, own) and same_bits(shared, res)
            assert same_bits(sv.correlate_stack(max_shift=shift, patch_grid=grid, planes=planes, reference_planes=T + planes % T), whole)
    finally:
        sv.close()


def test_host_and_device_output_repeats_and_recycled_memory():
    c = next(c for c in csc.CASES if c['name'] == 'pieces-r27')
    sv = handle(csc.stack('pieces'))
    try:
        want = run(sv, c)
        import torch                                                     # the project's plumbing: its absence is a failure, not a skip
        dev = torch.full(want.shape, 5.0, dtype=torch.float64, device='cuda:0')
        assert run(sv, c, output=dev) is None
        sv.synchronize()
        assert same_bits(dev.cpu().numpy(), want)
        with pytest.raises(ValueError):
            run(sv, c, output=torch.zeros(want.shape, dtype=torch.float32, device='cuda:0'))
        host = np.full(want.shape, np.nan)
        run(sv, c, output=host)
        assert same_bits(host, want)
        # other calls in between: they recycle the table buffer, the partials and the staging buffer
        small = next(c for c in csc.CASES if c['name'] == 'pieces-g35')
        first_small = run(sv, small)
        sv.filter_stack(np.array([0.25, 0.5, 0.25]))
        sv.extract_dot(np.eye(4)[None], np.ones((1, 8, 8), np.float32))
        assert same_bits(run(sv, c), want) and same_bits(run(sv, small), first_small)
        for _ in range(3):
            assert same_bits(run(sv, c), want)
    finally:
        sv.close()
    fresh = handle(csc.stack('pieces'))
    assert same_bits(run(fresh, c), want)
    fresh.close()


@pytest.mark.parametrize('stack_name,small,large,grid', [('small', (2, 3), (5, 11), (3, 5)), ('small', (0, 0), (18, 36), (1, 1)),
                                                          ('pieces', (1, 2), (12, 35), (1, 2)), ('pieces', (3, 0), (40, 3), (2, 1))])
def test_a_window_is_the_centre_of_a_larger_one(stack_name, small, large, grid):
    """The larger windows take other run lengths, runs per row and block counts."""
    s = csc.stack(stack_name)
    refs = csc.references(stack_name, s.shape[0])
    sv = handle(s)
    try:
        a = sv.correlate_stack(refs, small, grid)
        b = sv.correlate_stack(refs, large, grid)
    finally:
        sv.close()
    assert csm.plan(*s.shape[1:], small, grid) != csm.plan(*s.shape[1:], large, grid)
    du, dv = large[0] - small[0], large[1] - small[1]
    assert same_bits(a, b[:, :, :, du:du + 2 * small[0] + 1, dv:dv + 2 * small[1] + 1])


def test_a_patch_is_the_whole_of_its_cropped_stack():
    """Patch (a, b) of a grid against the (1, 1) grid of the stack cropped to that patch, at shift (0, 0), where nothing outside the
    patch is read: the order of additions starts from the patch's own first row and column."""
    s = csc.stack('pieces')
    refs = csc.references('pieces', s.shape[0])
    H, W = s.shape[1:]
    sv = handle(s)
    try:
        for grid in ((1, 2), (2, 1), (3, 5), (1, 1)):
            whole = sv.correlate_stack(refs, (0, 0), grid)
            ye, xe = vt.utils.patch_bounds(H, grid[0]), vt.utils.patch_bounds(W, grid[1])
            for a in range(grid[0]):
                for b in range(grid[1]):
                    ys, xs = slice(ye[a], ye[a + 1]), slice(xe[b], xe[b + 1])
                    crop = handle(np.ascontiguousarray(s[:, ys, xs]))
                    one = crop.correlate_stack(np.ascontiguousarray(refs[:, ys, xs]), (0, 0))
                    crop.close()
                    assert same_bits(one[:, 0, 0], whole[:, a, b]), (grid, a, b)
    finally:
        sv.close()


def test_split_launches_give_the_same_bits(monkeypatch):
    """The cap on one launch's partial sums is 64 MiB; VT_DOT_PART_CAP (read when the handle is created) lowers it so that the 5 units
    of this call go two per launch, and to one unit less than a single unit needs (one unit per launch at least)."""
    s = csc.stack('pieces')
    ref = csc.references('pieces', 1)[0]
    planes = [0, 1, 1, 0, 1]
    shift, grid = (3, 3), (1, 1)
    p = csm.plan(*s.shape[1:], shift, grid)
    assert p['pieces'] == 6 and p['unit_part_bytes'] == 6 * 49 * 8
    sv = handle(s)
    want = sv.correlate_stack(ref, shift, grid, planes=planes)
    assert sv.info().last_grid == 5 * p['unit_wgs']
    sv.close()
    csm.check(want, *csm.model(s, ref, shift, grid, planes), 'unsplit')
    for cap, per, last in ((2 * p['unit_part_bytes'], 2, 1), (p['unit_part_bytes'] - 8, 1, 1), (3 * p['unit_part_bytes'] + 8, 3, 2)):
        assert csm.launches(*s.shape[1:], shift, grid, 5, cap=cap) == (per, last)
        monkeypatch.setenv('VT_DOT_PART_CAP', str(cap))
        sv = handle(s)
        monkeypatch.delenv('VT_DOT_PART_CAP')
        got = sv.correlate_stack(ref, shift, grid, planes=planes)
        assert sv.info().last_grid == last * p['unit_wgs']
        sv.close()
        assert same_bits(got, want), cap


# ---- 3. non-finite data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('stack_name,shift,grid', [('small', (2, 7), (3, 5)), ('pieces', (3, 12), (2, 2))])
def test_non_finite_pixels(stack_name, shift, grid, value):
    """A non-finite image pixel reaches exactly the model's (patch, shift) pairs; a non-finite pixel of a resident reference takes its
    whole patch at every shift, since zeros outside the image are multiplied."""
    s = csc.stack(stack_name).copy()
    T, H, W = s.shape
    s[1, H // 3, W - 2] = value                                                          # near the edge: some windows miss it
    refs = csc.references(stack_name, 1)[0]
    sv = handle(s)
    try:
        got = sv.correlate_stack(refs, shift, grid)
        vals, bounds = csm.model(s, refs, shift, grid)
        assert np.isfinite(vals[[0] + list(range(2, T))]).all() and 0 < (~np.isfinite(vals[1])).sum() < vals[1].size
        csm.check(got, vals, bounds, ('image', value))
        # image 1 as the reference of image 0
        rp = np.array([1] + [0] * (T - 1))
        got = sv.correlate_stack(max_shift=shift, patch_grid=grid, reference_planes=rp)
        vals, bounds = csm.model(s, None, shift, grid, None, rp)
        ye, xe = csm.patch_edges(H, grid[0]), csm.patch_edges(W, grid[1])
        a = max(k for k in range(grid[0]) if ye[k] <= H // 3)
        bad = np.zeros(vals.shape, bool)
        bad[0, a, grid[1] - 1] = True
        bad[1:] = ~np.isfinite(vals[1:])                                                 # the entries that read image 1 as their image
        assert np.array_equal(~np.isfinite(vals), bad) and bad[1:].any()
        csm.check(got, vals, bounds, ('reference', value))
    finally:
        sv.close()


# ---- 4. info() against plan() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['small-r00', 'small-r27', 'small-full', 'small-g35', 'small-gHW', 'pieces-r27', 'pieces-g12', 'pieces-g35',
                                  'flat-full', 'thin-full', 'pieces-v-edge-32', 'pieces-v-edge-33', 'pieces-u-edge-31-0',
                                  'pieces-u-edge-32-0'])
def test_info_against_the_plan(name):
    c = next(c for c in csc.CASES if c['name'] == name)
    s, refs, kw = csc.arguments(c)
    n = s.shape[0] if kw['planes'] is None else len(kw['planes'])
    sv = handle(s)
    try:
        before = sv.info()
        run(sv, c)
        info = sv.info()
    finally:
        sv.close()
    p = csm.plan(*s.shape[1:], c['max_shift'], c['grid'], n)
    assert info.last_kernel == 24 and tuple(info.last_tile) == p['tile'] and tuple(info.last_lds_dims) == p['lds_dims']
    assert info.last_lds_bytes == p['lds_bytes'] <= csm.max_lds_bytes() and info.last_grid == p['grid']
    assert (info.out_depth, info.out_height, info.out_width) == (before.out_depth, before.out_height, before.out_width)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    s = csc.stack('small')
    T, H, W = s.shape
    ref = csc.references('small', 1)[0]
    out = np.zeros((1, 1, 1, 3, 5))
    p0 = np.zeros(1, np.int32)

    def call(h, n=1, planes=p0, refs=ref, n_refs=1, ref_planes=None, gh=1, gw=1, rh=1, rw=2, o=out, flags=0):
        refs = None if refs is None else np.ascontiguousarray(refs, np.float32)
        return lib.vt_volume_correlate_stack(h, n, None if planes is None else planes.ctypes.data, None if refs is None else refs.ctypes.data,
                                             n_refs, None if ref_planes is None else ref_planes.ctypes.data, gh, gw, rh, rw,
                                             None if o is None else o.ctypes.data, flags)

    for interp in ('filt_bspline', 'filt_bspline_simple'):
        for stack in (False, True):
            sv = handle(s, interp, stack=stack)
            with pytest.raises(ValueError, match='linear'):
                sv.correlate_stack(ref)
            assert call(sv._handle) == VT_EUNSUPPORTED and b'linear handle' in lib.vt_last_error()
            sv.close()
    sv = handle(s, edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == s.shape
    sv.close()

    sv = handle(s)
    hd = sv._handle
    want = sv.correlate_stack(ref, (1, 2), planes=[0]).copy()
    assert want.any()

    def good():
        out[...] = 0
        _native.check(call(hd), 'correlate_stack')
        assert same_bits(out, want)

    i32 = lambda *v: np.array(v, np.int32)
    nan_ref, inf_ref = ref.copy(), ref.copy()
    nan_ref[3, 3], inf_ref[18, 36] = np.nan, -np.inf
    refusals = [
        (dict(n=0), VT_EINVAL), (dict(n=-2), VT_EINVAL), (dict(o=None), VT_EINVAL),
        (dict(n_refs=2), VT_EINVAL), (dict(n_refs=-1), VT_EINVAL), (dict(n_refs=0), VT_EINVAL),
        (dict(refs=None), VT_EINVAL), (dict(ref_planes=i32(0)), VT_EINVAL),                 # neither, both
        (dict(refs=None, ref_planes=i32(T)), VT_EINVAL), (dict(refs=None, ref_planes=i32(-1)), VT_EINVAL),
        (dict(refs=None, ref_planes=i32(0), n_refs=3), VT_EINVAL),
        (dict(planes=i32(T)), VT_EINVAL), (dict(planes=i32(-1)), VT_EINVAL), (dict(planes=None), VT_EINVAL),      # n = 1 != T
        (dict(gh=0), VT_EINVAL), (dict(gw=0), VT_EINVAL), (dict(gh=H + 1), VT_EINVAL), (dict(gw=W + 1), VT_EINVAL), (dict(gh=-3), VT_EINVAL),
        (dict(rh=-1), VT_EINVAL), (dict(rw=-1), VT_EINVAL), (dict(rh=H), VT_EINVAL), (dict(rw=W), VT_EINVAL),
        (dict(refs=nan_ref), VT_EINVAL), (dict(refs=inf_ref), VT_EINVAL),
        # the bounds, decided before anything of the arrays is read: the arrays passed here hold one entry
        (dict(n=(1 << 31) - 1), VT_EUNSUPPORTED), (dict(n=1 << 28), VT_EUNSUPPORTED),       # 2^28 x 15 scores
        (dict(n=1 << 20, gh=H, gw=W, rh=1, rw=1), VT_EUNSUPPORTED),                         # 2^20 x 703 x 9
    ]
    for kw, code in refusals:
        rc = call(hd, **kw)
        assert rc == code, (kw, rc, lib.vt_last_error())
        good()
    assert lib.vt_volume_correlate_stack(None, 1, p0.ctypes.data, ref.ctypes.data, 1, None, 1, 1, 1, 2, out.ctypes.data, 0) == VT_EINVAL
    # resident references are taken as they are, n_refs is ignored with them; other flags are ignored
    out[...] = 0
    _native.check(call(hd, refs=None, ref_planes=i32(2), n_refs=1), 'resident')
    csm.check(out, *csm.model(s, None, (1, 2), (1, 1), [0], [2]), 'resident through the C interface')
    out[...] = 0
    _native.check(call(hd, flags=_native.KEEP_OUTSIDE | _native.ACCUMULATE | _native.FORCE_DIRECT), 'flags')
    assert same_bits(out, want)
    with pytest.raises(ValueError):
        sv.correlate_stack(ref, (H, 0))
    with pytest.raises(ValueError):
        sv.correlate_stack()
    good()
    sv.close()


def test_slab_and_unfinalized_handles_are_refused():
    lib = _native.load()
    vol = np.random.default_rng(9).standard_normal((20, 24, 28)).astype(np.float32)
    out = np.zeros((20, 1, 1, 3, 3))
    rp = np.roll(np.arange(20, dtype=np.int32), 1)

    def call(h):
        return lib.vt_volume_correlate_stack(h, 20, None, None, 0, rp.ctypes.data, 1, 1, 1, 1, out.ctypes.data, 0)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    _native.check(call(h), 'correlate_stack')
    lib.vt_volume_destroy(h)
    csm.check(out, *csm.model(vol, None, (1, 1), (1, 1), None, rp), 'finalized')


# ---- 6. the pipeline ----------------------------------------------------------------------------------------------------------------------
def test_find_shifts_then_align_stack_restores_a_shifted_series():
    """A white field displaced by a known integer per image: find_shifts recovers it (the integer part exactly, per patch too), and
    align_stack(shifts=-d) moves every image back onto the reference in the overlap."""
    R, n, H, W = 6, 4, 96, 80
    rng = np.random.default_rng(21)
    field = rng.standard_normal((H + 2 * R, W + 2 * R)).astype(np.float32)
    ref = np.ascontiguousarray(field[R:R + H, R:R + W])
    d = rng.integers(-R, R + 1, (n, 2))
    imgs = np.stack([field[R - dy:R - dy + H, R - dx:R - dx + W] for dy, dx in d])      # image[y + d] = reference[y]
    sv = handle(imgs, stack=True)
    try:
        found = sv.find_shifts(ref, (R, R))
        assert found.shape == (n, 1, 1, 2) and np.array_equal(np.round(found[:, 0, 0]), d) and (np.abs(found[:, 0, 0] - d) < 0.5).all()
        per_patch = sv.find_shifts(ref, (R, R), (2, 2), subpixel=False)                   # patches of 48 x 40
        assert np.array_equal(per_patch, np.broadcast_to(d[:, None, None, :], (n, 2, 2, 2)))
        assert np.array_equal(per_patch, vt.StaticVolume(imgs, device='cpu').find_shifts(ref, (R, R), (2, 2), subpixel=False))
        back = sv.align_stack(shifts=-np.round(found[:, 0, 0]))
    finally:
        sv.close()
    inner = (slice(None), slice(R, -R), slice(R, -R))
    assert np.abs(back[inner] - ref[None][inner]).max() < 1e-5
