"""-m gpu: StaticVolume.moments_stack (vt_volume_moments_stack, kernel 25): the sum and the sum of squares of the samples under every
patch of a grid at every shift, for every image of a resident stack; correlate_stack_normalized and find_shifts(normalized=True) on top
of it.  The definition, the per-value bounds (N + 2) 2^-53 sum |s| and (N + 2) 2^-53 sum s^2 and the kernel's plan are
tests/moments_stack_model.py's, the cases tests/moments_stack_cases.py's; every value is held to its bound.  Bit identities are compared
as uint64.

Out of reach of a test: the refusals for workgroups or row sums of one entry at or above 2^31 need handles of several GiB; the output
bound is reached through n alone."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import moments_stack_model as msm
import moments_stack_cases as msc

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
    c = next(c for c in msc.CASES if c['name'] == name)
    s, kw = msc.arguments(c, integers)
    return msm.model(s, c['max_shift'], c['grid'], kw['planes'])


def run(sv, c, integers=False, **more):
    s, kw = msc.arguments(c, integers)
    return sv.moments_stack(c['max_shift'], c['grid'], **kw, **more)


# ---- 1. every case against the model, on random data within the bound and on small integers exactly ---------------------------------------
@pytest.mark.parametrize('stack_name', sorted(msc.SHAPES))
def test_cases_against_the_model(stack_name):
    for integers in (False, True):
        sv = handle(msc.stack(stack_name, integers))
        try:
            for c in msc.CASES:
                if c['stack'] != stack_name:
                    continue
                got = run(sv, c, integers)
                assert sv.info().last_kernel == 25
                vals, bounds = modelled(c['name'], integers)
                if integers:
                    # values in [-8, 8], at most 97 x 150 pixels per patch: every partial sum is an integer below 2^20, whatever the order
                    assert np.array_equal(got, vals), (c['name'], int((got != vals).sum()))
                else:
                    msm.check(got, vals, bounds, c['name'])
        finally:
            sv.close()


@pytest.mark.parametrize('stack_name,shift,grid', [('small', (2, 7), (1, 1)), ('small', (3, 2), (3, 5)), ('pieces', (4, 12), (1, 2)),
                                                    ('pieces', (1, 30), (3, 5)), ('flat', (0, 5), (1, 3)), ('thin', (5, 0), (4, 1))])
def test_cross_check_against_correlate_stack(stack_name, shift, grid):
    """Independent device code on the same integer data, bit for bit: [..., 0] is kernel 24 against a reference of ones on the same
    handle, [..., 1] kernel 24 against ones on a handle that holds the squared stack."""
    s = msc.stack(stack_name, True)
    ones = np.ones(s.shape[1:], np.float32)
    sv, sq = handle(s), handle(s * s)
    try:
        got = sv.moments_stack(shift, grid)
        first = sv.correlate_stack(ones, shift, grid)
        second = sq.correlate_stack(ones, shift, grid)
    finally:
        sv.close()
        sq.close()
    assert same_bits(np.ascontiguousarray(got[..., 0]), first) and same_bits(np.ascontiguousarray(got[..., 1]), second)
    assert got[..., 0].any() and got[..., 1].any()


def test_sample_interpolations_and_stack_flag():
    c = next(c for c in msc.CASES if c['name'] == 'small-g3-5')
    want = None
    for interp in ('linear', 'bspline', 'bspline_simple'):
        for stack in (False, True):
            sv = handle(msc.stack('small'), interp, stack=stack)
            got = run(sv, c)
            sv.close()
            want = got if want is None else want
            assert same_bits(got, want), (interp, stack)
    msm.check(want, *modelled('small-g3-5'), 'interpolations')


# ---- 2. bit identities on random data -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stack_name', ['small', 'pieces'])
def test_alone_in_a_batch_and_permuted(stack_name):
    s = msc.stack(stack_name)
    T = s.shape[0]
    planes = np.array([3, 0, 4, 4, 1, 2, 0]) % T
    n = len(planes)
    sv = handle(s)
    try:
        for shift, grid in (((2, 7), (1, 1)), ((3, 2), (3, 5)), ((1, 21), (2, 1))):
            whole = sv.moments_stack(shift, grid, planes=planes)
            msm.check(whole, *msm.model(s, shift, grid, planes), ('batch', shift, grid))
            for i in range(n):                                                            # alone
                one = sv.moments_stack(shift, grid, planes=planes[i:i + 1])
                assert same_bits(one[0], whole[i]), (shift, grid, i)
            perm = np.random.default_rng(2).permutation(n)                                # permuted
            assert same_bits(sv.moments_stack(shift, grid, planes=planes[perm]), whole[perm])
            every = sv.moments_stack(shift, grid)                                         # planes=None: every image in order
            assert same_bits(every[planes], whole)
    finally:
        sv.close()


def test_host_and_device_output_repeats_and_recycled_memory():
    c = next(c for c in msc.CASES if c['name'] == 'pieces-r2-7')
    sv = handle(msc.stack('pieces'))
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
        small = next(c for c in msc.CASES if c['name'] == 'pieces-g3-5')
        first_small = run(sv, small)
        sv.filter_stack(np.array([0.25, 0.5, 0.25]))
        sv.correlate_stack(np.ones(msc.SHAPES['pieces'][1:], np.float32), (3, 3))         # several pieces: it fills the partials
        sv.extract_dot(np.eye(4)[None], np.ones((1, 8, 8), np.float32))
        assert same_bits(run(sv, c), want) and same_bits(run(sv, small), first_small)
        for _ in range(3):
            assert same_bits(run(sv, c), want)
    finally:
        sv.close()
    fresh = handle(msc.stack('pieces'))
    assert same_bits(run(fresh, c), want)
    fresh.close()


@pytest.mark.parametrize('stack_name,small,large,grid', [('small', (2, 3), (5, 11), (3, 5)), ('small', (0, 0), (18, 36), (1, 1)),
                                                          ('pieces', (1, 2), (12, 35), (1, 2)), ('pieces', (3, 0), (40, 6), (2, 1)),
                                                          ('pieces', (0, 15), (2, 45), (1, 1))])
def test_a_window_is_the_centre_of_a_larger_one(stack_name, small, large, grid):
    """The larger windows take other run lengths, runs per row, row blocks and blocks of column shifts."""
    s = msc.stack(stack_name)
    sv = handle(s)
    try:
        a = sv.moments_stack(small, grid)
        b = sv.moments_stack(large, grid)
    finally:
        sv.close()
    pa, pb = msm.plan(*s.shape[1:], small, grid), msm.plan(*s.shape[1:], large, grid)
    assert (pa['cv'], pa['runs'], pa['row_blocks'], pa['blocks_v']) != (pb['cv'], pb['runs'], pb['row_blocks'], pb['blocks_v'])
    du, dv = large[0] - small[0], large[1] - small[1]
    assert same_bits(a, np.ascontiguousarray(b[:, :, :, du:du + 2 * small[0] + 1, dv:dv + 2 * small[1] + 1]))


def test_a_patch_is_the_whole_of_its_cropped_stack():
    """Patch (a, b) of a grid against the (1, 1) grid of the stack cropped to that patch, at the shifts where both see the same
    samples: shift (0, 0) for every patch, and every shift of the window for a crop that keeps a margin of the window around the
    patch compared at the shifts that stay inside the crop -- there the crop's zeros are never reached."""
    s = msc.stack('pieces')
    H, W = s.shape[1:]
    sv = handle(s)
    try:
        for grid in ((1, 2), (2, 1), (3, 5), (1, 1)):
            whole = sv.moments_stack((0, 0), grid)
            ye, xe = vt.utils.patch_bounds(H, grid[0]), vt.utils.patch_bounds(W, grid[1])
            for a in range(grid[0]):
                for b in range(grid[1]):
                    crop = handle(np.ascontiguousarray(s[:, ye[a]:ye[a + 1], xe[b]:xe[b + 1]]))
                    one = crop.moments_stack((0, 0))
                    crop.close()
                    assert same_bits(one[:, 0, 0], whole[:, a, b]), (grid, a, b)
        # the interior patch of the 3 x 3 grid under (3, 4): rows 32..64, columns 50..100.  The crop that is 3 x 3 patches of exactly the
        # patch's size with the patch in its centre sees the same samples at every shift of the window.
        rh, rw = 3, 4
        whole = sv.moments_stack((rh, rw), (3, 3))
        ye, xe = vt.utils.patch_bounds(H, 3), vt.utils.patch_bounds(W, 3)
        ph, pw = int(ye[2] - ye[1]), int(xe[2] - xe[1])
        assert ye[1] - ph >= 0 and ye[2] + ph <= H and xe[1] - pw >= 0 and xe[2] + pw <= W and ph > rh and pw > rw
        crop = handle(np.ascontiguousarray(s[:, ye[1] - ph:ye[2] + ph, xe[1] - pw:xe[2] + pw]))
        one = crop.moments_stack((rh, rw), (3, 3))
        crop.close()
        assert same_bits(one[:, 1, 1], whole[:, 1, 1])
    finally:
        sv.close()


def test_split_launches_give_the_same_bits(monkeypatch):
    """The cap on one launch's row sums is 64 MiB; VT_DOT_PART_CAP (read when the handle is created) lowers it so that the 5 entries of
    this call go two per launch, and to less than a single entry needs (one entry per launch at least)."""
    s = msc.stack('pieces')
    planes = [0, 1, 1, 0, 1]
    shift, grid = (3, 3), (1, 1)
    p = msm.plan(*s.shape[1:], shift, grid)
    assert p['unit_part_bytes'] == 97 * 7 * 2 * 8
    sv = handle(s)
    want = sv.moments_stack(shift, grid, planes=planes)
    assert sv.info().last_grid == 5 * p['unit_wgs']
    sv.close()
    msm.check(want, *msm.model(s, shift, grid, planes), 'unsplit')
    for cap, per, last in ((2 * p['unit_part_bytes'], 2, 1), (p['unit_part_bytes'] - 8, 1, 1), (3 * p['unit_part_bytes'] + 8, 3, 2)):
        assert msm.launches(*s.shape[1:], shift, grid, 5, cap=cap) == (per, last)
        monkeypatch.setenv('VT_DOT_PART_CAP', str(cap))
        sv = handle(s)
        monkeypatch.delenv('VT_DOT_PART_CAP')
        got = sv.moments_stack(shift, grid, planes=planes)
        assert sv.info().last_grid == last * p['unit_wgs']
        sv.close()
        assert same_bits(got, want), cap


# ---- 3. non-finite data ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('value', [np.nan, np.inf, -np.inf])
@pytest.mark.parametrize('stack_name,shift,grid', [('small', (2, 7), (3, 5)), ('pieces', (3, 12), (2, 2))])
def test_non_finite_pixels(stack_name, shift, grid, value):
    """A non-finite image pixel makes exactly the (patch, shift) pairs whose window covers it non-finite; every other value keeps the
    bits it has without the pixel."""
    clean = msc.stack(stack_name)
    T, H, W = clean.shape
    s = clean.copy()
    y, x = H // 3, W - 2                                                                 # near the edge: some windows miss it
    s[1, y, x] = value
    a, b = handle(clean), handle(s)
    try:
        want, got = a.moments_stack(shift, grid), b.moments_stack(shift, grid)
    finally:
        a.close()
        b.close()
    hit = np.zeros(got.shape[:-1], bool)
    hit[1] = msm.covered(H, W, shift, grid, y, x)
    assert 0 < hit[1].sum() < hit[1].size
    for k in (0, 1):
        assert np.array_equal(~np.isfinite(got[..., k]), hit), k
        assert same_bits(np.ascontiguousarray(got[..., k][~hit]), np.ascontiguousarray(want[..., k][~hit]))
    msm.check(got, *msm.model(s, shift, grid), ('image', value))
    if np.isinf(value):
        assert (got[..., 0][hit] == value).all() and (got[..., 1][hit] == np.inf).all()


# ---- 4. info() against plan() -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['small-r0-0', 'small-r2-7', 'small-r18-36', 'small-g3-5', 'small-g19-37', 'pieces-r2-7', 'pieces-permuted',
                                  'pieces-g3-5', 'pieces-r40-45', 'flat-r0-22', 'thin-r22-0', 'pieces-edge-21', 'pieces-edge-22',
                                  'pieces-edge-38', 'pieces-edge-39'])
def test_info_against_the_plan(name):
    c = next(c for c in msc.CASES if c['name'] == name)
    s, kw = msc.arguments(c)
    n = s.shape[0] if kw['planes'] is None else len(kw['planes'])
    sv = handle(s)
    try:
        before = sv.info()
        run(sv, c)
        info = sv.info()
    finally:
        sv.close()
    p = msm.plan(*s.shape[1:], c['max_shift'], c['grid'], n)
    assert info.last_kernel == 25 and tuple(info.last_tile) == p['tile'] and tuple(info.last_lds_dims) == p['lds_dims']
    assert info.last_lds_bytes == p['lds_bytes'] <= msm.max_lds_bytes() and info.last_grid == p['grid']
    assert (info.out_depth, info.out_height, info.out_width) == (before.out_depth, before.out_height, before.out_width)


# ---- 5. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    s = msc.stack('small')
    T, H, W = s.shape
    out = np.zeros((1, 1, 1, 3, 5, 2))
    p0 = np.zeros(1, np.int32)

    def call(h, n=1, planes=p0, gh=1, gw=1, rh=1, rw=2, o=out, flags=0):
        return lib.vt_volume_moments_stack(h, n, None if planes is None else planes.ctypes.data, gh, gw, rh, rw,
                                           None if o is None else o.ctypes.data, flags)

    for interp in ('filt_bspline', 'filt_bspline_simple'):
        for stack in (False, True):
            sv = handle(s, interp, stack=stack)
            with pytest.raises(ValueError, match='linear'):
                sv.moments_stack()
            assert call(sv._handle) == VT_EUNSUPPORTED and b'linear handle' in lib.vt_last_error()
            sv.close()
    sv = handle(s, edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == s.shape
    sv.close()

    sv = handle(s)
    hd = sv._handle
    want = sv.moments_stack((1, 2), planes=[0]).copy()
    assert want.any()

    def good():
        out[...] = 0
        _native.check(call(hd), 'moments_stack')
        assert same_bits(out, want)

    i32 = lambda *v: np.array(v, np.int32)
    refusals = [
        (dict(n=0), VT_EINVAL), (dict(n=-2), VT_EINVAL), (dict(o=None), VT_EINVAL),
        (dict(planes=i32(T)), VT_EINVAL), (dict(planes=i32(-1)), VT_EINVAL), (dict(planes=None), VT_EINVAL),      # n = 1 != T
        (dict(gh=0), VT_EINVAL), (dict(gw=0), VT_EINVAL), (dict(gh=H + 1), VT_EINVAL), (dict(gw=W + 1), VT_EINVAL), (dict(gh=-3), VT_EINVAL),
        (dict(rh=-1), VT_EINVAL), (dict(rw=-1), VT_EINVAL), (dict(rh=H), VT_EINVAL), (dict(rw=W), VT_EINVAL),
        # the bounds, decided before anything of the arrays is read: the arrays passed here hold one entry
        (dict(n=(1 << 31) - 1), VT_EUNSUPPORTED),
        (dict(n=1 << 27), VT_EUNSUPPORTED),                                 # 2^27 x 15 shifts x 2: beyond 2^31 by the factor 2 alone
        (dict(n=1 << 20, gh=H, gw=W, rh=1, rw=1), VT_EUNSUPPORTED),                         # 2^20 x 703 x 18
    ]
    for kw, code in refusals:
        rc = call(hd, **kw)
        assert rc == code, (kw, rc, lib.vt_last_error())
        good()
    assert lib.vt_volume_moments_stack(None, 1, p0.ctypes.data, 1, 1, 1, 2, out.ctypes.data, 0) == VT_EINVAL
    out[...] = 0                                                                            # other flags are ignored
    _native.check(call(hd, flags=_native.KEEP_OUTSIDE | _native.ACCUMULATE | _native.FORCE_DIRECT), 'flags')
    assert same_bits(out, want)
    with pytest.raises(ValueError):
        sv.moments_stack((H, 0))
    good()
    sv.close()


def test_slab_and_unfinalized_handles_are_refused():
    lib = _native.load()
    vol = np.random.default_rng(9).standard_normal((20, 24, 28)).astype(np.float32)
    out = np.zeros((20, 1, 1, 3, 3, 2))

    def call(h):
        return lib.vt_volume_moments_stack(h, 20, None, 1, 1, 1, 1, out.ctypes.data, 0)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    _native.check(call(h), 'moments_stack')
    lib.vt_volume_destroy(h)
    msm.check(out, *msm.model(vol, (1, 1), (1, 1)), 'finalized')


# ---- 6. the coefficient and the pipeline ----------------------------------------------------------------------------------------------
def test_correlate_stack_normalized_is_normalized_scores_of_the_device_results():
    s = msc.stack('pieces')
    T, H, W = s.shape
    refs = np.random.default_rng(4).standard_normal((T, H, W)).astype(np.float32)
    both = np.concatenate([s, refs])
    sv = handle(both)
    try:
        for shift, grid in (((2, 3), (1, 1)), ((3, 12), (3, 5))):
            planes, rp = np.arange(T), T + np.arange(T)
            scores = sv.correlate_stack(refs, shift, grid, planes=planes)
            moments = sv.moments_stack(shift, grid, planes=planes)
            want = vt.utils.normalized_scores(scores, moments, vt.utils.patch_moments(refs, grid), image_shape=(H, W))
            got = sv.correlate_stack_normalized(refs, shift, grid, planes=planes)
            assert same_bits(got, want) and np.abs(got).max() <= 1 and got.any()
            # resident references: their moments come from the device, nothing is downloaded
            rm = sv.moments_stack((0, 0), grid, planes=rp)[:, :, :, 0, 0, :]
            want = vt.utils.normalized_scores(sv.correlate_stack(max_shift=shift, patch_grid=grid, planes=planes, reference_planes=rp),
                                              moments, rm, image_shape=(H, W))
            res = sv.correlate_stack_normalized(max_shift=shift, patch_grid=grid, planes=planes, reference_planes=rp)
            assert same_bits(res, want)
            assert np.abs(res - got).max() < 1e-12                                        # the two routes differ in the last bits at most
            out = np.empty(got.shape)
            assert sv.correlate_stack_normalized(refs, shift, grid, output=out, planes=planes) is out and same_bits(out, got)
    finally:
        sv.close()


def test_normalized_find_shifts_recovers_what_raw_scores_miss():
    """tests/test_moments_stack_host.py's 18 trials on the device."""
    msc.check_recovery(msc.recovery('gpu:0'))
