"""-m gpu: StaticVolume.filter_stack (vt_volume_filter_stack, kernel 23): a 1-D filter along axis 1 or 2 of every image of a resident
stack.  The definition and the per-pixel bound are tests/filter_stack_model.py's; every pixel is held to the bound.  Bit identities are
compared as uint32, so the sign of a zero counts.

The stack is (5, 19, 37): one strip and one segment per image.  Segments, strips and the tap chunks are crossed by the shapes of
test_segments, test_several_strips and the two tests of the bounds.  Two refusals of the contract are out of reach of a test: n x image
bytes beyond size_t and an extent above 2^31 - 257 need handles of more than 8 GiB."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import filter_stack_model as fm

pytestmark = pytest.mark.gpu

VT_EINVAL, VT_EUNSUPPORTED = 10001, 10004
STACK = (5, 19, 37)
PLANES = np.array([0, 4, 2, 2, 3, 1, 0])
WEIGHTS = np.array([0.75, -1.5, 2.0, 0.0, 1.25, -0.5, 1.0])                  # mixed signs, one exact 0
N = len(PLANES)
PADS = ('zero', 'edge')
SAMPLE_INTERPS = ('linear', 'bspline', 'bspline_simple')                     # the interpolations whose handles hold samples
ASYM9 = np.array([0.5, -1.25, 0.0, 2.0, 0.75, 0.0, -0.375, 1.5, 0.25])       # asymmetric, interior zeros


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def data(shape=STACK, seed=53):
    s = np.random.RandomState(seed).random_sample(shape).astype(np.float32)
    s.setflags(write=False)
    return s


def tap_rows(name, axis, shared, stack=STACK):
    """The tap sets of the parity test.  Per-entry rows are the shared row scaled and, from K = 3 on, with one more tap zeroed per
    entry, so that the rows differ in their non-zero sets as well."""
    L = stack[axis]
    rng = np.random.RandomState(7)
    row = {'k1': np.array([-1.75]), 'k3': np.array([0.25, 0.5, -0.125]), 'k9': ASYM9, 'full': rng.uniform(-1, 1, 2 * L - 1),
           'ramp': vt.utils.ramp_taps(L)}[name]
    if shared:
        return row
    rows = np.stack([row * s for s in np.linspace(-1.5, 2.0, N)])
    if row.size >= 3:
        for i in range(N):
            rows[i, (3 * i) % row.size] = 0.0
    return rows


def handle(src=None, interp='linear'):
    return vt.StaticVolume(data() if src is None else src, interpolation=interp, device='gpu:0')


# ---- 1. parity with the model ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', SAMPLE_INTERPS)
@pytest.mark.parametrize('shared', [True, False], ids=['shared', 'per-entry'])
@pytest.mark.parametrize('axis', [1, 2])
def test_parity_with_the_model(axis, shared, interp):
    sv = handle(interp=interp)
    try:
        for name in ('k1', 'k3', 'k9', 'full', 'ramp'):
            taps = tap_rows(name, axis, shared)
            assert name != 'full' or taps.shape[-1] == (37, 73)[axis - 1]               # the halo exceeds the line
            for pad in PADS:
                got = sv.filter_stack(taps, axis, WEIGHTS, pad, planes=PLANES)
                assert sv.info().last_kernel == 23
                fm.check(got, *fm.model(data(), taps, axis, pad, PLANES, WEIGHTS), (interp, name, axis, pad, shared))
    finally:
        sv.close()


def test_defaults_and_stack_flag():
    """planes None (n = T), weights None; VT_STACK changes nothing for an interpolation that holds samples."""
    for stack in (False, True):
        sv = vt.StaticVolume(data(), device='gpu:0', stack=stack)
        got = sv.filter_stack(ASYM9)
        sv.close()
        fm.check(got, *fm.model(data(), ASYM9, 2, 'zero'), ('defaults', stack))


# ---- 2. segments, strips, tap chunks --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pad', PADS)
@pytest.mark.parametrize('axis', [2, 1])
def test_segments(axis, pad):
    """Three lines of 1500 samples under a full-length row of 2999 taps: 24 segments of 64 outputs, 24 tap chunks of 128, of which the
    ones wholly outside the line are not staged under pad 0."""
    src = data((2, 3, 1500), 59)
    if axis == 1:
        src = np.ascontiguousarray(src.transpose(0, 2, 1))
    taps = np.random.RandomState(3).uniform(-1, 1, 2999) / 50
    w = np.array([1.5, -0.5])
    sv = handle(src)
    try:
        got = sv.filter_stack(taps, axis, w, pad)
        info = sv.info()
        seg = info.last_tile[axis]
        assert info.last_kernel == 23 and seg > 0 and -(-1500 // seg) >= 3, tuple(info.last_tile)
    finally:
        sv.close()
    fm.check(got, *fm.model(src, taps, axis, pad, None, w), ('segments', axis, pad))


@pytest.mark.parametrize('axis', [1, 2])
def test_several_strips(axis):
    """150 lines: three strips of 64, the last one cut; 70 samples along the filtered axis: two segments, the last one cut."""
    shape = (2, 150, 70) if axis == 2 else (2, 70, 150)
    src = data(shape, 61)
    taps = np.stack([vt.utils.ramp_taps(70, 'hann', 20), vt.utils.ramp_taps(70, half_width=20)])
    sv = handle(src)
    try:
        for pad in PADS:
            got = sv.filter_stack(taps, axis, [1.0, -2.0], pad)
            info = sv.info()
            t = tuple(info.last_tile)
            assert info.last_grid == 2 * -(-shape[1] // t[1]) * -(-shape[2] // t[2]) == 2 * 3 * 2
            fm.check(got, *fm.model(src, taps, axis, pad, None, [1.0, -2.0]), ('strips', axis, pad))
    finally:
        sv.close()


# ---- 3. bounds ------------------------------------------------------------------------------------------------------------------------
def test_full_ramp_of_an_8192_pixel_axis():
    src = data((1, 2, 8192), 67)
    taps = vt.utils.ramp_taps(8192)
    assert taps.size == 16383
    sv = handle(src)
    try:
        for pad in PADS:
            got = sv.filter_stack(taps, 2, pad=pad)
            fm.check(got, *fm.model(src, taps, 2, pad), ('K = 16383', pad))
    finally:
        sv.close()


def test_no_bound_on_k_below_the_table_bound():
    """The kernel walks the taps in chunks, so k has no bound of its own (include/voltools_hip.h): K = 16385 is served; 2^26 + 1 taps in
    one call are refused before anything is read, and the handle then still answers."""
    lib = _native.load()
    src = data((1, 1, 8200), 71)
    taps = np.random.RandomState(5).uniform(-1, 1, 16385) / 100
    sv = handle(src)
    try:
        got = sv.filter_stack(taps, 2, pad='edge')
        fm.check(got, *fm.model(src, taps, 2, 'edge'), 'K = 16385')
        out = np.zeros((1, 1, 8200), np.float32)
        one = np.ones(3)
        # n = 2^14 entries of 4097 taps each (n_taps = n): 2^26 + 2^14 taps; rejected on the counts alone, the arrays are never read
        rc = lib.vt_volume_filter_stack(sv._handle, 1 << 14, one.ctypes.data, one.ctypes.data, 1 << 14, 4097, 2, 0, None, out.ctypes.data, 0)
        assert rc == VT_EUNSUPPORTED and b'taps' in lib.vt_last_error()
        k3 = np.array([1.0, -2.0, 0.5])
        fm.check(sv.filter_stack(k3), *fm.model(src, k3, 2, 'zero'), 'K = 3 after the refusal')
    finally:
        sv.close()


# ---- 4. bit identities ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('axis', [1, 2])
def test_an_image_does_not_depend_on_its_batch(axis):
    taps = tap_rows('k9', axis, False)
    perm = np.array([3, 0, 6, 2, 5, 1, 4])
    sv = handle()
    try:
        for pad in PADS:
            whole = sv.filter_stack(taps, axis, WEIGHTS, pad, planes=PLANES).copy()
            again = sv.filter_stack(taps, axis, WEIGHTS, pad, planes=PLANES)
            assert same_bits(whole, again), 'two calls'
            mixed = sv.filter_stack(taps[perm], axis, WEIGHTS[perm], pad, planes=PLANES[perm]).copy()
            assert same_bits(mixed, whole[perm]), 'a permuted batch'
            for i in range(N):
                alone = sv.filter_stack(taps[i:i + 1], axis, WEIGHTS[i:i + 1], pad, planes=PLANES[i:i + 1])
                assert same_bits(alone[0], whole[i]), ('alone', i)
                shared = sv.filter_stack(taps[i], axis, WEIGHTS[i:i + 1], pad, planes=PLANES[i:i + 1])        # the row as the shared row
                assert same_bits(shared[0], whole[i]), ('shared row', i)
            dev = vt.empty((N,) + STACK[1:], device='gpu:0')
            assert sv.filter_stack(taps, axis, WEIGHTS, pad, planes=PLANES, output=dev) is None
            assert same_bits(dev.get(), whole), 'device output'
            dev.free()
    finally:
        sv.close()


@pytest.mark.parametrize('pad', PADS)
def test_transposed_stack_along_the_other_axis_gives_the_transposed_bits(pad):
    src = data((3, 70, 150), 73)                                # both axes cross strips and segments
    taps = np.stack([ASYM9, vt.utils.ramp_taps(70, half_width=40)[:81][20:-52], ASYM9[::-1]])
    assert taps.shape == (3, 9)
    w = np.array([1.0, -0.75, 2.5])
    a = handle(src)
    b = handle(np.ascontiguousarray(src.transpose(0, 2, 1)))
    try:
        for axis in (1, 2):
            got = a.filter_stack(taps, axis, w, pad)
            other = b.filter_stack(taps, 3 - axis, w, pad)
            assert same_bits(got, np.ascontiguousarray(other.transpose(0, 2, 1))), axis
        long_taps = vt.utils.ramp_taps(70)
        assert same_bits(a.filter_stack(long_taps, 1, w, pad), np.ascontiguousarray(b.filter_stack(long_taps, 2, w, pad).transpose(0, 2, 1)))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('axis', [1, 2])
def test_zero_taps_on_both_sides_change_nothing(axis):
    L = STACK[axis]
    sv = handle()
    try:
        for pad in PADS:
            want = sv.filter_stack(ASYM9, axis, WEIGHTS, pad, planes=PLANES).copy()
            for grow in (1, 7, (2 * L - 1 - 9) // 2):
                padded = np.concatenate([np.zeros(grow), ASYM9, -np.zeros(grow)])     # zeros of both signs
                assert same_bits(sv.filter_stack(padded, axis, WEIGHTS, pad, planes=PLANES), want), (pad, grow)
    finally:
        sv.close()


def test_identity_tap_returns_the_source():
    src = np.array(data())
    src[1, 3, 4] = -0.0
    src[2, 0, 0] = np.float32(1e-42)                              # a float32 subnormal
    sv = handle(src)
    try:
        for axis in (1, 2):
            for pad in PADS:
                got = sv.filter_stack([1.0], axis, pad=pad)
                assert np.array_equal(got, src) and same_bits(np.abs(got), np.abs(src))       # up to the sign of a zero
    finally:
        sv.close()


@pytest.mark.parametrize('axis', [1, 2])
def test_pad_zero_equals_a_frame_of_zeros(axis):
    r = 4
    taps = ASYM9
    inner = data()
    framed = np.zeros((STACK[0], STACK[1] + (2 * r if axis == 1 else 0), STACK[2] + (2 * r if axis == 2 else 0)), np.float32)
    cut = (slice(None), slice(r, r + STACK[1]) if axis == 1 else slice(None), slice(r, r + STACK[2]) if axis == 2 else slice(None))
    framed[cut] = inner
    a, b = handle(inner), handle(framed)
    try:
        got = a.filter_stack(taps, axis, WEIGHTS, 'zero', planes=PLANES)
        big = b.filter_stack(taps, axis, WEIGHTS, 'zero', planes=PLANES)
        assert same_bits(got, np.ascontiguousarray(big[cut]))
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize('axis', [1, 2])
def test_a_nan_spreads_through_the_non_zero_taps_only(axis):
    taps = vt.utils.ramp_taps(STACK[axis], half_width=4)          # K = 9: non-zero at offsets 0, +-1, +-3
    assert taps.size == 9 and np.array_equal(taps != 0, [0, 1, 0, 1, 1, 1, 0, 1, 0])
    p, line, x0 = 2, 6, 11
    at = (p, line, x0) if axis == 2 else (p, x0, line)
    src = np.array(data())
    clean = src.copy()
    clean[at] = 0.625
    src[at] = np.nan
    a, b = handle(src), handle(clean)
    try:
        for pad in PADS:
            got = a.filter_stack(taps, axis, pad=pad)
            ref = b.filter_stack(taps, axis, pad=pad)
            bad = np.isnan(got)
            want = np.zeros(STACK, bool)
            for off in (-3, -1, 0, 1, 3):
                want[(p, line, x0 + off) if axis == 2 else (p, x0 + off, line)] = True
            assert np.array_equal(bad, want), (pad, np.argwhere(bad != want))
            for off in (-4, -2, 2, 4):                                                    # finite, and the bits of the clean source
                q = (p, line, x0 + off) if axis == 2 else (p, x0 + off, line)
                assert np.isfinite(got[q]) and bits(got)[q] == bits(ref)[q], (pad, off)
            assert same_bits(got[~want], ref[~want])
    finally:
        a.close()
        b.close()


# ---- 5. info() ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,axis', [(STACK, 1), (STACK, 2), ((2, 130, 70), 1), ((2, 130, 70), 2)])
def test_info(shape, axis):
    sv = handle(data(shape, 79))
    try:
        sv.filter_stack(ASYM9, axis)
        info = sv.info()
        t = tuple(info.last_tile)
        assert info.last_kernel == 23 and t[0] == 1 and t[1] > 0 and t[2] > 0
        assert info.last_grid == shape[0] * -(-shape[1] // t[1]) * -(-shape[2] // t[2])
        d = tuple(info.last_lds_dims)
        assert 0 < info.last_lds_bytes == 4 * d[0] * d[1] * d[2] <= 160 * 1024
        assert (info.out_depth, info.out_height, info.out_width) == shape                # the output shape is not touched
    finally:
        sv.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    out = np.zeros((1,) + STACK[1:], np.float32)
    p0 = np.zeros(1, np.int32)
    k3 = np.array([0.25, 0.5, -0.125])

    def call(h, n=1, planes=p0, taps=k3, n_taps=1, k=None, axis=2, pad=0, w=None, flags=0, o=out):
        taps = None if taps is None else np.ascontiguousarray(taps, np.float64)
        k = (taps.shape[-1] if taps is not None else 3) if k is None else k
        return lib.vt_volume_filter_stack(h, n, None if planes is None else planes.ctypes.data, None if taps is None else taps.ctypes.data,
                                          n_taps, k, axis, pad, None if w is None else w.ctypes.data, None if o is None else o.ctypes.data,
                                          flags)

    # handles that hold coefficients, in Python and by the library, VT_STACK or not; VT_EDGE_SCIPY
    for interp in ('filt_bspline', 'filt_bspline_simple'):
        for stack in (False, True):
            sv = vt.StaticVolume(data(), interpolation=interp, device='gpu:0', stack=stack)
            with pytest.raises(ValueError, match='linear'):
                sv.filter_stack(k3)
            assert call(sv._handle) == VT_EUNSUPPORTED and b'linear handle' in lib.vt_last_error()
            sv.close()
    sv = vt.StaticVolume(data(), device='gpu:0', edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()

    sv = handle()
    hd = sv._handle
    want = sv.filter_stack(k3, planes=[0]).copy()
    assert want.any()

    def good():
        out[...] = 0
        _native.check(call(hd), 'filter_stack')
        assert same_bits(out, want)

    refusals = [
        (dict(n=0), VT_EINVAL), (dict(n=-2), VT_EINVAL),
        (dict(taps=None), VT_EINVAL), (dict(o=None), VT_EINVAL),
        (dict(taps=np.ones(4)), VT_EINVAL), (dict(k=0), VT_EINVAL), (dict(k=-1), VT_EINVAL),
        (dict(taps=np.ones(2 * STACK[2] + 1)), VT_EINVAL), (dict(taps=np.ones(2 * STACK[1] + 1), axis=1), VT_EINVAL),
        (dict(n_taps=0), VT_EINVAL), (dict(n_taps=2), VT_EINVAL),
        (dict(axis=0), VT_EINVAL), (dict(axis=3), VT_EINVAL), (dict(pad=2), VT_EINVAL), (dict(pad=-1), VT_EINVAL),
        (dict(taps=[1.0, np.nan, 1.0]), VT_EINVAL), (dict(taps=[1.0, -np.inf, 1.0]), VT_EINVAL),
        (dict(w=np.array([np.inf])), VT_EINVAL), (dict(w=np.array([np.nan])), VT_EINVAL),
        (dict(planes=np.array([STACK[0]], np.int32)), VT_EINVAL), (dict(planes=np.array([-1], np.int32)), VT_EINVAL),
        (dict(planes=None), VT_EINVAL),                                                     # n = 1 != T
    ]
    for kw, code in refusals:
        rc = call(hd, **kw)
        assert rc == code, (kw, rc, lib.vt_last_error())
        good()
    assert lib.vt_volume_filter_stack(None, 1, p0.ctypes.data, k3.ctypes.data, 1, 3, 2, 0, None, out.ctypes.data, 0) == VT_EINVAL
    # the bounds, decided before anything of the arrays is read: the arrays passed here hold one entry
    big = handle(data((1, 70, 70), 83))
    assert call(big._handle, n=1 << 29) == VT_EUNSUPPORTED and b'grid' in lib.vt_last_error()       # 2^29 images x 4 workgroups
    assert call(big._handle, n=(1 << 31) - 1) == VT_EUNSUPPORTED
    fm.check(big.filter_stack(k3), *fm.model(data((1, 70, 70), 83), k3, 2, 'zero'), 'after the grid refusal')
    big.close()
    # Python raises for what it can see, the library for the rest
    with pytest.raises(ValueError):
        sv.filter_stack(np.ones(4))
    with pytest.raises(ValueError):
        sv.filter_stack(k3, planes=[STACK[0]])
    # flags other than VT_OUT_DEVICE are ignored
    out[...] = 0
    _native.check(call(hd, flags=_native.KEEP_OUTSIDE | _native.ACCUMULATE | _native.FORCE_DIRECT), 'filter_stack')
    assert same_bits(out, want)
    sv.close()


def test_slab_and_unfinalized_handles_are_refused():
    lib = _native.load()
    vol = data((20, 24, 28), 89)
    k3 = np.array([0.25, 0.5, -0.125])
    out = np.zeros((20, 24, 28), np.float32)

    def call(h):
        return lib.vt_volume_filter_stack(h, 20, None, k3.ctypes.data, 1, 3, 2, 0, None, out.ctypes.data, 0)

    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, vol.ctypes.data, 0, 4, 40, 4, 20, ctypes.byref(h)), 'create_slab')
    assert call(h) == VT_EINVAL and b'slab' in lib.vt_last_error()
    lib.vt_volume_destroy(h)
    h = ctypes.c_void_p()
    _native.check(lib.vt_volume_create_slab(0, 20, 24, 28, 0, None, _native.SRC_DEFERRED, 0, 20, 0, 20, ctypes.byref(h)), 'create deferred')
    assert call(h) == VT_EINVAL and b'finalize' in lib.vt_last_error()
    _native.check(lib.vt_volume_upload_planes(h, 0, 20, vol.ctypes.data, 0), 'upload')
    _native.check(lib.vt_volume_finalize(h), 'finalize')
    _native.check(call(h), 'filter_stack')
    lib.vt_volume_destroy(h)
    fm.check(out, *fm.model(vol, k3, 2, 'zero'), 'finalized')


def test_an_all_zero_row_writes_plus_zero():
    rows = np.zeros((N, 5))
    rows[1::2] = ASYM9[:5]
    rows[2, 3] = -0.0
    sv = handle()
    try:
        for axis in (1, 2):
            for pad in PADS:
                got = sv.filter_stack(rows, axis, WEIGHTS, pad, planes=PLANES)
                assert not bits(got[0::2]).any(), (axis, pad)                               # +0, whatever the weight's sign
                assert got[1].any()
                shared = sv.filter_stack(np.zeros(3), axis, -np.ones(STACK[0]), pad)
                assert not bits(shared).any()
    finally:
        sv.close()


# ---- 7. sequences and the pipeline ----------------------------------------------------------------------------------------------------
def test_sequence_on_one_handle_gives_the_bits_of_fresh_handles():
    """affine_stack -> filter_stack -> backproject -> filter_stack on one handle: the calls share the table buffer."""
    ms = vt.utils.stack_matrices(np.array([[1.5, -2.0]] * STACK[0]), None, None, STACK[1:])
    bp = vt.utils.backproject_matrices(np.linspace(-50.0, 50.0, STACK[0]), 1, (8, 19, 37), STACK)
    taps = tap_rows('ramp', 2, False)

    def steps(sv, which):
        if which == 0:
            return sv.affine_stack(ms)
        if which == 1:
            return sv.filter_stack(taps, 2, WEIGHTS, 'edge', planes=PLANES)
        if which == 2:
            return sv.backproject(bp, (8, 19, 37))
        return sv.filter_stack(ASYM9, 1)

    fresh = []
    for which in range(4):
        sv = handle()
        fresh.append(steps(sv, which).copy())
        sv.close()
    sv = handle()
    for which, kernel in zip(range(4), (21, 23, 18, 23)):
        got = steps(sv, which)
        assert sv.info().last_kernel == kernel and same_bits(got, fresh[which]), which
    sv.close()


@pytest.mark.parametrize('tilt_axis', [1, 2])
def test_ramp_filtered_series_reconstructs_closer_to_the_phantom(tilt_axis):
    plain, filtered = fm.pipeline_correlations(vt, 'gpu:0', tilt_axis)
    print(f'tilt_axis {tilt_axis}: correlation with the phantom {plain:.3f} unfiltered, {filtered:.3f} ramp-filtered')
    assert filtered > plain


def test_ramp_filter_is_filter_stack_along_the_other_axis():
    sv = handle()
    try:
        for tilt_axis in (1, 2):
            axis = 3 - tilt_axis
            got = sv.ramp_filter(tilt_axis, 'hamming', 7).copy()
            assert same_bits(got, sv.filter_stack(vt.utils.ramp_taps(STACK[axis], 'hamming', 7), axis, pad='edge'))
    finally:
        sv.close()
