"""StaticVolume.backproject (vt_volume_backproject, kernel 18): the float64 model of tests/backproject_model.py on every voxel, bit
identity with place on plane-row matrices (linear), plain crops, the all-outside entry, plane independence of stack=True coefficients,
determinism and output kinds, accumulation, refusals, and tilt_series -> backproject_tilts end to end."""
import ctypes
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, rand_vol, rot3
from test_gpu_place import bits, tiles_of, check_sum, check_own

import backproject_model as bm

pytestmark = pytest.mark.gpu

VT_EUNSUPPORTED = 10004
STACK = (6, 40, 52)
OUT = (48, 56, 72)
BIG = (160, 160, 176)
SMALL = (12, 12, 12)                   # linear: the (8, 16, 16) tile, as BIG; OUT takes (8, 8, 16); cubic outputs always take (8, 8, 16)
PLANES = np.array([0, 5, 2, 2, 3, 1, 4, 0, 5, 3])
WEIGHTS = np.array([0.75, -1.5, 2.0, 0.0, 1.25, -0.5, 1.0, 0.6, 1.5, -2.0])       # mixed signs, one exact 0
SCALED, OUTSIDE, HUGE, IDENT = 6, 7, 8, 9
IDENT_AT = (5, 10)                     # the identity entry: image pixel (0, 0) sits at output (h, w) = IDENT_AT


def in_plane(rows, out, at=None):
    """4x4 float64 matrix whose rows 1 and 2 have the linear parts `rows` (2 x 3) and send the centre of `out` to the image point `at`
    (default: the image centre).  Row 0 is junk on purpose: it is ignored."""
    c = (np.asarray(out, np.float64) - 1) / 2
    at = (np.asarray(STACK[1:], np.float64) - 1) / 2 if at is None else np.asarray(at, np.float64)
    m = np.eye(4)
    m[0] = (0.3, -0.7, 0.2, 11.0)
    m[1:3, :3] = rows
    m[1:3, 3] = at - np.asarray(rows, np.float64) @ c
    return m


def bp_batch(out=OUT):
    """Ten float32 matrices: tilts about axis 1 at -60, -30.5, 0 and 45 degrees, a tilt about axis 2, a general 3-D rotation, in-plane
    scale 2 (y) and 0.5 (x), one entry entirely outside the image, an in-plane scale of about 40 (its patch fits no LDS buffer), the
    identity at an integer offset."""
    ms = list(vt.utils.backproject_matrices([-60.0, -30.5, 0.0, 45.0], 1, out, STACK))
    ms.append(vt.utils.backproject_matrices([25.0], 2, out, STACK)[0])
    ms.append(in_plane(rot3((20, 35, -50))[1:3], out, (21.3, 24.6)))
    ms.append(in_plane([[0, 2.0, 0], [0, 0, 0.5]], out))
    ms.append(in_plane([[0, 1.0, 0], [0, 0, 1.0]], out, (1000.0, -700.0)))
    ms.append(in_plane([[0.25, 40.0, 0], [0, 0, 40.5]], out, (27.5, 17.0)))
    ident = np.eye(4)
    ident[1, 3], ident[2, 3] = -IDENT_AT[0], -IDENT_AT[1]
    ms.append(ident)
    return np.ascontiguousarray(np.stack(ms), dtype=np.float32)


def plane_rows(ms, planes):
    """The matrices place takes for the same sums: row 0 = (0, 0, 0, plane)."""
    p = np.array(ms)
    p[:, 0, :3] = 0
    p[:, 0, 3] = planes
    return p


@functools.lru_cache(maxsize=None)
def model_case(interp):
    """(matrices, per-entry float64 model volumes, inside masks) of bp_batch on OUT: computed once per interpolation, never modified."""
    ms = bp_batch()
    vols, masks = bm.per_entry(rand_vol(STACK, 41), ms, PLANES, OUT, interp)
    for a in (ms, vols, masks):
        a.setflags(write=False)
    return ms, vols, masks


def handle(interp, seed=41, data=None):
    return vt.StaticVolume(rand_vol(STACK, seed) if data is None else data, interpolation=interp, device='gpu:0',
                           stack=interp.startswith('filt_'))


def tile_classes(mask, tile):
    """Per output tile of one entry: 0 no voxel inside, 2 every voxel inside, 1 cut."""
    nt = [-(-s // t) for s, t in zip(mask.shape, tile)]
    cls = np.zeros(nt, int)
    for a in range(nt[0]):
        for b in range(nt[1]):
            for c in range(nt[2]):
                blk = mask[a * tile[0]:(a + 1) * tile[0], b * tile[1]:(b + 1) * tile[1], c * tile[2]:(c + 1) * tile[2]]
                cls[a, b, c] = 2 if blk.all() else (1 if blk.any() else 0)
    return cls


# ---- 1. parity against the model on every voxel ----------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_parity_against_the_model(interp):
    ms, vols, masks = model_case(interp)
    assert len(ms) == 10 and not masks[OUTSIDE].any() and all(masks[i].any() for i in range(10) if i != OUTSIDE)
    assert 0 < masks[HUGE].sum() < 200                                     # the strongly minified entry reaches a few voxels
    sv = handle(interp)
    for flags in (0, _native.FORCE_DIRECT):
        got = sv.backproject(ms, OUT, WEIGHTS, planes=PLANES, _flags=flags)
        info = sv.info()
        tile = tuple(info.last_tile)
        assert info.last_kernel == 18 and tile == (8, 8, 16), (interp, flags, info.last_kernel, tile)
        assert info.last_grid == tiles_of(info, OUT) and info.last_lds_bytes <= 160 * 1024
        dims = tuple(info.last_lds_dims)
        if flags == 0:
            assert dims[0] == 2 and dims[1] > 0 and dims[2] % 4 == 0 and info.last_lds_bytes >= 2 * 4 * dims[1] * dims[2], dims
        else:
            assert dims == (2, 0, 0)
        check_sum(got, vols, WEIGHTS, TOL[interp], (interp, flags))
    # the image covers only part of this output: cut tiles occur, and for some entry whole tiles lie outside while others are reached
    classes = [tile_classes(masks[i], tile) for i in range(10)]
    assert any((c == 1).any() for c in classes) and any((c == 2).any() for c in classes)
    assert any((c == 0).any() and (c != 0).any() for i, c in enumerate(classes) if i != OUTSIDE)
    # a batch of one equals the model
    for i in (1, 5, IDENT):
        got = sv.backproject(ms[i:i + 1], OUT, [WEIGHTS[i]], planes=PLANES[i:i + 1])
        check_sum(got, vols[i:i + 1], WEIGHTS[i:i + 1], TOL[interp], (interp, 'single', i))
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline_simple'])
def test_other_tiles_and_float64_matrices(interp):
    """SMALL takes the linear (8, 16, 16) tile (one tile, cut by the end of the output in every direction); float64 matrices."""
    ms = bp_batch(SMALL).astype(np.float64)
    ms[:, 1:3, 3] += np.array([1e-9, -3e-10])                              # not representable in float32
    vols, masks = bm.per_entry(rand_vol(STACK, 41), ms, PLANES, SMALL, interp)
    assert masks.any()
    sv = handle(interp)
    for flags in (0, _native.FORCE_DIRECT):
        got = sv.backproject(ms, SMALL, WEIGHTS, planes=PLANES, _flags=flags)
        info = sv.info()
        assert info.last_kernel == 18 and tuple(info.last_tile) == ((8, 16, 16) if interp == 'linear' else (8, 8, 16))
        assert info.last_grid == tiles_of(info, SMALL)
        check_sum(got, vols, WEIGHTS, TOL[interp], (interp, SMALL, flags))
    sv.close()


# ---- 2. linear: bit for bit what place writes for the plane-row matrices -----------------------------------------------------
@pytest.mark.parametrize('out', [OUT, BIG])
def test_linear_equals_place_on_plane_rows(out):
    sv = handle('linear')
    base = np.random.RandomState(6).standard_normal(out).astype(np.float32)
    base[1, 2, 3], base[out[0] - 1, out[1] - 1, out[2] - 1], base[7, 30, 40] = -0.0, -0.0, -0.0
    for dtype in (np.float32, np.float64):
        ms = bp_batch(out).astype(dtype)
        if dtype == np.float64:
            ms[:, 1:3, 3] += np.array([1e-9, -3e-10])
        pm = plane_rows(ms, PLANES)
        for flags in (0, _native.FORCE_DIRECT):
            want = sv.place(pm, out, WEIGHTS, _flags=flags)
            assert sv.info().last_kernel == 17
            got = sv.backproject(ms, out, WEIGHTS, planes=PLANES, _flags=flags)
            info = sv.info()
            assert info.last_kernel == 18 and tuple(info.last_tile) == ((8, 8, 16) if out == OUT else (8, 16, 16))
            assert got.any() and np.array_equal(bits(got), bits(want)), (out, dtype, flags)
            a, b = base.copy(), base.copy()
            sv.place(pm, out, WEIGHTS, output=a, accumulate=True, _flags=flags)
            sv.backproject(ms, out, WEIGHTS, output=b, planes=PLANES, accumulate=True, _flags=flags)
            assert np.array_equal(bits(a), bits(b)) and not np.array_equal(bits(b), bits(base)), (out, dtype, flags, 'accumulate')
    sv.close()


# ---- 3. / 4. known answers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', [0, _native.FORCE_DIRECT])
def test_identity_entry_reproduces_the_image_in_every_plane(flags):
    stack = rand_vol(STACK, 41)
    ms = bp_batch()
    sv = handle('linear')
    p = int(PLANES[IDENT])
    got = sv.backproject(ms[IDENT:IDENT + 1], OUT, [1.0], planes=[p], _flags=flags)
    assert sv.info().last_kernel == 18
    a, b = IDENT_AT
    want = np.zeros(OUT, np.float32)
    want[:, a:a + STACK[1], b:b + STACK[2]] = stack[p]                      # the image fits the output plane: 5 + 40 <= 56, 10 + 52 <= 72
    assert np.array_equal(bits(got), bits(want)), flags
    # the other way round: an output smaller than the image shows the crop stack[p][a:a + oH, b:b + oW]
    m = np.eye(4, dtype=np.float32)
    m[1, 3], m[2, 3] = 7, 12
    got = sv.backproject(m[None], (9, 20, 30), [1.0], planes=[p], _flags=flags)
    assert np.array_equal(bits(got), bits(np.broadcast_to(stack[p][7:27, 12:42], (9, 20, 30))))
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_all_outside_entry_adds_nothing(interp):
    ms = bp_batch()
    w_other = WEIGHTS.copy()
    w_other[OUTSIDE] = 1000.0
    sv = handle(interp)
    for flags in (0, _native.FORCE_DIRECT):
        a = sv.backproject(ms, OUT, WEIGHTS, planes=PLANES, _flags=flags)
        b = sv.backproject(ms, OUT, w_other, planes=PLANES, _flags=flags)
        assert a.any() and np.array_equal(bits(a), bits(b)), (interp, flags)
    only = sv.backproject(ms[OUTSIDE:OUTSIDE + 1], OUT, [3.0], planes=[0])
    assert not bits(only).any()                                             # all +0
    sv.close()


# ---- 5. stack=True coefficients do not mix the images ---------------------------------------------------------------------------
def test_plane_independence_of_stack_coefficients():
    """Fails if an axis-0 prefilter pass ran: image 2 would leak into its neighbours' coefficients."""
    a = rand_vol(STACK, 41)
    b = a.copy()
    b[2] = rand_vol(STACK[1:], 77)
    ms = bp_batch()
    keep = PLANES != 2
    assert keep.sum() == 8
    outs = []
    for data in (a, b):
        sv = handle('filt_bspline', data=data)
        outs.append(sv.backproject(ms[keep], OUT, WEIGHTS[keep], planes=PLANES[keep]))
        full = sv.backproject(ms, OUT, WEIGHTS, planes=PLANES)
        sv.close()
        outs.append(full)
    assert outs[0].any() and np.array_equal(bits(outs[0]), bits(outs[2]))
    assert not np.array_equal(bits(outs[1]), bits(outs[3]))                 # the entries that read image 2 do differ


# ---- 6. determinism and output kinds -----------------------------------------------------------------------------------------
def test_determinism_and_output_kinds():
    ms, w = bp_batch(), WEIGHTS
    sv = handle('filt_bspline')
    fresh = sv.backproject(ms, OUT, w, planes=PLANES).copy()
    assert fresh.shape == OUT and fresh.dtype == np.float32 and fresh.any()
    assert np.array_equal(bits(fresh), bits(sv.backproject(ms, OUT, w, planes=PLANES)))
    sv.backproject(ms[:3], (9, 10, 11), planes=PLANES[:3])
    assert np.array_equal(bits(fresh), bits(sv.backproject(ms, OUT, w, planes=PLANES)))
    dims = (sv.info().out_depth, sv.info().out_height, sv.info().out_width)
    assert dims == STACK                                                 # the handle's own output shape is untouched
    other = handle('filt_bspline')
    assert np.array_equal(bits(fresh), bits(other.backproject(ms, OUT, w, planes=PLANES)))
    other.close()
    host = np.full(OUT, 5, np.float32)
    assert sv.backproject(ms, OUT, w, output=host, planes=PLANES) is None
    dev = vt.empty(OUT, device='gpu:0')
    dev.set(np.full(OUT, 5, np.float32))
    assert sv.backproject(ms, OUT, w, output=dev, planes=PLANES) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(host)) and np.array_equal(bits(fresh), bits(dev.get()))
    assert np.array_equal(bits(fresh), bits(sv.backproject(ms.astype(np.float64), OUT, w, planes=PLANES)))      # the float64 entry point
    torch = pytest.importorskip('torch')
    tens = torch.full(OUT, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.backproject(ms, OUT, w, output=tens, planes=PLANES) is None
    sv.synchronize()
    assert np.array_equal(bits(fresh), bits(tens.cpu().numpy()))
    # planes=None: image i belongs to matrix i
    six = sv.backproject(ms[:6], OUT, w[:6])
    assert np.array_equal(bits(six), bits(sv.backproject(ms[:6], OUT, w[:6], planes=np.arange(6))))
    sv.close()


# ---- 7. accumulate ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_accumulate(interp):
    ms, _, masks = model_case(interp)
    sub = [IDENT, SCALED]
    w = np.array([1.5, -0.75])
    reached = masks[IDENT] | masks[SCALED]
    assert reached.any() and not reached[:, 48:, :].any()               # whole tiles of (8, 8, 16) stay unreached: the rows h >= 48
    base = np.random.RandomState(9).standard_normal(OUT).astype(np.float32)
    base[3, 50, 66], base[10, 52, 68], base[40, 49, 70], base[5, 20, 30] = np.nan, -0.0, np.inf, -0.0
    assert not reached[3, 50, 66] and not reached[10, 52, 68] and not reached[40, 49, 70] and reached[5, 20, 30]
    sv = handle(interp)
    host = None
    for flags in (0, _native.FORCE_DIRECT):
        # the library's own per-entry results on the same route (a batch of one with weight 1 returns B_i itself)
        ref, mag = base.astype(np.float64), np.abs(base).astype(np.float64)
        for k, i in enumerate(sub):
            own = sv.backproject(ms[i:i + 1], OUT, [1.0], planes=PLANES[i:i + 1], _flags=flags).astype(np.float64)
            assert np.array_equal(own != 0, masks[i] & (own != 0))
            ref += w[k] * own
            mag += abs(w[k]) * np.abs(own)
        got = base.copy()
        assert sv.backproject(ms[sub], OUT, w, output=got, planes=PLANES[sub], accumulate=True, _flags=flags) is None
        info = sv.info()
        assert info.last_kernel == 18 and info.last_grid == tiles_of(info, OUT)
        # no entry reaches: every bit as found (NaN, Inf and -0 included); elsewhere double(base) + the sum, rounded once
        assert np.array_equal(bits(got)[~reached], bits(base)[~reached])
        assert np.isnan(got[3, 50, 66]) and bits(got)[10, 52, 68] == 0x80000000
        check_own(got[reached], ref[reached], mag[reached], (interp, 'accumulate', flags))
        assert not np.array_equal(bits(got)[reached], bits(base)[reached])
        if flags == 0:
            host = got
    dev = vt.empty(OUT, device='gpu:0')
    dev.set(base)
    assert sv.backproject(ms[sub], OUT, w, output=dev, planes=PLANES[sub], accumulate=True) is None
    sv.synchronize()
    assert np.array_equal(bits(dev.get()), bits(host))
    sv.close()


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    lib = _native.load()
    ms = bp_batch()
    m1 = np.ascontiguousarray(ms[IDENT:IDENT + 1])
    one = np.ones(1)
    p0 = np.zeros(1, np.int32)
    out = np.zeros((8, 8, 16), np.float32)

    def call(sv, n=1, mat=m1, planes=p0, w=one, shape=(8, 8, 16), flags=0):
        return lib.vt_volume_backproject(sv._handle, n, mat.ctypes.data, None if planes is None else planes.ctypes.data,
                                         None if w is None else w.ctypes.data, *shape, out.ctypes.data, flags)

    # coefficients prefiltered along axis 0 as well: refused, in Python and by the library
    sv = vt.StaticVolume(rand_vol(STACK, 41), interpolation='filt_bspline', device='gpu:0')
    with pytest.raises(ValueError):
        sv.backproject(ms, OUT, planes=PLANES)
    assert call(sv) == VT_EUNSUPPORTED and b'VT_STACK' in lib.vt_last_error()
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK           # ... and the handle does everything else
    sv.close()
    # in-plane coefficients: every 3-D sampling entry point refuses them
    sv = handle('filt_bspline')
    eye = np.eye(4, dtype=np.float32)
    for what in (lambda: sv.affine(eye), lambda: sv.affine_batch(eye[None]), lambda: sv.extract(eye[None], (4, 4, 4)),
                 lambda: sv.extract_sum(eye[None], (4, 4, 4)), lambda: sv.place(eye[None], (8, 8, 8)),
                 lambda: sv.projection(eye), lambda: sv.projection_batch(eye[None])):
        with pytest.raises(RuntimeError, match='in-plane'):
            what()
    assert f'code {VT_EUNSUPPORTED}' in str(pytest.raises(RuntimeError, sv.affine, eye).value)
    # plane indices
    for bad in ([6], [-1]):
        with pytest.raises(ValueError):
            sv.backproject(m1, OUT, planes=bad)
        assert call(sv, planes=np.array(bad, np.int32)) == VT_EINVAL and b'plane' in lib.vt_last_error()
    with pytest.raises(ValueError):
        sv.backproject(ms[:5], OUT)                                        # planes=None with n != T
    assert call(sv, planes=None) == VT_EINVAL and b'plane' in lib.vt_last_error()
    # non-finite matrix or weight, n, dims
    bad = m1.copy()
    bad[0, 2, 1] = np.nan
    with pytest.raises(RuntimeError, match='finite'):
        sv.backproject(bad, OUT, planes=[0])
    assert call(sv, mat=bad) == VT_EINVAL
    with pytest.raises(ValueError):
        sv.backproject(m1, OUT, [np.inf], planes=[0])
    assert call(sv, w=np.array([np.inf])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    assert call(sv, n=0) == VT_EINVAL and call(sv, shape=(0, 8, 16)) == VT_EINVAL
    with pytest.raises(ValueError):
        sv.backproject(m1, OUT, planes=[0], accumulate=True)               # accumulate without output
    # the handle is still usable; NULL weights are ones; flags other than the four are ignored
    _native.check(call(sv, w=None, flags=_native.KEEP_OUTSIDE | _native.PLACE_DENSE), 'backproject')
    want = sv.backproject(m1, (8, 8, 16), planes=[0])
    assert want.any() and np.array_equal(bits(out), bits(want))
    sv.close()
    # create: VT_STACK with VT_EDGE_SCIPY, a slab window or deferred construction
    vol = rand_vol(STACK, 41)
    h = ctypes.c_void_p()
    assert lib.vt_volume_create(0, *STACK, 3, vol.ctypes.data, _native.STACK | _native.EDGE_SCIPY, ctypes.byref(h)) == VT_EUNSUPPORTED
    assert lib.vt_volume_create_slab(0, *STACK, 3, vol.ctypes.data, _native.STACK, 2, 12, 2, 6, ctypes.byref(h)) == VT_EUNSUPPORTED
    assert lib.vt_volume_create_slab(0, *STACK, 3, None, _native.STACK | _native.SRC_DEFERRED, 0, 6, 0, 6, ctypes.byref(h)) == VT_EUNSUPPORTED
    with pytest.raises(ValueError):
        vt.StaticVolume(vol, device='gpu:0', stack=True, edge='scipy')
    # with the other interpolations the flag changes nothing
    m = vt.utils.transform_matrix(rotation=(10, 45, -20), center=np.divide(np.subtract(STACK, 1), 2, dtype=np.float32))
    for interp in ('linear', 'bspline'):
        a = vt.StaticVolume(vol, interpolation=interp, device='gpu:0', stack=True)
        b = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
        assert np.array_equal(bits(a.affine(m)), bits(b.affine(m)))
        assert np.array_equal(bits(a.backproject(ms, OUT, planes=PLANES)), bits(b.backproject(ms, OUT, planes=PLANES)))
        a.close()
        b.close()


# ---- 9. end to end ---------------------------------------------------------------------------------------------------------------
def test_tilt_series_then_backproject_finds_the_blob():
    n = 48
    blob = (20, 30, 17)
    g = np.arange(n, dtype=np.float64)
    vol = np.exp(-((g[:, None, None] - blob[0]) ** 2 + (g[None, :, None] - blob[1]) ** 2 + (g[None, None, :] - blob[2]) ** 2) / (2 * 2.0 ** 2))
    angles = np.linspace(-60, 60, 13)
    sv = vt.StaticVolume(vol.astype(np.float32), device='gpu:0')
    series = sv.tilt_series(angles, 1)
    sv.close()
    assert series.shape == (13, n, n)
    for interp in ('linear', 'filt_bspline'):
        st = vt.StaticVolume(series, interpolation=interp, device='gpu:0', stack=True)
        rec = st.backproject_tilts(angles, 1, output_shape=(n, n, n))
        assert st.info().last_kernel == 18
        st.close()
        peak = np.unravel_index(int(np.argmax(rec)), rec.shape)
        print(interp, 'blob', blob, 'peak', peak)
        assert max(abs(int(a) - b) for a, b in zip(peak, blob)) <= 1, (interp, peak)
