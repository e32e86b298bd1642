"""-m gpu: StaticVolume.affine_stack (vt_volume_affine_stack, kernel 21): every image of a resident stack under its own 2-D affine map.
The definition is bm.per_entry(stack, M4, planes, (1, Ho, Wo), interp) of tests/backproject_model.py times the entry's weight; tolerances
are TOL of tests/test_gpu_extract.py on unit-range data times |w_i|.  Bit identities are compared as uint32, so the sign of a zero counts.

The stack is (6, 40, 52).  Output (37, 45) takes the (1, 16, 16) tile with cut tiles on both axes, (61, 59) the (1, 32, 32) tile."""
import functools

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from test_gpu_extract import TOL, ALL_INTERPS, VT_EINVAL, rand_vol
from test_gpu_box_lattice import positive

import backproject_model as bm

pytestmark = pytest.mark.gpu

VT_EUNSUPPORTED = 10004
STACK = (6, 40, 52)
OUT = (37, 45)
OUT32 = (61, 59)
TILE = {OUT: (1, 16, 16), OUT32: (1, 32, 32)}
PLANES = np.array([0, 5, 2, 2, 3, 1, 4, 0, 5, 3])
WEIGHTS = np.array([0.75, -1.5, 2.0, 0.0, 1.25, -0.5, 1.0, 0.6, 1.5, -2.0])       # mixed signs, one exact 0
NONZERO = np.where(WEIGHTS == 0, 0.5, WEIGHTS)
OUTSIDE = 7
FLAGS = (0, _native.FORCE_DIRECT)
CAP = 32 * 1024                        # bytes of LDS a staged patch may take (include/voltools_hip.h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def in_plane(lin, out, at=None, image=STACK):
    """4x4 float64 matrix whose rows 1 and 2 carry the 2 x 2 linear part `lin` in columns 1 and 2 and send the centre of the output image
    to the image point `at` (default: the image centre).  Row 0 and column 0 are junk on purpose: they are ignored."""
    lin = np.asarray(lin, np.float64)
    c = (np.asarray(out, np.float64) - 1) / 2
    at = (np.asarray(image[-2:], np.float64) - 1) / 2 if at is None else np.asarray(at, np.float64)
    m = np.eye(4)
    m[0] = (0.3, -0.7, 0.2, 11.0)
    m[1:3, 0] = (0.25, -0.5)
    m[1:3, 1:3] = lin
    m[1:3, 3] = at - lin @ c
    return m


def rot(deg):
    t = np.deg2rad(deg)
    return np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])


@functools.lru_cache(maxsize=None)
def batch(out=OUT):
    """Ten float64 matrices: the identity at an integer offset, a rotation by 30 degrees, a rotation within 1e-3 of 45 degrees, scale 0.5,
    scale 2, a shear, a sub-pixel shift, one entry wholly outside, two entries partly outside."""
    ident = in_plane(np.eye(2), out)
    ident[1, 3], ident[2, 3] = 3.0, 4.0
    sub = in_plane(np.eye(2), out)
    sub[1, 3], sub[2, 3] = 1.375, 2.8125
    ms = [ident, in_plane(rot(30.0), out), in_plane(rot(45.0005), out, (19.25, 26.5)), in_plane(0.5 * np.eye(2), out),
          in_plane(2.0 * np.eye(2), out), in_plane([[1.0, 0.35], [-0.2, 1.0]], out), sub,
          in_plane(np.eye(2), out, (1000.0, -700.0)), in_plane(np.eye(2), out, (35.5, -4.25)), in_plane(1.2 * rot(-70.0), out, (6.0, 44.0))]
    ms = np.ascontiguousarray(np.stack(ms))
    ms.setflags(write=False)
    return ms


@functools.lru_cache(maxsize=None)
def data(seed=41, shape=STACK):
    s = rand_vol(shape, seed)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def model_case(interp, out=OUT, f32=False, pos=False):
    """(per-entry float64 model images (10, Ho, Wo), inside masks) of batch(out): computed once, never modified."""
    ms = batch(out)
    ms = ms.astype(np.float32).astype(np.float64) if f32 else ms
    src = positive(data()) if pos else data()
    vols, masks = bm.per_entry(src, ms, PLANES, (1,) + out, interp)
    vols, masks = vols[:, 0], masks[:, 0]
    vols.setflags(write=False)
    masks.setflags(write=False)
    return vols, masks


def handle(interp, src=None):
    return vt.StaticVolume(data() if src is None else src, interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))


def check_entries(got, vols, w, tol, what):
    """Every pixel of every entry: |got_i - w_i B_i| <= |w_i| tol."""
    assert got.dtype == np.float32 and got.shape == vols.shape, what
    for i in range(len(vols)):
        err = float(np.abs(got[i].astype(np.float64) - w[i] * vols[i]).max())
        print(what, f'entry {i}: max|hip - model| {err:.3e}  bound {abs(w[i]) * tol:.3e}')
        assert err <= abs(w[i]) * tol, (what, i, err)


def tiles_in(out, tile):
    return -(-out[0] // tile[1]) * -(-out[1] // tile[2])


def patch_dims(m, tile, cubic):
    """The staged patch of an entry (include/voltools_hip.h; extract_box_dims' formula on rows 1 and 2)."""
    L = []
    for r in (1, 2):
        ext = abs(m[r, 1]) * (tile[1] - 1) + abs(m[r, 2]) * (tile[2] - 1)
        L.append(int(np.floor(ext + 2.0 ** -23)) + 3 + (2 if cubic else 0))
    return L[0], (L[1] + 6) & ~3


# ---- 1. parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
@pytest.mark.parametrize('out', [OUT, OUT32], ids=['16x16', '32x32'])
def test_parity_against_the_model(out, interp):
    sv = handle(interp)
    try:
        for f32 in (True, False):
            ms = batch(out).astype(np.float32) if f32 else batch(out)
            vols, masks = model_case(interp, out, f32)
            assert not masks[OUTSIDE].any() and all(masks[i].any() for i in range(10) if i != OUTSIDE)
            assert all(0 < masks[i].sum() < masks[i].size for i in (8, 9))
            for flags in FLAGS:
                got = sv.affine_stack(ms, out, WEIGHTS, planes=PLANES, _flags=flags)
                info = sv.info()
                assert info.last_kernel == 21 and tuple(info.last_tile) == TILE[out], (info.last_kernel, tuple(info.last_tile))
                assert info.last_grid == 10 * tiles_in(out, TILE[out])
                dims = tuple(info.last_lds_dims)
                if flags == 0:
                    assert dims[0] == 1 and dims[1] > 0 and dims[2] % 4 == 0 and info.last_lds_bytes == 4 * dims[1] * dims[2] <= CAP, dims
                else:
                    assert dims == (0, 0, 0) and info.last_lds_bytes == 0
                check_entries(got, vols, WEIGHTS, TOL[interp], (interp, out, f32, flags))
                assert not bits(got[OUTSIDE]).any() and not bits(got[3]).any()         # all outside, weight 0: +0 throughout
    finally:
        sv.close()


# ---- 2. the inside mask ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
@pytest.mark.parametrize('out', [OUT, OUT32], ids=['16x16', '32x32'])
def test_inside_mask_pixel_for_pixel(out, interp):
    """Data in [1, 2) and weights without a zero: inside the skirt the smallest weight on a real tap is positive, so `got != 0` is the
    model's mask."""
    _, masks = model_case(interp, out, False, True)
    sv = handle(interp, positive(data()))
    try:
        for flags in FLAGS:
            got = sv.affine_stack(batch(out), out, NONZERO, planes=PLANES, _flags=flags)
            for i in range(10):
                differs = int(((got[i] != 0) != masks[i]).sum())
                assert differs == 0, (interp, out, flags, i, differs)
                assert not bits(got[i][~masks[i]]).any()                                # outside: +0, not -0
    finally:
        sv.close()


# ---- 3. bit identities -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ALL_INTERPS)
def test_bit_identities(interp):
    sv = handle(interp)
    try:
        for out in (OUT, OUT32):
            for ms in (batch(out), batch(out).astype(np.float32)):
                tiled = sv.affine_stack(ms, out, WEIGHTS, planes=PLANES)
                direct = sv.affine_stack(ms, out, WEIGHTS, planes=PLANES, _flags=_native.FORCE_DIRECT)
                if interp == 'linear':                                                  # (a) the same taps and arithmetic on both routes
                    assert same_bits(tiled, direct), (out, ms.dtype)
                for i in range(10):
                    one = dict(weights=[WEIGHTS[i]], planes=PLANES[i:i + 1])
                    # (b) the direct route is backproject's for that entry alone at depth 1
                    want = sv.backproject(ms[i:i + 1], (1,) + out, _flags=_native.FORCE_DIRECT, **one)[0]
                    assert sv.info().last_kernel == 18
                    assert same_bits(direct[i], want), (interp, out, ms.dtype, i, int((bits(direct[i]) != bits(want)).sum()))
                    # (c) the default routes agree to rounding
                    want = sv.backproject(ms[i:i + 1], (1,) + out, **one)[0]
                    err = float(np.abs(tiled[i].astype(np.float64) - want).max())
                    assert err <= abs(WEIGHTS[i]) * TOL[interp], (interp, out, i, err)
    finally:
        sv.close()


# ---- 4. independence -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_an_image_does_not_depend_on_the_batch(interp):
    ms = batch()
    sv = handle(interp)
    try:
        for flags in FLAGS:
            full = sv.affine_stack(ms, OUT, WEIGHTS, planes=PLANES, _flags=flags).copy()
            assert full.any()
            assert same_bits(sv.affine_stack(ms, OUT, WEIGHTS, planes=PLANES, _flags=flags), full)           # repeated
            for perm in (np.arange(10)[::-1], np.array([4, 0, 6, 2, 9, 5, 1, 8, 3, 7])):
                got = sv.affine_stack(ms[perm], OUT, WEIGHTS[perm], planes=PLANES[perm], _flags=flags)
                assert same_bits(got, full[perm]), (interp, flags, perm)
            for i in range(10):
                got = sv.affine_stack(ms[i:i + 1], OUT, WEIGHTS[i:i + 1], planes=PLANES[i:i + 1], _flags=flags)
                assert sv.info().last_grid == tiles_in(OUT, TILE[OUT]) and same_bits(got[0], full[i]), (interp, flags, i)
            many = sv.affine_stack(np.tile(ms, (61, 1, 1)), OUT, np.tile(WEIGHTS, 61), planes=np.tile(PLANES, 61), _flags=flags)
            assert sv.info().last_grid == 610 * tiles_in(OUT, TILE[OUT])
            assert same_bits(many, np.tile(full, (61, 1, 1))), (interp, flags)
    finally:
        sv.close()


def test_output_kinds_and_recycled_memory():
    ms = batch()
    shape = (10,) + OUT
    for interp in ('linear', 'filt_bspline'):
        sv = handle(interp)
        fresh = sv.affine_stack(ms, OUT, WEIGHTS, planes=PLANES).copy()
        host = np.full(shape, 5, np.float32)
        assert sv.affine_stack(ms, OUT, WEIGHTS, output=host, planes=PLANES) is None and same_bits(host, fresh)
        dev = vt.empty(shape, device='gpu:0')
        dev.set(np.full(shape, 5, np.float32))
        assert sv.affine_stack(ms, OUT, WEIGHTS, output=dev, planes=PLANES) is None
        sv.synchronize()
        assert same_bits(dev.get(), fresh)
        assert (sv.info().out_depth, sv.info().out_height, sv.info().out_width) == STACK          # the handle's own output shape is untouched
        sv.close()
        # a handle whose resident buffer is the recycled allocation of one that held 1e3
        big = vt.StaticVolume(np.full(STACK, 1e3, np.float32), interpolation=interp, device='gpu:0', stack=interp.startswith('filt_'))
        big.affine_stack(ms, OUT, planes=PLANES)
        big.close()
        other = handle(interp)
        assert same_bits(other.affine_stack(ms, OUT, WEIGHTS, planes=PLANES), fresh)
        other.close()


def test_torch_output():
    torch = pytest.importorskip('torch')
    ms = batch()
    sv = handle('bspline')
    fresh = sv.affine_stack(ms, OUT, WEIGHTS, planes=PLANES).copy()
    tens = torch.full((10,) + OUT, 5.0, dtype=torch.float32, device='cuda:0')
    assert sv.affine_stack(ms, OUT, WEIGHTS, output=tens, planes=PLANES) is None
    sv.synchronize()
    assert same_bits(tens.cpu().numpy(), fresh)
    sv.close()


# ---- 5. exact cases --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags', FLAGS)
def test_identity_and_integer_shifts_are_crops(flags):
    stack = data()
    sv = handle('linear')
    shifts = [(0, 0), (3, 4), (-5, 7), (12, -20), (-39, 51), (40, 0)]
    for out in (OUT, STACK[1:], OUT32):
        ms = np.tile(np.eye(3), (6, 1, 1))
        ms[:, :2, 2] = shifts
        got = sv.affine_stack(ms, out, planes=[0, 1, 2, 3, 4, 5], _flags=flags)
        for i, (a, b) in enumerate(shifts):
            want = np.zeros(out, np.float32)
            h = np.arange(out[0])[:, None] + a
            w = np.arange(out[1])[None, :] + b
            ok = (h >= 0) & (h < STACK[1]) & (w >= 0) & (w < STACK[2])
            want[ok] = stack[i][np.clip(h, 0, STACK[1] - 1), np.clip(w, 0, STACK[2] - 1)][ok]
            assert same_bits(got[i], want), (out, flags, i)                              # pixels beyond the image: +0
    sv.close()


def test_filtered_stack_identity_and_plane_independence():
    """Under the identity a filt_bspline stack returns its images wherever the 3 x 3 stencil of non-zero weights lies inside the image.
    On the outermost rows and columns one tap row or column is beyond the image and reads 0 by definition, so the definition itself --
    the float64 model -- is up to 0.31 away from the image there (0.3057 on this data); those pixels are held to the model."""
    stack = data()
    sv = handle('filt_bspline')
    got = sv.affine_stack(np.tile(np.eye(3), (6, 1, 1)))
    err = float(np.abs(got.astype(np.float64) - stack)[:, 1:-1, 1:-1].max())
    print(f'filt_bspline identity: max|got - image| {err:.3e} on the interior')
    assert got.shape == STACK and err <= TOL['filt_bspline']
    vols, _ = bm.per_entry(stack, np.tile(np.eye(4), (6, 1, 1)), None, (1,) + STACK[1:], 'filt_bspline')
    check_entries(got, vols[:, 0], np.ones(6), TOL['filt_bspline'], 'filt_bspline identity, every pixel')
    sv.close()
    # changing image k changes the entries of plane k only: no axis-0 prefilter pass ran, no neighbouring plane was read
    k = 2
    other = np.array(stack)
    other[k] = rand_vol(STACK[1:], 9)
    ms = batch()
    for interp in ('filt_bspline', 'linear', 'bspline_simple'):
        for flags in FLAGS:
            a, b = handle(interp), handle(interp, other)
            ga = a.affine_stack(ms, OUT, NONZERO, planes=PLANES, _flags=flags)
            gb = b.affine_stack(ms, OUT, NONZERO, planes=PLANES, _flags=flags)
            for i in range(10):
                if PLANES[i] == k:
                    assert not np.array_equal(ga[i], gb[i]), (interp, flags, i)
                else:
                    assert same_bits(ga[i], gb[i]), (interp, flags, i)
            a.close()
            b.close()


# ---- 6. the staging cap, mixed routes, long rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_scale_sweep_across_the_staging_cap(interp):
    cubic = interp != 'linear'
    sv = handle(interp)
    staged = []
    try:
        for s in (4.0, 5.0, 5.3, 5.5, 5.7, 5.9, 6.5, 9.0):
            m = in_plane(s * np.eye(2), OUT)[None]
            vols, _ = bm.per_entry(data(), m, [1], (1,) + OUT, interp)
            got = sv.affine_stack(m, OUT, [1.5], planes=[1])
            info = sv.info()
            Ly, Lx = patch_dims(m[0], TILE[OUT], cubic)
            fits = 4 * Ly * Lx <= CAP
            staged.append(fits)
            assert tuple(info.last_lds_dims) == ((1, Ly, Lx) if fits else (0, 0, 0)), (s, tuple(info.last_lds_dims), Ly, Lx)
            assert info.last_lds_bytes == (4 * Ly * Lx if fits else 0)
            check_entries(got, vols[:, 0], [1.5], TOL[interp], (interp, 'scale', s))
    finally:
        sv.close()
    assert staged[0] and not staged[-1] and staged == sorted(staged, reverse=True)           # one switch, from staged to gathered


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
def test_routes_mixed_in_one_batch(interp):
    """A staged entry, an entry too large to stage, an outside entry, a staged entry of another patch size -- in this order and reversed."""
    ms = np.stack([in_plane(rot(20.0), OUT), in_plane(8.0 * rot(10.0), OUT), in_plane(np.eye(2), OUT, (-500.0, 90.0)),
                   in_plane(0.3 * np.eye(2), OUT, (11.2, 30.6)), in_plane(3.0 * np.eye(2), OUT)])
    planes = np.array([4, 1, 0, 5, 2])
    w = np.array([1.0, -0.75, 2.0, 0.5, 1.25])
    vols, masks = bm.per_entry(data(), ms, planes, (1,) + OUT, interp)
    assert masks[1].any() and not masks[2].any()
    sv = handle(interp)
    try:
        single, dims = [], []
        for i in range(5):
            single.append(sv.affine_stack(ms[i:i + 1], OUT, w[i:i + 1], planes=planes[i:i + 1])[0].copy())
            dims.append(tuple(sv.info().last_lds_dims))
        assert dims[1] == (0, 0, 0) and all(dims[i][0] == 1 for i in (0, 2, 3, 4)), dims
        sizes = [d[1] * d[2] for d in dims]
        assert sizes[4] > 2 * sizes[0] > 4 * sizes[3] > 0, sizes
        for order in (np.arange(5), np.arange(5)[::-1], np.array([1, 1, 0, 2, 1, 3, 4, 1])):
            got = sv.affine_stack(ms[order], OUT, w[order], planes=planes[order])
            assert tuple(sv.info().last_lds_dims) == dims[4] and sv.info().last_lds_bytes == 4 * sizes[4]
            check_entries(got, vols[order, 0], w[order], TOL[interp], (interp, 'mixed'))
            for k, i in enumerate(order):
                assert same_bits(got[k], single[i]), (interp, k, i)
    finally:
        sv.close()


@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_long_patch_rows(interp):
    """A (2, 8, 1200) stack under x = 70 w: the staged rows are longer than 1024 floats (more than 256 vectors: stage_patch's long-row
    regime)."""
    shape, out = (2, 8, 1200), (8, 16)
    src = data(43, shape)
    ms = np.stack([in_plane([[0.1, 0.0], [0.0, 70.0]], out, image=shape), in_plane([[0.1, 0.001], [0.5, -68.0]], out, (3.2, 600.7), image=shape)])
    vols, masks = bm.per_entry(src, ms, None, (1,) + out, interp)
    assert masks.all()
    sv = handle(interp, src)
    try:
        got = sv.affine_stack(ms, out, [1.0, -2.0])
        info = sv.info()
        assert tuple(info.last_tile) == (1, 16, 16) and info.last_lds_dims[2] > 1024 and info.last_lds_bytes <= CAP, tuple(info.last_lds_dims)
        check_entries(got, vols[:, 0], [1.0, -2.0], TOL[interp], (interp, 'long rows'))
        direct = sv.affine_stack(ms, out, [1.0, -2.0], _flags=_native.FORCE_DIRECT)
        check_entries(direct, vols[:, 0], [1.0, -2.0], TOL[interp], (interp, 'long rows, direct'))
        if interp == 'linear':
            assert same_bits(got, direct)
    finally:
        sv.close()


# ---- 7. small and odd shapes -----------------------------------------------------------------------------------------------------------
SMALL_CASES = [((2, 40, 49), (21, 33)), ((2, 40, 50), (21, 33)), ((2, 40, 51), (21, 33)), ((2, 3, 52), (7, 40)), ((2, 5, 52), (7, 40)),
               ((1, 1, 1), (5, 6)), ((1, 2, 3), (5, 6)), ((2, 40, 52), (1, 1)), ((2, 40, 52), (1, 70)), ((2, 40, 52), (70, 1))]


@pytest.mark.parametrize('interp', ['linear', 'bspline', 'filt_bspline'])
@pytest.mark.parametrize('shape,out', SMALL_CASES, ids=[f'{"x".join(map(str, s))}-{"x".join(map(str, o))}' for s, o in SMALL_CASES])
def test_small_and_odd_shapes(shape, out, interp):
    src = data(47, shape)
    ms = np.stack([in_plane(np.eye(2), out, image=shape), in_plane(0.8 * rot(25.0), out, image=shape),
                   in_plane([[0.4, 0.1], [-0.2, 0.7]], out, (shape[1] / 2 - 0.3, shape[2] / 2 + 0.2), image=shape)])
    planes = np.array([0, shape[0] - 1, 0])
    w = np.array([1.0, -1.5, 0.5])
    vols, masks = bm.per_entry(src, ms, planes, (1,) + out, interp)
    assert masks.any()
    sv = handle(interp, src)
    try:
        for flags in FLAGS:
            got = sv.affine_stack(ms, out, w, planes=planes, _flags=flags)
            assert sv.info().last_kernel == 21
            check_entries(got, vols[:, 0], w, TOL[interp], (interp, shape, out, flags))
    finally:
        sv.close()


# ---- 8. non-finite data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', ['linear', 'bspline'])
def test_non_finite_pixels_reach_their_stencils_only(interp):
    """Coordinates on the lattice (multiples of 0.1) + an offset: nowhere within 1e-3 of an integer, so every tap of a stencil has a
    non-zero weight and the model's set of non-finite outputs is exact.  The cubic gather's extra columns are dropped by selects."""
    src = np.array(data())
    src[1, 17, 23] = np.nan
    src[1, 9, 40] = np.inf
    src[4, 0, 0] = np.inf
    src[4, 39, 51] = np.nan
    ms = np.zeros((4, 4, 4))
    ms[:, 0, 0] = ms[:, 3, 3] = 1
    ms[0, 1:3, 1:] = [(0.8, 0.1, 3.33), (0.1, 0.9, 5.47)]
    ms[1, 1:3, 1:] = [(1.2, -0.3, 2.25), (0.3, 1.1, 4.55)]
    ms[2, 1:3, 1:] = [(1.0, 0.0, -1.35), (0.0, 1.0, -2.65)]
    ms[3, 1:3, 1:] = [(0.9, 0.2, 5.15), (-0.2, 1.3, 9.75)]
    planes = np.array([1, 1, 4, 4])
    w = np.array([1.0, -2.0, 0.5, 1.5])
    y = np.stack([np.stack(bm.coords(m, (1,) + OUT)) for m in ms])
    assert np.abs(y - np.round(y)).min() > 1e-3
    vols, masks = bm.per_entry(src, ms, planes, (1,) + OUT, interp)
    bad = ~np.isfinite(vols[:, 0])
    assert all(b.any() for b in bad) and not bad.all()
    sv = handle(interp, src)
    try:
        for flags in FLAGS:
            got = sv.affine_stack(ms, OUT, w, planes=planes, _flags=flags)
            assert np.array_equal(~np.isfinite(got), bad), (interp, flags, int((~np.isfinite(got) != bad).sum()))
            ok = ~bad
            err = np.abs(got.astype(np.float64) - w[:, None, None] * vols[:, 0])[ok].max()
            assert err <= 2.0 * TOL[interp]                                              # max |w| = 2
    finally:
        sv.close()


# ---- 9. refusals and sequences ---------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable():
    lib = _native.load()
    ms = batch()
    m1 = np.ascontiguousarray(ms[:1], dtype=np.float32)
    out = np.zeros((1,) + OUT, np.float32)
    p0 = np.zeros(1, np.int32)

    def call(h, n=1, mat=m1, planes=p0, w=None, shape=OUT, flags=0, f64=False):
        fn = lib.vt_volume_affine_stack_f64 if f64 else lib.vt_volume_affine_stack
        mat = np.ascontiguousarray(mat, dtype=np.float64 if f64 else np.float32)
        return fn(h, n, mat.ctypes.data, None if planes is None else planes.ctypes.data, None if w is None else w.ctypes.data,
                  *shape, out.ctypes.data, flags)

    # filt_* without VT_STACK, in Python and by the library; VT_EDGE_SCIPY
    sv = vt.StaticVolume(data(), interpolation='filt_bspline', device='gpu:0')
    with pytest.raises(ValueError):
        sv.affine_stack(ms, OUT, planes=PLANES)
    assert call(sv._handle) == VT_EUNSUPPORTED and b'VT_STACK' in lib.vt_last_error()
    assert call(sv._handle, f64=True) == VT_EUNSUPPORTED
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()
    sv = vt.StaticVolume(data(), device='gpu:0', edge='scipy')
    assert call(sv._handle) == VT_EUNSUPPORTED and b'EDGE_SCIPY' in lib.vt_last_error()
    with pytest.raises(RuntimeError, match=f'code {VT_EUNSUPPORTED}'):
        sv.affine_stack(ms, OUT, planes=PLANES)
    assert sv.affine(np.eye(4, dtype=np.float32)).shape == STACK
    sv.close()

    sv = handle('bspline')
    hd = sv._handle
    want = sv.affine_stack(m1, OUT, planes=[0]).copy()
    assert want.any()
    bad = m1.copy()
    bad[0, 1, 2] = np.nan
    assert call(hd, mat=bad) == VT_EINVAL and b'finite' in lib.vt_last_error()
    assert call(hd, mat=bad, f64=True) == VT_EINVAL
    with pytest.raises(RuntimeError, match='finite'):
        sv.affine_stack(bad, OUT, planes=[0])
    for p in ([STACK[0]], [-1]):
        assert call(hd, planes=np.array(p, np.int32)) == VT_EINVAL and b'plane' in lib.vt_last_error()
        with pytest.raises(ValueError):
            sv.affine_stack(m1, OUT, planes=p)
    assert call(hd, planes=None) == VT_EINVAL and b'plane' in lib.vt_last_error()           # n = 1 != T
    assert call(hd, w=np.array([np.inf])) == VT_EINVAL and b'weight' in lib.vt_last_error()
    for shape in ((0, 45), (37, -1)):
        assert call(hd, shape=shape) == VT_EINVAL
    assert call(hd, n=0) == VT_EINVAL and call(hd, n=-2) == VT_EINVAL
    assert call(hd, n=1 << 29) == VT_EUNSUPPORTED and b'grid' in lib.vt_last_error()        # 2^29 images x 9 tiles, before anything is read
    assert call(hd, n=1 << 29, f64=True) == VT_EUNSUPPORTED
    # the handle still answers; flags other than the routes' and VT_OUT_DEVICE are ignored
    _native.check(call(hd, flags=_native.KEEP_OUTSIDE | _native.ACCUMULATE), 'affine_stack')
    assert same_bits(out, want)
    _native.check(call(hd, f64=True), 'affine_stack_f64')
    assert same_bits(out, want)
    sv.close()


@pytest.mark.parametrize('interp', ['linear', 'filt_bspline'])
def test_sequence_on_one_handle_gives_the_bits_of_fresh_handles(interp):
    """backproject -> affine_stack -> backproject_boxes -> affine_stack on one handle: the calls share the table buffers."""
    ms = batch()
    vol, box = (12, 20, 24), (10, 18, 18)
    bp = vt.utils.backproject_matrices(np.linspace(-50.0, 50.0, 6), 1, vol, STACK)
    bx = vt.utils.backproject_box_matrices([[5.0, 9.0, 11.5], [6.5, 10.0, 8.0]], np.linspace(-50.0, 50.0, 6), 1, vol, box, STACK[1:])

    def steps(sv, which):
        if which == 0:
            return sv.backproject(bp, vol)
        if which == 1:
            return sv.affine_stack(ms, OUT, WEIGHTS, planes=PLANES)
        if which == 2:
            return sv.backproject_boxes(bx, box)
        return sv.affine_stack(ms[:6][::-1], OUT32)

    fresh = []
    for which in range(4):
        sv = handle(interp)
        fresh.append(steps(sv, which).copy())
        sv.close()
    sv = handle(interp)
    for which, kernel in zip(range(4), (18, 21, 19, 21)):
        got = steps(sv, which)
        assert sv.info().last_kernel == kernel and same_bits(got, fresh[which]), (interp, which)
    sv.close()


# ---- 10. align_stack -------------------------------------------------------------------------------------------------------------------
def test_align_stack_round_trip():
    stack = data()
    sh = np.array([[3, -4], [0, 0], [-7, 2], [1, 1], [10, -12], [-2, 9]])
    sv = handle('linear')
    moved = sv.align_stack(sh)
    assert sv.info().last_kernel == 21 and moved.shape == STACK
    sv.close()
    sv = handle('linear', moved)
    back = sv.align_stack(-sh)
    sv.close()
    for i, (a, b) in enumerate(sh):
        # pixel p of `back` is pixel p of the image wherever p + shift is inside the image as well
        h = np.arange(STACK[1])[:, None] + a
        w = np.arange(STACK[2])[None, :] + b
        ok = (h >= 0) & (h < STACK[1]) & (w >= 0) & (w < STACK[2])
        assert ok.any() and same_bits(back[i][ok], stack[i][ok]), i
        assert not bits(back[i][~ok]).any()
    # turned, magnified and moved: the matrices are utils.stack_matrices'
    sv = handle('bspline')
    rot_, sc = np.linspace(-20.0, 20.0, 6), np.linspace(0.8, 1.25, 6)
    got = sv.align_stack(sh + 0.25, rot_, sc, OUT)
    ms = vt.utils.stack_matrices(sh + 0.25, rot_, sc, STACK, OUT)
    assert same_bits(got, sv.affine_stack(ms, OUT))
    m4 = np.zeros((6, 4, 4))
    m4[:, 0, 0] = 1
    m4[:, 1:, 1:] = ms
    vols, _ = bm.per_entry(stack, m4, None, (1,) + OUT, 'bspline')
    check_entries(got, vols[:, 0], np.ones(6), TOL['bspline'], 'align_stack')
    sv.close()
