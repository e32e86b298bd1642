"""StaticVolume.affine_stack without a GPU: the device='cpu' path against the float64 model of tests/backproject_model.py (per_entry at
an output of depth 1 is the definition), the matrices of utils.stack_matrices, the 3 x 3 embedding, argument errors, library codes and
symbols."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

import backproject_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
STACK = (5, 64, 72)
OUT = (20, 24)
INTERPS = ['linear', 'bspline', 'bspline_simple', 'filt_bspline', 'filt_bspline_simple']
PLANES = np.array([3, 0, 4, 4, 1, 2, 0, 1, 2, 3])
WTS = np.array([0.5, -1.25, 2.0, 0.0, 0.75, 1.0, -0.5, 1.5, 0.25, 1.0])
N = len(PLANES)
Z = abs(np.sqrt(3.0) - 2.0)
# pixels compared: those whose coordinates stay this far inside the image.  2 (linear) and 4 (cubic): scipy's 'constant' boundary differs
# from the zero border of the model inside the stencil's reach of the edge.  filt_*: 14, test_backproject_host.py's MARGIN -- scipy's
# coefficients (mirror boundary) approach the library's (prefilter_model.prefilter_f64) as |z|^k only.
MARGIN = {'linear': 2, 'bspline': 4, 'bspline_simple': 4, 'filt_bspline': 14, 'filt_bspline_simple': 14}


@pytest.fixture(scope='module')
def stack():
    s = np.random.RandomState(11).random_sample(STACK).astype(np.float32)
    s.setflags(write=False)
    return s


def embed(m3):
    """(n, 3, 3) -> (n, 4, 4): rows and columns 1, 2, 3; row 0 and column 0 are junk on purpose, they are ignored."""
    m3 = np.asarray(m3)
    m4 = np.zeros((len(m3), 4, 4), m3.dtype)
    m4[:, 0] = (0.3, -0.7, 0.2, 11.0)
    m4[:, 1:, 0] = (0.25, -0.5, 7.0)
    m4[:, 1:, 1:] = m3
    return m4


def model_m4(m3):
    """What the model takes: the embedding with column 0 zero (the model multiplies it by d = 0 all the same)."""
    m4 = embed(np.asarray(m3, np.float64))
    m4[:, :, 0] = 0
    return m4


def batch():
    """Ten float64 (3, 3) matrices onto OUT: a rotation by 30 degrees, a rotation with magnification 1.3, an integer shift, a sub-pixel
    shift, a shear, one whose footprint leaves the image on one side, and four more turns and magnifications inside the image."""
    ms = vt.utils.stack_matrices(shifts=[[1.5, -2.25], [0.0, 3.0], [4.0, -6.0], [0.375, 0.625], [0.0, 0.0], [0.0, 0.0], [2.5, 1.0], [-1.0, 0.5],
                                         [0.0, -3.5], [1.25, 1.25]],
                                 rotations=[30.0, -17.0, 0.0, 0.0, 0.0, 0.0, 45.0, 90.0, -120.0, 7.5],
                                 scales=[1.0, 1.3, 1.0, 1.0, 1.0, 1.0, 0.8, 1.0, 2.0, 0.75], image_shape=STACK, output_shape=OUT)
    ms[4, :2] = [(1.0, 0.25, 21.0), (-0.125, 1.0, 26.0)]
    ms[5, :2] = [(1.0, 0.0, 46.0), (0.0, 1.0, 20.5)]                  # rows 46 .. 65: the last two are beyond the image
    return ms


def cpu_bound(interp, w, stack):
    """The CPU path samples in float64 and rounds the sample and the weighted value to float32, the model is float64: two roundings of
    values below 2, 2^-21 |w|.  filt_*: test_backproject_host.py's bound on scipy's coefficients against prefilter_f64's, 42 max|s|
    |z|^(k - 2) at k pixels from the edge."""
    b = 2.0 ** -21 * abs(w)
    if interp in bm.FILTERED:
        b += abs(w) * 42.0 * float(np.abs(stack).max()) * Z ** (MARGIN[interp] - 2)
    return b


# ---- the CPU device path against the model ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('interp', INTERPS)
def test_cpu_device_path_against_the_model(interp, stack):
    ms = batch()
    H, W = STACK[1:]
    k = MARGIN[interp]
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    for mats in (ms, ms.astype(np.float32)):
        m4 = model_m4(mats)
        vols, masks = bm.per_entry(stack, m4, PLANES, (1,) + OUT, interp)
        got = sv.affine_stack(mats, OUT, WTS, planes=PLANES)
        assert got.dtype == np.float32 and got.shape == (N,) + OUT
        kept = 0
        for i in range(N):
            y, x = bm.coords(m4[i], (1,) + OUT)
            keep = ((y >= k) & (y <= H - 1 - k) & (x >= k) & (x <= W - 1 - k))[0]
            kept += int(keep.sum())
            err = float(np.abs(got[i].astype(np.float64) - WTS[i] * vols[i, 0])[keep].max()) if keep.any() else 0.0
            bound = cpu_bound(interp, WTS[i], stack)
            print(f'{interp} {mats.dtype} entry {i}: kept {int(keep.sum())}/{keep.size}  max|cpu - model| {err:.3e}  bound {bound:.3e}')
            assert err <= bound, (interp, i, err, bound)
            # beyond the image the CPU path writes 0 as the model does
            far = ((y < -1) | (y > H) | (x < -1) | (x > W))[0]
            assert not got[i][far].any()
        assert kept >= 0.9 * N * OUT[0] * OUT[1], kept
        assert not masks[5].all() and masks[5].any()
    # the (n, 4, 4) form with junk in row 0 and column 0 gives the same bits; planes=None pairs matrix i with image i
    assert np.array_equal(sv.affine_stack(embed(ms), OUT, WTS, planes=PLANES), sv.affine_stack(ms, OUT, WTS, planes=PLANES))
    assert np.array_equal(sv.affine_stack(ms[:5], OUT), sv.affine_stack(ms[:5], OUT, np.ones(5), planes=np.arange(5)))
    # output=, and the default output shape
    out = np.full((N,) + OUT, 7, np.float32)
    assert sv.affine_stack(ms, OUT, WTS, output=out, planes=PLANES) is out
    assert np.array_equal(out, sv.affine_stack(ms, OUT, WTS, planes=PLANES))
    assert sv.affine_stack(ms[:5]).shape == STACK


def test_cpu_stack_prefilters_per_plane(stack):
    other = np.array(stack)
    other[2] = np.random.RandomState(9).random_sample(STACK[1:]).astype(np.float32)
    ms = batch()
    keep = PLANES != 2
    a = vt.StaticVolume(stack, 'filt_bspline', 'cpu', stack=True).affine_stack(ms[keep], OUT, planes=PLANES[keep])
    b = vt.StaticVolume(other, 'filt_bspline', 'cpu', stack=True).affine_stack(ms[keep], OUT, planes=PLANES[keep])
    c = vt.StaticVolume(other, 'filt_bspline', 'cpu', stack=True).affine_stack(ms[~keep], OUT, planes=PLANES[~keep])
    d = vt.StaticVolume(stack, 'filt_bspline', 'cpu', stack=True).affine_stack(ms[~keep], OUT, planes=PLANES[~keep])
    assert np.array_equal(a, b) and a.any() and not np.array_equal(c, d)


def test_cpu_align_stack(stack):
    sv = vt.StaticVolume(stack, device='cpu')
    sh = np.array([[1.0, -2.0], [0.5, 0.25], [0.0, 0.0], [-3.0, 4.0], [2.0, 2.0]])
    rot = np.array([0.0, 10.0, -20.0, 0.0, 5.0])
    sc = np.array([1.0, 1.1, 0.9, 1.0, 1.0])
    ms = vt.utils.stack_matrices(sh, rot, sc, STACK[1:], OUT)
    assert np.array_equal(sv.align_stack(sh, rot, sc, OUT), sv.affine_stack(ms, OUT))
    got = sv.align_stack(sh, weights=WTS[:5], planes=[4, 3, 2, 1, 0])
    assert np.array_equal(got, sv.affine_stack(vt.utils.stack_matrices(sh, image_shape=STACK), None, WTS[:5], planes=[4, 3, 2, 1, 0]))
    # an integer shift moves the image: output pixel p shows image pixel p - shift
    assert np.array_equal(got[0][1:, :-2], np.float32(WTS[0]) * stack[4][:-1, 2:])


# ---- the matrices ----------------------------------------------------------------------------------------------------------------
def test_stack_matrices_identity_and_crop():
    ms = vt.utils.stack_matrices(shifts=np.zeros((3, 2)), image_shape=(40, 52))
    assert ms.shape == (3, 3, 3) and ms.dtype == np.float64
    assert np.array_equal(ms, np.broadcast_to(np.eye(3), (3, 3, 3)))
    assert np.array_equal(vt.utils.stack_matrices(rotations=[0.0], image_shape=(7, 40, 52), output_shape=(40, 52))[0], np.eye(3))
    assert np.array_equal(vt.utils.stack_matrices(scales=[1.0, 1.0], image_shape=(41, 51))[1], np.eye(3))
    # an integer shift onto a smaller output of the same parity is a plain crop: q = p + (ci - co - shift), all integers
    ms = vt.utils.stack_matrices(shifts=[[3, -2], [-4, 6]], image_shape=(40, 52), output_shape=(20, 30))
    for m, off in zip(ms, ((7, 13), (14, 5))):
        assert np.array_equal(m, [[1, 0, off[0]], [0, 1, off[1]], [0, 0, 1]]), m
    img = np.arange(2 * 40 * 52, dtype=np.float32).reshape(2, 40, 52)
    got = vt.StaticVolume(img, device='cpu').affine_stack(ms, (20, 30))
    assert np.array_equal(got[0], img[0, 7:27, 13:43]) and np.array_equal(got[1], img[1, 14:34, 5:35])


@pytest.mark.parametrize('units', ['deg', 'rad'])
def test_stack_matrices_definition_and_inverse(units):
    """q = ci + R^T (p - co - shift) / s.  The inverse map of (shift, theta, k) is again of the family: (-R^T shift / k, -theta, 1 / k)
    -- the shift is carried through the turn and the magnification, so negating all three parameters inverts the map when only the shift
    or only the turn and the magnification are given, and with the carried shift otherwise.  All to 1e-12 (test_place_host.py's
    bound)."""
    th = np.array([30.0, -75.5, 180.0, 0.0, 12.0])
    k = np.array([1.0, 1.3, 0.5, 2.0, 0.8])
    s = np.array([[1.5, -2.25], [0.0, 3.0], [-7.0, 0.125], [4.0, 4.0], [0.0, 0.0]])
    rad = np.deg2rad(th)
    ang = rad if units == 'rad' else th
    shape = (40, 52)
    fwd = vt.utils.stack_matrices(s, ang, k, shape, rotation_units=units)
    c = np.array([19.5, 25.5])
    for i in range(5):
        R = np.array([[np.cos(rad[i]), -np.sin(rad[i])], [np.sin(rad[i]), np.cos(rad[i])]])
        for p in ([0.0, 0.0], [39.0, 51.0], [7.25, 30.5]):
            want = c + R.T @ (np.asarray(p) - c - s[i]) / k[i]
            assert np.abs((fwd[i] @ [p[0], p[1], 1.0])[:2] - want).max() <= 1e-12
    eye = np.broadcast_to(np.eye(3), (5, 3, 3))
    # shifts alone; turns and magnifications alone
    a, b = vt.utils.stack_matrices(s, image_shape=shape), vt.utils.stack_matrices(-s, image_shape=shape)
    assert np.abs(a @ b - eye).max() <= 1e-12 and np.abs(b @ a - eye).max() <= 1e-12
    a = vt.utils.stack_matrices(None, ang, k, shape, rotation_units=units)
    b = vt.utils.stack_matrices(None, -ang, 1.0 / k, shape, rotation_units=units)
    assert np.abs(a @ b - eye).max() <= 1e-12 and np.abs(b @ a - eye).max() <= 1e-12
    # all three: the shift carried through
    carried = np.stack([-(np.array([[np.cos(r), -np.sin(r)], [np.sin(r), np.cos(r)]]).T @ si) / ki for r, si, ki in zip(rad, s, k)])
    inv = vt.utils.stack_matrices(carried, -ang, 1.0 / k, shape, rotation_units=units)
    assert np.abs(fwd @ inv - eye).max() <= 1e-12 and np.abs(inv @ fwd - eye).max() <= 1e-12
    # other centres: the image centre goes to the output centre plus the shift
    m = vt.utils.stack_matrices(s, ang, k, (40, 52), (31, 70), units)
    for i in range(5):
        got = m[i] @ [15.0 + s[i, 0], 34.5 + s[i, 1], 1.0]
        assert np.abs(got[:2] - c).max() <= 1e-12


def test_stack_matrices_errors():
    for kw in (dict(), dict(shifts=[[1, 2]]), dict(shifts=[1, 2], image_shape=(4, 5)), dict(shifts=[[1, 2]], rotations=[1, 2], image_shape=(4, 5)),
               dict(scales=[0.0], image_shape=(4, 5)), dict(scales=[np.nan], image_shape=(4, 5)), dict(rotations=[np.inf], image_shape=(4, 5)),
               dict(rotations=[1.0], image_shape=(4,)), dict(rotations=[1.0], image_shape=(4, 0)), dict(rotations=[1.0], image_shape=(4, 5.0)),
               dict(rotations=[1.0], image_shape=(4, 5), output_shape=7), dict(rotations=[1.0], image_shape=(4, 5), rotation_units='turns'),
               dict(rotations=[], image_shape=(4, 5)), dict(rotations=3.0, image_shape=(4, 5))):
        with pytest.raises(ValueError):
            vt.utils.stack_matrices(**kw)


# ---- argument errors -------------------------------------------------------------------------------------------------------------
def test_argument_errors(stack):
    sv = vt.StaticVolume(stack, device='cpu')
    ms = batch()
    for bad in (np.eye(3), np.eye(4, dtype=np.float32), np.zeros((0, 3, 3)), np.zeros((2, 3, 4)), np.zeros((2, 2, 2)), np.zeros((2, 5, 5))):
        with pytest.raises(ValueError):
            sv.affine_stack(bad, OUT, planes=[0] * len(bad))
    with pytest.raises(ValueError):
        sv.affine_stack(ms, OUT, WTS[:4], planes=PLANES)
    with pytest.raises(ValueError):
        sv.affine_stack(ms, OUT, np.ones((N, 1)), planes=PLANES)
    for bad in (np.nan, np.inf):
        w = WTS.copy()
        w[2] = bad
        with pytest.raises(ValueError):
            sv.affine_stack(ms, OUT, w, planes=PLANES)
    with pytest.raises(ValueError):
        sv.affine_stack(ms, OUT)                                                            # planes=None with n = 10 != T = 5
    with pytest.raises(ValueError):
        sv.affine_stack(ms[:3], OUT)
    for bad in ([0, 1, 2, 3, 4, 5, 0, 0, 0, 0], [0, 1, 2, 3, 4, -1, 0, 0, 0, 0], [0, 1, 2, 3], [0.0, 1.0, 2.0, 3.0, 4.0, 0.0, 0.0, 0.0, 0.0, 0.0], [[0, 1, 2, 3, 4, 0, 0, 0, 0, 0]]):
        with pytest.raises(ValueError):
            sv.affine_stack(ms, OUT, planes=bad)
    for bad in (np.zeros((N, 20, 25), np.float32), np.zeros((5,) + OUT, np.float32), np.zeros(OUT, np.float32)):
        with pytest.raises(ValueError):
            sv.affine_stack(ms, OUT, output=bad, planes=PLANES)
    for shape in ((0, 12), (6, 8, 12), (6, 8.0), (6,), 5):
        with pytest.raises(ValueError):
            sv.affine_stack(ms, shape, planes=PLANES)
    # prefiltered coefficients that mix the images are refused
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, 'filt_bspline', 'cpu').affine_stack(ms, OUT, planes=PLANES)
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, 'filt_bspline_simple', 'cpu').align_stack(np.zeros((5, 2)))


# ---- the library without a GPU ---------------------------------------------------------------------------------------------------
def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    w = np.ones(1)
    pl = np.zeros(1, np.int32)
    out = np.zeros((1, 4, 4), np.float32)
    assert lib.vt_volume_affine_stack(None, 1, m32.ctypes.data, pl.ctypes.data, w.ctypes.data, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_affine_stack_f64(None, 1, m64.ctypes.data, pl.ctypes.data, w.ctypes.data, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_affine_stack_f64(None, 1, m64.ctypes.data, None, None, 4, 4, out.ctypes.data, _native.FORCE_DIRECT) == VT_EINVAL
    assert b'NULL' in lib.vt_last_error()


def test_symbols_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_affine_stack', 'vt_volume_affine_stack_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 9
    assert '21 per-image 2-D transforms of a stack' in header                  # the last_kernel comment names the new kernel
    assert 'stack_matrices' in dir(vt.utils)
