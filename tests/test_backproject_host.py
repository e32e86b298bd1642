"""StaticVolume.backproject without a GPU: the float64 model of tests/backproject_model.py against the project's oracle, the matrices of
utils.backproject_matrices, the device='cpu' path against the model, argument errors, library codes, symbols and the new create flag."""
import os
import re

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native
from oracle import oracle

import backproject_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VT_EINVAL = 10001
TOL = 1e-6                             # TOL[interp] of tests/test_gpu_extract.py for linear, bspline and bspline_simple
STACK = (5, 40, 52)
ANGLES = (-60.0, -30.5, 0.0, 20.0, 45.0)
INTERPS = ['linear', 'bspline', 'bspline_simple', 'filt_bspline', 'filt_bspline_simple']
Z = abs(np.sqrt(3.0) - 2.0)


@pytest.fixture(scope='module')
def stack():
    s = np.random.RandomState(11).random_sample(STACK).astype(np.float32)
    s.setflags(write=False)
    return s


def plane_row(m, plane):
    p = np.array(m, np.float64)
    p[0] = (0.0, 0.0, 0.0, float(plane))
    return p


# ---- the model against the project's oracle --------------------------------------------------------------------------------
@pytest.mark.parametrize('out', [(24, 28, 40), (20, 48, 60)])
@pytest.mark.parametrize('interp', ['linear', 'bspline', 'bspline_simple'])
def test_model_against_the_oracle(interp, out, stack):
    """Linear: the trilinear sample at an exactly integer plane is the bilinear sample in that plane.  Cubic: three equal planes meet the
    z weights 1/6 + 4/6 + 1/6.  The second output is larger than the image, so skirt and zero-border voxels are compared too."""
    ms = vt.utils.backproject_matrices(ANGLES, 1, out, STACK).astype(np.float32)
    vols, masks = bm.per_entry(stack, ms, None, out, interp)
    assert masks.any()
    if out[1] > STACK[1]:
        assert (~masks).any() and all(mk.any() for mk in masks)
    worst = 0.0
    for i in range(len(ms)):
        if interp == 'linear':
            want = oracle.affine_ex(stack, plane_row(ms[i], i), interp, out)
        else:
            want = oracle.affine_ex(np.repeat(stack[i][None], 3, 0), plane_row(ms[i], 1), interp, out)
        assert np.array_equal(want != 0, masks[i] & (want != 0)) and not want[~masks[i]].any(), (interp, i)
        worst = max(worst, float(np.abs(vols[i] - want.astype(np.float64)).max()))
    print(f'{interp} {out}: max|model - oracle| {worst:.3e}')
    assert worst <= TOL, (interp, worst)


# ---- the matrices --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('axis', [0, 1, 2])
@pytest.mark.parametrize('units', ['deg', 'rad'])
def test_backproject_matrices_invert_tilt_matrices(axis, units):
    angles = np.array([-60.0, -12.5, 0.0, 33.0, 90.0])
    if units == 'rad':
        angles = np.deg2rad(angles)
    shape = (24, 28, 40)
    for center in (None, (3.0, 10.5, 7.25)):
        fwd = np.asarray(vt.utils.tilt_matrices(angles, axis, shape, units, center), np.float64)
        inv = vt.utils.backproject_matrices(angles, axis, shape, None, units, center)
        assert inv.shape == (5, 4, 4) and inv.dtype == np.float64
        eye = np.broadcast_to(np.eye(4), (5, 4, 4))
        assert np.abs(inv @ fwd - eye).max() <= 1e-12 and np.abs(fwd @ inv - eye).max() <= 1e-12      # test_place_host.py's bound
        assert np.array_equal(inv[:, 3], np.broadcast_to([0.0, 0.0, 0.0, 1.0], (5, 4)))


def test_backproject_matrices_image_shape_shift_and_errors():
    shape = (24, 28, 40)
    base = vt.utils.backproject_matrices(ANGLES, 1, shape)
    for image in ((40, 52), (7, 40, 52)):
        got = vt.utils.backproject_matrices(ANGLES, 1, shape, image)
        want = base.copy()
        want[:, 1, 3] += (40 - 1) / 2 - (28 - 1) / 2
        want[:, 2, 3] += (52 - 1) / 2 - (40 - 1) / 2
        assert np.array_equal(got, want)
    assert np.array_equal(vt.utils.backproject_matrices(ANGLES, 1, shape, shape[1:]), base)
    # the centre of the volume lands on the centre of the image
    c = np.array([11.5, 13.5, 19.5, 1.0])
    got = vt.utils.backproject_matrices(ANGLES, 1, shape, (40, 52)) @ c
    assert np.abs(got[:, 1] - 19.5).max() <= 1e-5 and np.abs(got[:, 2] - 25.5).max() <= 1e-5
    for bad in ((40,), (40, 0), (40, 52.0), (1, 2, 3, 4), 5):
        with pytest.raises(ValueError):
            vt.utils.backproject_matrices(ANGLES, 1, shape, bad)
    for bad in ((24, 28), None, (24, 0, 40)):
        with pytest.raises(ValueError):
            vt.utils.backproject_matrices(ANGLES, 1, bad)
    with pytest.raises(ValueError):
        vt.utils.backproject_matrices(ANGLES, 3, shape)
    with pytest.raises(ValueError):
        vt.utils.backproject_matrices([], 1, shape)


# ---- the CPU device path against the model -----------------------------------------------------------------------------------
OUT_IN = (6, 8, 12)
MARGIN = 14                            # pixels between every footprint and the nearest image edge
W5 = np.array([0.5, -1.25, 2.0, 0.0, 0.75])
PLANES = np.array([3, 0, 4, 4, 1])


def interior_matrices():
    """Five float64 matrices whose footprints of OUT_IN stay MARGIN pixels inside a 40 x 52 image."""
    rs = np.random.RandomState(5)
    ms = np.zeros((5, 4, 4))
    ms[:, 3, 3] = 1.0
    ms[:, 0, :3] = rs.uniform(-1, 1, (5, 3))            # row 0 is ignored
    ms[:, 0, 3] = 100.0
    ms[:, 1] = [(0.3, 0.8, 0.1, 14.5), (-0.3, 0.9, -0.2, 18.25), (0.0, 1.0, 0.0, 15.0), (0.5, 0.5, 0.25, 14.125), (0.25, -0.75, 0.1, 22.0)]
    ms[:, 2] = [(0.4, 0.2, 1.5, 15.25), (0.2, -0.3, 1.25, 18.5), (0.0, 0.0, 1.0, 20.0), (-0.5, 0.25, 1.0, 20.5), (0.3, 0.3, -1.5, 33.0)]
    return ms


def cpu_bound(interp, w, stack):
    """linear and the unfiltered cubics: 1e-5 * sum|w| (float32 values of O(1) against float64, the bound of test_place_host.py's CPU
    comparisons).  filt_*: the CPU path's coefficients are scipy's (mirror boundary), the model's are prefilter_f64's (the library's
    boundary); both solve the same recursion, so along one axis they differ by a solution of the homogeneous recursion: at most
    3.5 max|s| |z|^k from either end, k samples from it (the start values differ by at most lambda max|s| (1 + 2|z| / (1 - |z|)), the
    anticausal pass scales that by |z| / (1 - z^2)).  The second pass multiplies the first one's error by the filter's gain
    sqrt(3) (1 + |z|) / (1 - |z|) = 3 and adds its own on data of up to 3 max|s|: 42 max|s| |z|^k in the plane, and interpolation
    weights are non-negative and sum to 1.  tests/test_prefilter_model.py holds the same decay at k = 24; tests/test_cpu_path.py, which
    compares bits with the reference's own outputs, has no figure for it.  k = MARGIN - 2 (the stencil reaches 2 further)."""
    b = 1e-5 * np.abs(w).sum()
    if interp in bm.FILTERED:
        b += np.abs(w).sum() * 42.0 * float(np.abs(stack).max()) * Z ** (MARGIN - 2)
    return b


@pytest.mark.parametrize('interp', INTERPS)
def test_cpu_device_path_against_the_model(interp, stack):
    ms = interior_matrices()
    H, W = STACK[1:]
    for m in ms:
        y, x = bm.coords(m, OUT_IN)
        assert y.min() >= MARGIN and y.max() <= H - 1 - MARGIN and x.min() >= MARGIN and x.max() <= W - 1 - MARGIN
    sv = vt.StaticVolume(stack, interpolation=interp, device='cpu', stack=True)
    want = bm.backproject(stack, ms, PLANES, W5, OUT_IN, interp).astype(np.float64)
    bound = cpu_bound(interp, W5, stack)
    for mats in (ms, ms.astype(np.float32)):
        got = sv.backproject(mats, OUT_IN, W5, planes=PLANES)
        want_m = want if mats.dtype == np.float64 else bm.backproject(stack, mats, PLANES, W5, OUT_IN, interp).astype(np.float64)
        err = float(np.abs(got.astype(np.float64) - want_m).max())
        print(f'{interp} {mats.dtype}: max|cpu - model| {err:.3e}  bound {bound:.3e}')
        assert got.dtype == np.float32 and got.shape == OUT_IN and err <= bound, (interp, err)
    # planes=None: image i belongs to matrix i
    got = sv.backproject(ms, OUT_IN)
    want = bm.backproject(stack, ms, None, None, OUT_IN, interp).astype(np.float64)
    assert np.abs(got - want).max() <= cpu_bound(interp, np.ones(5), stack)
    # accumulate starts from the output
    base = np.random.RandomState(2).standard_normal(OUT_IN).astype(np.float32)
    out = base.copy()
    assert sv.backproject(ms, OUT_IN, W5, output=out, planes=PLANES, accumulate=True) is out
    want = bm.backproject(stack, ms, PLANES, W5, OUT_IN, interp, base=base).astype(np.float64)
    assert np.abs(out - want).max() <= bound + 2.0 ** -23 * np.abs(want).max()
    assert not np.array_equal(out, base)
    # without accumulate the output's contents do not count
    out2 = base.copy()
    sv.backproject(ms, OUT_IN, W5, output=out2, planes=PLANES)
    assert np.array_equal(out2, sv.backproject(ms, OUT_IN, W5, planes=PLANES))


def test_cpu_stack_prefilters_per_plane(stack):
    """Two stacks that differ in image 2 only give the same bits for entries that read other images."""
    other = np.array(stack)
    other[2] = np.random.RandomState(9).random_sample(STACK[1:]).astype(np.float32)
    ms = interior_matrices()
    keep = PLANES != 2
    a = vt.StaticVolume(stack, 'filt_bspline', 'cpu', stack=True).backproject(ms[keep], OUT_IN, W5[keep], planes=PLANES[keep])
    b = vt.StaticVolume(other, 'filt_bspline', 'cpu', stack=True).backproject(ms[keep], OUT_IN, W5[keep], planes=PLANES[keep])
    assert np.array_equal(a, b) and a.any()


def test_cpu_backproject_tilts(stack):
    out = (24, 28, 40)
    sv = vt.StaticVolume(stack, device='cpu')
    ms = vt.utils.backproject_matrices(ANGLES, 1, out, STACK[1:])
    assert np.array_equal(sv.backproject_tilts(ANGLES, output_shape=out), sv.backproject(ms, out))
    assert np.array_equal(sv.backproject_tilts(ANGLES, 1, 'deg', None, out, W5), sv.backproject(ms, out, W5))
    with pytest.raises(ValueError):
        sv.backproject_tilts(ANGLES)
    with pytest.raises(ValueError):
        sv.backproject_tilts(ANGLES[:4], output_shape=out)            # four matrices, five images


# ---- argument errors ----------------------------------------------------------------------------------------------------
def test_argument_errors(stack):
    sv = vt.StaticVolume(stack, device='cpu')
    ms = interior_matrices()
    for bad in (np.eye(4, dtype=np.float32), np.zeros((0, 4, 4), np.float32), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError):
            sv.backproject(bad, OUT_IN)
    with pytest.raises(ValueError):
        sv.backproject(ms, OUT_IN, W5[:4])
    with pytest.raises(ValueError):
        sv.backproject(ms, OUT_IN, np.ones((5, 1)))
    for bad in (np.nan, np.inf):
        w = W5.copy()
        w[2] = bad
        with pytest.raises(ValueError):
            sv.backproject(ms, OUT_IN, w)
    with pytest.raises(ValueError):
        sv.backproject(ms[:3], OUT_IN)                                                      # planes=None with n != T
    for bad in ([0, 1, 2, 3, 5], [0, 1, 2, 3, -1], [0, 1, 2, 3], [0.0, 1.0, 2.0, 3.0, 4.0], [[0, 1, 2, 3, 4]]):
        with pytest.raises(ValueError):
            sv.backproject(ms, OUT_IN, planes=bad)
    with pytest.raises(ValueError):
        sv.backproject(ms, OUT_IN, output=np.zeros((6, 8, 13), np.float32))
    for shape in ((6, 0, 12), (6, 8), (6, 8, 12.0), None):
        with pytest.raises(ValueError):
            sv.backproject(ms, shape)
    with pytest.raises(ValueError):
        sv.backproject(ms, OUT_IN, W5, accumulate=True)                                     # nothing to add into
    with pytest.raises(ValueError):
        sv.backproject_tilts(ANGLES, output_shape=OUT_IN, accumulate=True)


def test_stack_argument(stack):
    assert vt.StaticVolume(stack, device='cpu').stack is False
    assert vt.StaticVolume(stack, device='cpu', stack=True).stack is True
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, device='cpu', stack=True, edge='scipy')
    with pytest.raises(ValueError):
        vt.StaticVolume(stack, device='cpu', stack=1)
    with pytest.raises(TypeError):
        vt.StaticVolume(stack, 'linear', 'cpu', 'texture', 0, True)                           # keyword-only
    # prefiltered coefficients that mix the images are refused
    sv = vt.StaticVolume(stack, 'filt_bspline', 'cpu')
    with pytest.raises(ValueError):
        sv.backproject(interior_matrices(), OUT_IN)


# ---- the library without a GPU ----------------------------------------------------------------------------------------------
def test_library_argument_codes_without_a_gpu():
    lib = _native.load()
    m32 = np.eye(4, dtype=np.float32)
    m64 = np.eye(4, dtype=np.float64)
    w = np.ones(1)
    pl = np.zeros(1, np.int32)
    out = np.zeros((4, 4, 4), np.float32)
    assert lib.vt_volume_backproject(None, 1, m32.ctypes.data, pl.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_backproject_f64(None, 1, m64.ctypes.data, pl.ctypes.data, w.ctypes.data, 4, 4, 4, out.ctypes.data, 0) == VT_EINVAL
    assert lib.vt_volume_backproject_f64(None, 1, m64.ctypes.data, None, None, 4, 4, 4, out.ctypes.data, _native.ACCUMULATE) == VT_EINVAL
    assert lib.vt_last_error()


def test_symbols_and_the_create_flag_declared_and_bound():
    header = open(os.path.join(ROOT, 'include', 'voltools_hip.h')).read()
    declared = set(re.findall(r'\b(vt_[a-z0-9_]+)\s*\(', header))
    lib = _native.load()
    for name in ('vt_volume_backproject', 'vt_volume_backproject_f64'):
        assert name in declared and name in _native.SYMBOLS
        assert getattr(lib, name).argtypes is not None and len(getattr(lib, name).argtypes) == 10
    assert '18 a stack of images back-projected into one volume' in header     # the last_kernel comment names the new kernel
    body = re.search(r'enum vt_create_flags \{(.*?)\};', header, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    flags = {k: int(val) for k, val in re.findall(r'\b(VT_[A-Z_]+)\s*=\s*(\d+)', body)}
    assert flags['VT_STACK'] == _native.STACK == 32
    values = list(flags.values())
    assert len(set(values)) == len(values) and all(val & (val - 1) == 0 for val in values)
    assert flags['VT_SRC_DEVICE'] == 1 and flags['VT_EDGE_SCIPY'] == _native.EDGE_SCIPY == 16 and flags['VT_SRC_DEFERRED'] == 8
    # VT_ACCUMULATE's comment names the new call
    assert re.search(r'VT_ACCUMULATE = 262144,/\* vt_volume_place and vt_volume_backproject only', header)
