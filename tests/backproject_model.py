"""A float64 numpy model of StaticVolume.backproject (vt_volume_backproject, kernel 18), written from the definition in
include/voltools_hip.h and sharing nothing with the library:

  * (y, x) of output voxel (d, h, w) by the fma chain fma(m0, d, fma(m1, h, fma(m2, w, t))) on rows 1 and 2 of the matrix (fma emulated
    as box_index_model does: the longdouble product-sum rounded to float64),
  * floor / fraction, four (bilinear) or sixteen (cubic B-spline) taps of the image with a border of zeros,
  * the skirt rule -0.5 <= y < H - 0.5 and -0.5 <= x < W - 0.5 on those coordinates,
  * for filt_* the coefficients of prefilter_model.prefilter_f64 applied to every image on its own,
  * out = float32(base + sum_i w_i B_i) in float64.

The interpolation arithmetic is float64 throughout; what the library does in float32 is covered by the tolerances of the tests."""
import numpy as np

import prefilter_model as pm

_LD = np.longdouble
CUBIC = ('bspline', 'bspline_simple', 'filt_bspline', 'filt_bspline_simple')
FILTERED = ('filt_bspline', 'filt_bspline_simple')


def _fma(a, x, c):
    return (_LD(a) * np.asarray(x, _LD) + np.asarray(c, _LD)).astype(np.float64)


def coords(m, shape):
    """float64 (y, x) of every output voxel, each of shape `shape`."""
    m = np.asarray(m, np.float64)
    d = np.arange(shape[0]).reshape(-1, 1, 1)
    h = np.arange(shape[1]).reshape(1, -1, 1)
    w = np.arange(shape[2]).reshape(1, 1, -1)
    out = []
    for r in (1, 2):
        s = _fma(m[r, 0], d, _fma(m[r, 1], h, _fma(m[r, 2], w, m[r, 3])))
        out.append(np.broadcast_to(s, shape))
    return out[0], out[1]


def inside(y, x, H, W):
    return (y >= -0.5) & (y < H - 0.5) & (x >= -0.5) & (x < W - 0.5)


def _weights(f, simple):
    """The four cubic B-spline weights at fraction f (taps -1, 0, 1, 2); both forms of the library are the same polynomial."""
    del simple
    g = 1.0 - f
    return [g * g * g / 6.0, 2.0 / 3.0 - 0.5 * f * f * (2.0 - f), 2.0 / 3.0 - 0.5 * g * g * (2.0 - g), f * f * f / 6.0]


def _tap(img, iy, ix):
    H, W = img.shape
    ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    return np.where(ok, img[np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], 0.0)


def sample(img, y, x, interp):
    """The 2-D interpolation of float64 image `img` at (y, x), zero border, no skirt rule."""
    fy0, fx0 = np.floor(y), np.floor(x)
    fy, fx = y - fy0, x - fx0
    iy, ix = fy0.astype(np.int64), fx0.astype(np.int64)
    if interp == 'linear':
        a00, a01 = _tap(img, iy, ix), _tap(img, iy, ix + 1)
        a10, a11 = _tap(img, iy + 1, ix), _tap(img, iy + 1, ix + 1)
        x0 = a00 + fx * (a01 - a00)
        x1 = a10 + fx * (a11 - a10)
        return x0 + fy * (x1 - x0)
    wy, wx = _weights(fy, interp.endswith('simple')), _weights(fx, interp.endswith('simple'))
    val = np.zeros(y.shape, np.float64)
    for b in range(4):
        row = np.zeros(y.shape, np.float64)
        for a in range(4):
            row += wx[a] * _tap(img, iy - 1 + b, ix - 1 + a)
        val += wy[b] * row
    return val


def images(stack, interp):
    """What the interpolation reads, float64 (T, H, W): the float32 samples, or for filt_* each image's own coefficients."""
    s = np.asarray(stack, np.float32).astype(np.float64)
    if interp in FILTERED:
        return np.stack([pm.prefilter_f64(s[k]) for k in range(s.shape[0])])
    return s


def per_entry(stack, ms, planes, shape, interp):
    """(n,) + shape float64: B_i of every entry (0 outside the skirt), and the boolean inside masks."""
    img = images(stack, interp)
    T, H, W = img.shape
    planes = range(len(ms)) if planes is None else planes
    vols, masks = [], []
    for m, k in zip(ms, planes):
        assert 0 <= int(k) < T
        y, x = coords(m, shape)
        ins = inside(y, x, H, W)
        vols.append(np.where(ins, sample(img[int(k)], y, x, interp), 0.0))
        masks.append(ins)
    return np.stack(vols), np.stack(masks)


def backproject(stack, ms, planes, weights, shape, interp, base=None):
    vols, _ = per_entry(stack, ms, planes, shape, interp)
    w = np.ones(len(ms)) if weights is None else np.asarray(weights, np.float64)
    acc = np.zeros(shape, np.float64) if base is None else np.asarray(base).astype(np.float64)
    for i in range(len(ms)):
        acc = acc + w[i] * vols[i]
    return acc.astype(np.float32)
