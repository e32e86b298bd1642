"""Float64 model of StaticVolume.filter_stack (vt_volume_filter_stack, kernel 23) and the bound its results are held to.

The definition (include/voltools_hip.h), for a line of extent L, K taps t, r = (K - 1) / 2:
    acc = 0;  for j ascending with t[j] != 0:  x = w + r - j;  pad 0: skip j when x is outside [0, L);  pad 1: x = clamp(x, 0, L - 1)
    acc += t[j] * line[x];   out = float32(weight * acc)
summed here in numpy.longdouble, so zero taps and pad-0 taps outside the line contribute nothing, not even a NaN.

The bound is derived, not measured, per pixel:
    |out - model| <= 2^-24 |model| + 2 |w| nnz 2^-53 sum_j |t_j s_j| + 2^-149
the single float32 rounding, the standard bound of a chain of nnz fmas (doubled for the model's own rounding and the product with the
weight), and one float32 subnormal step."""
import numpy as np


def filter_image(img, taps, axis, pad):
    """(sum, sum of magnitudes) as longdouble arrays of img's shape (H, W).  axis: 1 or 2 as in the stack; pad: 0 zero, 1 edge."""
    taps = np.asarray(taps, np.float64)
    assert taps.ndim == 1 and taps.size % 2 == 1 and axis in (1, 2) and pad in (0, 1)
    a = np.moveaxis(np.asarray(img), axis - 1, -1).astype(np.longdouble)
    L, r = a.shape[-1], (taps.size - 1) // 2
    val = np.zeros(a.shape, np.longdouble)
    mag = np.zeros(a.shape, np.longdouble)
    base = np.arange(L)
    for j in np.flatnonzero(taps):
        idx = base + r - int(j)
        ok = (idx >= 0) & (idx < L)
        if pad == 0:
            if not ok.any():
                continue
            term = np.zeros(a.shape, np.longdouble)
            term[..., ok] = np.longdouble(taps[j]) * a[..., idx[ok]]
        else:
            term = np.longdouble(taps[j]) * a[..., np.clip(idx, 0, L - 1)]
        val += term
        mag += np.abs(term)
    return np.moveaxis(val, -1, axis - 1), np.moveaxis(mag, -1, axis - 1)


def model(stack, taps, axis, pad, planes=None, weights=None):
    """(values (n, H, W) float64 = w_i * sum, bounds (n, H, W) float64) of filter_stack(taps, axis, weights, pad, planes=planes).  taps:
    (K,) or (n, K); pad: 'zero' | 'edge' | 0 | 1."""
    stack = np.asarray(stack)
    taps = np.asarray(taps, np.float64)
    pad = {'zero': 0, 'edge': 1}.get(pad, pad)
    planes = np.arange(stack.shape[0]) if planes is None else np.asarray(planes)
    n = len(planes)
    weights = np.ones(n) if weights is None else np.asarray(weights, np.float64)
    vals = np.empty((n,) + stack.shape[1:], np.float64)
    bounds = np.empty_like(vals)
    cache = {}
    for i in range(n):
        t = taps if taps.ndim == 1 else taps[i]
        key = (int(planes[i]), t.tobytes())
        if key not in cache:
            cache[key] = filter_image(stack[planes[i]], t, axis, pad)
        val, mag = cache[key]
        w = np.longdouble(weights[i])
        nnz = int(np.count_nonzero(t))
        with np.errstate(invalid='ignore'):
            vals[i] = (w * val).astype(np.float64)
            bounds[i] = (2.0 ** -24 * np.abs(w * val) + 2.0 * abs(w) * nnz * 2.0 ** -53 * mag + 2.0 ** -149).astype(np.float64)
    return vals, bounds


def check(got, vals, bounds, what=''):
    """Every pixel of every entry within its bound; a pixel the model has as NaN must be NaN."""
    got = np.asarray(got)
    assert got.dtype == np.float32 and got.shape == vals.shape, (what, got.dtype, got.shape, vals.shape)
    bad = np.isnan(vals)
    assert np.array_equal(np.isnan(got), bad), (what, 'NaN pixels differ', int((np.isnan(got) != bad).sum()))
    ok = ~bad
    err = np.abs(got.astype(np.float64)[ok] - vals[ok])
    over = err > bounds[ok]
    worst = float((err / bounds[ok]).max()) if err.size else 0.0
    print(what, f'max|got - model| {float(err.max()) if err.size else 0.0:.3e}  worst error / bound {worst:.3f}')
    assert not over.any(), (what, int(over.sum()), worst)


def phantom(size=32):
    """Two Gaussian blobs of different width and height in a size^3 volume, float32."""
    z, y, x = np.meshgrid(*(np.arange(size, dtype=np.float64),) * 3, indexing='ij')
    c = (size - 1) / 2

    def blob(dz, dy, dx, s, a):
        return a * np.exp(-((z - c - dz) ** 2 + (y - c - dy) ** 2 + (x - c - dx) ** 2) / (2 * s * s))
    return (blob(-4, 3, -5, 2.5, 1.0) + blob(5, -4, 4, 3.5, 0.7)).astype(np.float32)


def correlation(a, b):
    a = np.asarray(a, np.float64).ravel() - np.mean(a, dtype=np.float64)
    b = np.asarray(b, np.float64).ravel() - np.mean(b, dtype=np.float64)
    return float(a @ b / np.sqrt((a @ a) * (b @ b)))


def pipeline_correlations(vt, device, tilt_axis, size=32, n_tilts=41):
    """(unfiltered, ramp-filtered) correlation with the phantom of its back-projection from n_tilts projections over +-60 degrees."""
    vol = phantom(size)
    angles = np.linspace(-60.0, 60.0, n_tilts)
    series = np.array(vt.StaticVolume(vol, device=device).tilt_series(angles, tilt_axis=tilt_axis))
    sv = vt.StaticVolume(series, device=device, stack=True)
    plain = np.array(sv.backproject_tilts(angles, tilt_axis, output_shape=vol.shape))
    filtered = np.array(sv.ramp_filter(tilt_axis))
    rec = np.array(vt.StaticVolume(filtered, device=device, stack=True).backproject_tilts(angles, tilt_axis, output_shape=vol.shape))
    return correlation(plain, vol), correlation(rec, vol)
