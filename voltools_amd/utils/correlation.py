"""Patch edges, peak positions, patch sums and correlation coefficients for ``StaticVolume.correlate_stack`` / ``moments_stack`` /
``find_shifts``."""
import numpy as np


def patch_bounds(extent: int, g: int) -> np.ndarray:
    """The ``g + 1`` edges of the ``g`` patches ``correlate_stack`` cuts an axis of ``extent`` samples into: patch ``a`` covers
    ``[edges[a], edges[a + 1])`` with ``edges[a] = a * extent // g`` (int64, ``1 <= g <= extent``): the patches are disjoint, none is
    empty, and together they cover the axis."""
    for name, val in (('extent', extent), ('g', g)):
        if isinstance(val, bool) or not isinstance(val, (int, np.integer)) or val < 1:
            raise ValueError(f'{name} must be a positive int')
    if g > extent:
        raise ValueError(f'g must lie inside [1, {extent}]')
    return np.arange(int(g) + 1, dtype=np.int64) * int(extent) // int(g)


def peak_shifts(scores, subpixel: bool = True) -> np.ndarray:
    """The position of the largest score of every window: ``scores`` ``(..., 2 Rh + 1, 2 Rw + 1)`` -> float64 ``(..., 2)``, ``(dy, dx)``
    relative to the window centre (the first maximum in C order when several tie).  ``subpixel`` adds, per axis, the vertex of the
    parabola through the peak and its two neighbours along that axis, ``0.5 (c- - c+) / (c- - 2 c0 + c+)``, where the peak is not on
    the window's rim along that axis and the denominator is negative; otherwise it adds 0.  The refinement lies inside (-0.5, 0.5).
    Pure numpy."""
    c = np.asarray(scores, dtype=np.float64)
    if c.ndim < 2 or c.shape[-2] % 2 == 0 or c.shape[-1] % 2 == 0:
        raise ValueError('scores must have shape (..., 2 Rh + 1, 2 Rw + 1)')
    nu, nv = c.shape[-2:]
    lead = c.shape[:-2]
    flat = c.reshape((-1, nu, nv))
    at = flat.reshape((flat.shape[0], -1)).argmax(axis=1) if flat.shape[0] else np.zeros(0, dtype=np.int64)
    iu, iv = at // nv, at % nv
    out = np.empty((flat.shape[0], 2), dtype=np.float64)
    out[:, 0] = iu - (nu - 1) // 2
    out[:, 1] = iv - (nv - 1) // 2
    if subpixel:
        rows = np.arange(flat.shape[0])
        for axis, (idx, size) in enumerate(((iu, nu), (iv, nv))):
            inside = (idx > 0) & (idx < size - 1)
            lo, hi = np.clip(idx - 1, 0, size - 1), np.clip(idx + 1, 0, size - 1)
            if axis == 0:
                cm, c0, cp = flat[rows, lo, iv], flat[rows, iu, iv], flat[rows, hi, iv]
            else:
                cm, c0, cp = flat[rows, iu, lo], flat[rows, iu, iv], flat[rows, iu, hi]
            with np.errstate(all='ignore'):
                den = cm - 2.0 * c0 + cp
                use = inside & (den < 0)
                d = np.where(use, 0.5 * (cm - cp) / np.where(use, den, 1.0), 0.0)
            # c0 is the maximum, so |c- - c+| <= -den and |d| <= 0.5; a tie with a neighbour gives the half-way point, which stays with
            # the peak that argmax chose
            out[:, axis] += np.clip(np.where(np.isfinite(d), d, 0.0), np.nextafter(-0.5, 0.0), np.nextafter(0.5, 0.0))
    return out.reshape(lead + (2,))


def patch_moments(images, patch_grid) -> np.ndarray:
    """The sum and the sum of squares of every patch of every image: ``images`` ``(n, H, W)`` (or ``(H, W)``, taken as ``n = 1``), read
    as float32 like ``correlate_stack``'s references -> float64 ``(n, gH, gW, 2)``, ``[..., 0]`` the sum and ``[..., 1]`` the sum of
    squares over patch ``(a, b)`` of ``patch_grid = (gH, gW)`` (``patch_bounds`` gives its edges), added in float64.  The reference's
    side of ``normalized_scores``.  Pure numpy."""
    imgs = np.asarray(images, dtype=np.float32)
    if imgs.ndim == 2:
        imgs = imgs[None]
    if imgs.ndim != 3 or 0 in imgs.shape:
        raise ValueError('images must have shape (n, H, W) or (H, W)')
    try:
        gh, gw = patch_grid
    except (TypeError, ValueError):
        raise ValueError('patch_grid must be a pair of ints') from None
    ye, xe = patch_bounds(imgs.shape[1], gh)[:-1], patch_bounds(imgs.shape[2], gw)[:-1]
    wide = imgs.astype(np.float64)
    out = np.empty((imgs.shape[0], int(gh), int(gw), 2), dtype=np.float64)
    with np.errstate(invalid='ignore', over='ignore'):
        for k, field in enumerate((wide, wide * wide)):
            out[..., k] = np.add.reduceat(np.add.reduceat(field, ye, axis=1), xe, axis=2)
    return out


def normalized_scores(scores, moments, reference_moments, image_shape=None, pixels=None) -> np.ndarray:
    """Correlation coefficients from raw shift scores.  With ``C = scores`` ``(n, gH, gW, 2 Rh + 1, 2 Rw + 1)`` (``correlate_stack``),
    ``moments`` ``(n, gH, gW, 2 Rh + 1, 2 Rw + 1, 2)`` the sums ``S1, S2`` of the image samples and of their squares under the patch at
    every shift (``moments_stack``), ``reference_moments`` ``(n or 1, gH, gW, 2)`` the sums ``R1, R2`` of the reference and of its squares
    over the patch (``patch_moments``) and ``N`` the pixels of the patch,

        ``ncc = (C - R1 S1 / N) / sqrt((R2 - R1^2 / N) (S2 - S1^2 / N))``,

    float64 of ``scores``' shape.  ``N`` comes from exactly one of ``image_shape = (H, W)``, from which the patch sizes follow through
    ``patch_bounds``, and ``pixels``, the counts themselves (a scalar or anything that broadcasts against ``(gH, gW)``).
    The zero rule: the result is exactly 0 wherever the product under the root is not a positive finite number -- a constant patch of
    the reference, constant samples under the patch, a non-finite sum -- or the numerator is not finite.
    Samples outside the image count as zeros AMONG THE ``N``.  That is ``correlate_stack``'s own convention (its score multiplies them
    by the reference), so a patch on the image border sees a dark frame at the shifts that leave the image and is pulled towards the
    shifts that stay inside.  Pure numpy."""
    c = np.asarray(scores, dtype=np.float64)
    m = np.asarray(moments, dtype=np.float64)
    r = np.asarray(reference_moments, dtype=np.float64)
    if c.ndim != 5 or m.shape != c.shape + (2,):
        raise ValueError('scores must have shape (n, gH, gW, 2 Rh + 1, 2 Rw + 1) and moments that shape with a last axis of 2')
    n, gh, gw = c.shape[:3]
    if r.ndim != 4 or r.shape[0] not in (1, n) or r.shape[1:] != (gh, gw, 2):
        raise ValueError(f'reference_moments must have shape ({n} or 1, {gh}, {gw}, 2)')
    if (image_shape is None) == (pixels is None):
        raise ValueError('exactly one of image_shape and pixels must be given')
    if image_shape is not None:
        H, W = image_shape
        count = np.outer(np.diff(patch_bounds(H, gh)), np.diff(patch_bounds(W, gw))).astype(np.float64)
    else:
        count = np.broadcast_to(np.asarray(pixels, dtype=np.float64), (gh, gw))
        if not (count >= 1).all():
            raise ValueError('pixels must be positive')
    count = count[None, :, :, None, None]
    r1, r2 = r[:, :, :, None, None, 0], r[:, :, :, None, None, 1]
    s1, s2 = m[..., 0], m[..., 1]
    with np.errstate(all='ignore'):
        num = c - r1 * s1 / count
        under = (r2 - r1 * r1 / count) * (s2 - s1 * s1 / count)
        ok = np.isfinite(under) & (under > 0) & np.isfinite(num)
        return np.where(ok, num / np.sqrt(np.where(ok, under, 1.0)), 0.0)
