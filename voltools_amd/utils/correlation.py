"""Patch edges and peak positions for ``StaticVolume.correlate_stack`` / ``find_shifts``."""
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
