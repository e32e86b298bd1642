"""Model of StaticVolume.moments_stack (vt_volume_moments_stack, kernel 25), from the text of include/voltools_hip.h alone, the bound
its sums are held to, the kernel's launch plan restated, and the correlation coefficient in longdouble.

The definition: patch (a, b) of the grid (gH, gW) covers rows [a H // gH, (a + 1) H // gH) and columns [b W // gW, (b + 1) W // gW);
    out[i, a, b, u, v, 0] = sum over (y, x) in the patch of  s(y + u - Rh, x + v - Rw),      s = the image inside, +0 outside
    out[i, a, b, u, v, 1] = the same sum of                  s(..)^2
Summed here in numpy.longdouble (a float32 and its square are exact in it), so the model's own rounding is far below the bound.

The bound is derived, not measured, per value: (N + 2) 2^-53 sum |s|, respectively (N + 2) 2^-53 sum s^2, with N the pixels of the
patch -- the standard bound of N rounded additions of exact terms in any order (N 2^-53 / (1 - N 2^-53) sum |term|, N <= 2^26 here),
with room for the model's own rounding and its conversion to float64; tests/correlate_stack_model.py derives the same for products.  The
header's order (row sums over the patch's columns, then over its rows) is one such order.  On small-integer data every partial sum is
an integer below 2^53 and the bound is not needed: the sums are exact."""
import numpy as np

from correlate_stack_model import check, patch_edges      # the comparison against (values, bounds) and the patch edges, shared

CHUNK, GROUP, MAX_RUNS, WAVES = 32, 8, 7, 4


def moments_image(img, max_shift, patch_grid):
    """(values, magnitudes) as longdouble arrays (gH, gW, 2 Rh + 1, 2 Rw + 1, 2) of one image (H, W): the sums of s and s^2, and the
    sums of |s| and s^2."""
    img = np.asarray(img, np.float32).astype(np.longdouble)
    H, W = img.shape
    (rh, rw), (gh, gw) = max_shift, patch_grid
    assert 0 <= rh <= H - 1 and 0 <= rw <= W - 1
    ye, xe = patch_edges(H, gh)[:-1], patch_edges(W, gw)[:-1]
    padded = np.zeros((H + 2 * rh, W + 2 * rw), np.longdouble)
    padded[rh:rh + H, rw:rw + W] = img
    val = np.empty((gh, gw, 2 * rh + 1, 2 * rw + 1, 2), np.longdouble)
    mag = np.empty_like(val)
    with np.errstate(invalid='ignore', over='ignore'):
        fields = (padded, padded * padded, np.abs(padded))
        for v in range(2 * rw + 1):
            # the patch columns of every padded row under column shift v, then the patch rows under every row shift
            cols = [np.add.reduceat(f[:, v:v + W], xe, axis=1) for f in fields]
            for u in range(2 * rh + 1):
                s1, s2, sa = (np.add.reduceat(c[u:u + H], ye, axis=0) for c in cols)
                val[:, :, u, v, 0], val[:, :, u, v, 1] = s1, s2
                mag[:, :, u, v, 0], mag[:, :, u, v, 1] = sa, s2
    return val, mag


def model(stack, max_shift, patch_grid, planes=None):
    """(values, bounds), float64 (n, gH, gW, 2 Rh + 1, 2 Rw + 1, 2), of moments_stack(max_shift, patch_grid, planes=planes)."""
    stack = np.asarray(stack)
    T, H, W = stack.shape
    planes = np.arange(T) if planes is None else np.asarray(planes)
    n = len(planes)
    (rh, rw), (gh, gw) = max_shift, patch_grid
    pixels = np.outer(np.diff(patch_edges(H, gh)), np.diff(patch_edges(W, gw))).astype(np.float64)          # N per patch
    vals = np.empty((n, gh, gw, 2 * rh + 1, 2 * rw + 1, 2), np.float64)
    bounds = np.empty_like(vals)
    cache = {}
    for i in range(n):
        p = int(planes[i])
        if p not in cache:
            cache[p] = moments_image(stack[p], max_shift, patch_grid)
        val, mag = cache[p]
        with np.errstate(invalid='ignore', over='ignore'):
            vals[i] = val.astype(np.float64)
            bounds[i] = ((pixels[:, :, None, None, None] + 2.0) * 2.0 ** -53 * mag).astype(np.float64)
    return vals, bounds


def naive(img, max_shift, patch_grid):
    """The definition as loops over plain Python floats (tiny cases only)."""
    H, W = img.shape
    (rh, rw), (gh, gw) = max_shift, patch_grid
    out = np.zeros((gh, gw, 2 * rh + 1, 2 * rw + 1, 2), np.float64)
    for a in range(gh):
        for b in range(gw):
            for u in range(2 * rh + 1):
                for v in range(2 * rw + 1):
                    s1 = s2 = 0.0
                    for y in range(a * H // gh, (a + 1) * H // gh):
                        for x in range(b * W // gw, (b + 1) * W // gw):
                            yy, xx = y + u - rh, x + v - rw
                            s = float(img[yy, xx]) if 0 <= yy < H and 0 <= xx < W else 0.0
                            s1 += s
                            s2 += s * s
                    out[a, b, u, v] = s1, s2
    return out


def covered(H, W, max_shift, patch_grid, y, x):
    """bool (gH, gW, 2 Rh + 1, 2 Rw + 1): the (patch, shift) pairs whose window covers image pixel (y, x)."""
    (rh, rw), (gh, gw) = max_shift, patch_grid
    ye, xe = patch_edges(H, gh), patch_edges(W, gw)
    out = np.zeros((gh, gw, 2 * rh + 1, 2 * rw + 1), bool)
    for a in range(gh):
        for b in range(gw):
            for u in range(2 * rh + 1):
                for v in range(2 * rw + 1):
                    out[a, b, u, v] = ye[a] <= y - (u - rh) < ye[a + 1] and xe[b] <= x - (v - rw) < xe[b + 1]
    return out


# ---- the launch plan ------------------------------------------------------------------------------------------------------------------
def plan(H, W, max_shift, patch_grid, n=1):
    """The kernel's launch plan restated (the header's words): the run of column shifts a lane owns, runs per row, image rows per
    workgroup, row blocks, shift blocks, the staged block, LDS bytes, and the workgroups of a call of n entries that fits one launch."""
    (rh, rw), (gh, gw) = max_shift, patch_grid
    nu, nv = 2 * rh + 1, 2 * rw + 1
    pad9, pad11 = -(-nv // 9) * 9, -(-nv // 11) * 11
    cv = 11 if pad11 < pad9 else 9
    runs = min(MAX_RUNS, -(-nv // cv))
    rows_wg = WAVES * (64 // runs)
    row_blocks, blocks_v = -(-H // rows_wg), -(-nv // (runs * cv))
    pitch = CHUNK + runs * cv
    unit_wgs = row_blocks * gw * blocks_v
    return dict(cv=cv, runs=runs, rows_wg=rows_wg, row_blocks=row_blocks, blocks_v=blocks_v, tile=(1, rows_wg, CHUNK),
                lds_dims=(1, rows_wg, pitch), lds_bytes=rows_wg * pitch * 4, unit_wgs=unit_wgs, unit_part_bytes=H * gw * nv * 2 * 8,
                grid=n * unit_wgs)


def launches(H, W, max_shift, patch_grid, n, cap=64 << 20):
    """Entries per launch of a call, as the entry point splits it: (entries per run, entries of the last run)."""
    p = plan(H, W, max_shift, patch_grid)
    per = min(n, (2 ** 31 - 1) // p['unit_wgs'], max(1, cap // p['unit_part_bytes']))
    return per, n - (n - 1) // per * per


def plan_edges(H, W, limit):
    """Every Rw < limit at which Rw and Rw + 1 differ in the count of runs, of row blocks or of column-shift blocks (the counts are not
    monotonic: the run length switches between 9 and 11 with the window): both sides of each are windows to test."""
    key = lambda rw: tuple(plan(H, W, (0, rw), (1, 1))[k] for k in ('runs', 'row_blocks', 'blocks_v'))
    return [rw for rw in range(limit) if key(rw) != key(rw + 1)]


def max_lds_bytes():
    """The roof over every window: the header states 44032."""
    return max(plan(2 ** 12, 2 ** 12, (0, rw), (1, 1))['lds_bytes'] for rw in range(0, 200))


# ---- the coefficient --------------------------------------------------------------------------------------------------------------------
def coefficient(scores, moments, reference_moments, pixels):
    """The header-free formula of utils.normalized_scores in longdouble, from longdouble sums: (ncc, kappa), kappa = max(sum r^2 / D_r,
    sum s^2 / D_s) with D the centred sums of squares, the condition number the tolerance 16 N 2^-53 kappa is scaled by.  pixels
    broadcasts against scores."""
    c = np.asarray(scores, np.longdouble)
    m = np.asarray(moments, np.longdouble)
    r = np.asarray(reference_moments, np.longdouble)
    n = np.asarray(pixels, np.longdouble)
    r1, r2 = r[:, :, :, None, None, 0], r[:, :, :, None, None, 1]
    s1, s2 = m[..., 0], m[..., 1]
    d_r, d_s = r2 - r1 * r1 / n, s2 - s1 * s1 / n
    ncc = (c - r1 * s1 / n) / np.sqrt(d_r * d_s)
    return ncc, np.maximum(r2 / d_r, s2 / d_s)
