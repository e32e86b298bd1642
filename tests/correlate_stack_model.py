"""Model of StaticVolume.correlate_stack (vt_volume_correlate_stack, kernel 24), from the text of include/voltools_hip.h alone, the
bound its scores are held to, and the kernel's launch plan restated.

The definition: patch (a, b) of the grid (gH, gW) covers rows [a H // gH, (a + 1) H // gH) and columns [b W // gW, (b + 1) W // gW);
    out[i, a, b, u, v] = sum over (y, x) in the patch of  r_i[y, x] * s(y + u - Rh, x + v - Rw),   s = the image inside, +0 outside
with the zero MULTIPLIED: a non-finite reference pixel poisons its patch at every shift.  Summed here in numpy.longdouble (the
products of two float32 are exact in it), so the model's own rounding is far below the bound.

The bound is derived, not measured, per score: (N + 2) 2^-53 sum |r s| with N the pixels of the patch -- the standard bound of N
rounded additions of exact products in any order (N 2^-53 / (1 - N 2^-53) sum |r s|, N <= 2^26 here), with room for the model's own
rounding and its conversion to float64.  On small-integer data every partial sum is an integer below 2^53 and the bound is not
needed: the scores are exact."""
import numpy as np

PIECE, BAND, GROUP, MAX_RUNS = 64, 16, 8, 7


def patch_edges(extent, g):
    assert 1 <= g <= extent
    return [a * extent // g for a in range(g + 1)]


def correlate_image(img, ref, max_shift, patch_grid):
    """(scores, sum of magnitudes) as longdouble arrays (gH, gW, 2 Rh + 1, 2 Rw + 1) of one image (H, W) against one reference."""
    img = np.asarray(img, np.float32).astype(np.longdouble)
    ref = np.asarray(ref, np.float32).astype(np.longdouble)
    H, W = img.shape
    assert ref.shape == (H, W)
    (rh, rw), (gh, gw) = max_shift, patch_grid
    assert 0 <= rh <= H - 1 and 0 <= rw <= W - 1
    ye, xe = patch_edges(H, gh), patch_edges(W, gw)
    padded = np.zeros((H + 2 * rh, W + 2 * rw), np.longdouble)
    padded[rh:rh + H, rw:rw + W] = img
    val = np.empty((gh, gw, 2 * rh + 1, 2 * rw + 1), np.longdouble)
    mag = np.empty_like(val)
    with np.errstate(invalid='ignore', over='ignore'):
        for u in range(2 * rh + 1):
            for v in range(2 * rw + 1):
                prod = ref * padded[u:u + H, v:v + W]
                val[:, :, u, v] = np.add.reduceat(np.add.reduceat(prod, ye[:-1], axis=0), xe[:-1], axis=1)
                mag[:, :, u, v] = np.add.reduceat(np.add.reduceat(np.abs(prod), ye[:-1], axis=0), xe[:-1], axis=1)
    return val, mag


def model(stack, references, max_shift, patch_grid, planes=None, reference_planes=None):
    """(values, bounds), float64 (n, gH, gW, 2 Rh + 1, 2 Rw + 1), of correlate_stack(references, max_shift, patch_grid, planes=planes,
    reference_planes=reference_planes).  references: (H, W), (n, H, W) or None with reference_planes."""
    stack = np.asarray(stack)
    T, H, W = stack.shape
    refs = None if references is None else np.asarray(references, np.float32)
    assert (refs is None) != (reference_planes is None)
    if planes is not None:
        n = len(planes)
    elif reference_planes is not None:
        n = len(reference_planes)
    elif refs.ndim == 3:
        n = refs.shape[0]
    else:
        n = T
    planes = np.arange(n) if planes is None else np.asarray(planes)
    (rh, rw), (gh, gw) = max_shift, patch_grid
    ye, xe = patch_edges(H, gh), patch_edges(W, gw)
    pixels = np.outer(np.diff(ye), np.diff(xe)).astype(np.float64)              # N per patch
    vals = np.empty((n, gh, gw, 2 * rh + 1, 2 * rw + 1), np.float64)
    bounds = np.empty_like(vals)
    cache = {}
    for i in range(n):
        if refs is None:
            ref, rkey = stack[reference_planes[i]], ('plane', int(reference_planes[i]))
        elif refs.ndim == 2:
            ref, rkey = refs, ('shared',)
        else:
            ref, rkey = refs[i], ('own', refs[i].tobytes())
        key = (int(planes[i]), rkey)
        if key not in cache:
            cache[key] = correlate_image(stack[planes[i]], ref, max_shift, patch_grid)
        val, mag = cache[key]
        with np.errstate(invalid='ignore', over='ignore'):
            vals[i] = val.astype(np.float64)
            bounds[i] = ((pixels[:, :, None, None] + 2.0) * 2.0 ** -53 * mag).astype(np.float64)
    return vals, bounds


def naive(img, ref, max_shift, patch_grid):
    """The definition as loops over plain Python floats (tiny cases only)."""
    H, W = img.shape
    (rh, rw), (gh, gw) = max_shift, patch_grid
    out = np.zeros((gh, gw, 2 * rh + 1, 2 * rw + 1), np.float64)
    for a in range(gh):
        for b in range(gw):
            for u in range(2 * rh + 1):
                for v in range(2 * rw + 1):
                    acc = 0.0
                    for y in range(a * H // gh, (a + 1) * H // gh):
                        for x in range(b * W // gw, (b + 1) * W // gw):
                            yy, xx = y + u - rh, x + v - rw
                            s = float(img[yy, xx]) if 0 <= yy < H and 0 <= xx < W else 0.0
                            acc += float(ref[y, x]) * s
                    out[a, b, u, v] = acc
    return out


def check(got, vals, bounds, tag=''):
    """Every score within its bound; a score the model has as non-finite must hold the same non-finite value (NaN, or the infinity of
    the same sign)."""
    got = np.asarray(got)
    assert got.dtype == np.float64 and got.shape == vals.shape, (tag, got.dtype, got.shape, vals.shape)
    odd = ~np.isfinite(vals)
    assert np.array_equal(np.isnan(got), np.isnan(vals)), (tag, 'NaN scores differ', int((np.isnan(got) != np.isnan(vals)).sum()))
    assert np.array_equal(got[odd & ~np.isnan(vals)], vals[odd & ~np.isnan(vals)]), (tag, 'infinite scores differ')
    ok = ~odd
    err = np.abs(got[ok] - vals[ok])
    over = err > bounds[ok]
    with np.errstate(invalid='ignore', divide='ignore'):
        ratio = np.where(bounds[ok] > 0, err / bounds[ok], np.where(err > 0, np.inf, 0.0))
    worst = float(ratio.max()) if err.size else 0.0
    print(tag, f'max|got - model| {float(err.max()) if err.size else 0.0:.3e}  worst error / bound {worst:.3f}')
    assert not over.any(), (tag, int(over.sum()), worst)


def plan(H, W, max_shift, patch_grid, n=1):
    """The kernel's launch plan restated (vt_kernels_correlatestack.hip; the header's words): pieces, shift blocks, the staged block,
    LDS bytes, and the workgroups of a call of n entries that fits one launch."""
    (rh, rw), (gh, gw) = max_shift, patch_grid
    nu, nv = 2 * rh + 1, 2 * rw + 1
    pieces_y = -(-(-(-H // gh)) // PIECE)                     # of the largest patch, ceil(H / gH) rows
    pieces_x = -(-(-(-W // gw)) // PIECE)
    pad9, pad11 = -(-nv // 9) * 9, -(-nv // 11) * 11
    cv = 11 if pad11 < pad9 else 9
    runs = min(MAX_RUNS, -(-nv // cv))
    rows_blk = min(64 // runs, nu)
    blocks_u, blocks_v = -(-nu // rows_blk), -(-nv // (runs * cv))
    lds_rows, pitch = PIECE + rows_blk - 1, PIECE + runs * cv
    pieces = pieces_y * pieces_x
    unit_wgs = pieces * blocks_u * blocks_v
    return dict(pieces_y=pieces_y, pieces_x=pieces_x, pieces=pieces, cv=cv, runs=runs, rows_blk=rows_blk, blocks_u=blocks_u,
                blocks_v=blocks_v, tile=(1, PIECE, PIECE), lds_dims=(1, lds_rows, pitch), lds_bytes=PIECE * PIECE * 4 + lds_rows * pitch * 4,
                unit_wgs=unit_wgs, unit_part_bytes=pieces * nu * nv * 8 if pieces > 1 else 0, grid=n * gh * gw * unit_wgs)


def launches(H, W, max_shift, patch_grid, n, cap=64 << 20):
    """Units (entry, patch) per launch of a call, as the entry point splits it: (units per launch, units of the last launch)."""
    p = plan(H, W, max_shift, patch_grid)
    units = n * patch_grid[0] * patch_grid[1]
    per = min(units, (2 ** 31 - 1) // p['unit_wgs'])
    if p['unit_part_bytes']:
        per = min(per, max(1, cap // p['unit_part_bytes']))
    return per, units - (units - 1) // per * per


def block_edges_v(limit):
    """Every Rw < limit at which Rw and Rw + 1 give a different number of column blocks (the count is not monotonic: the run length
    switches between 9 and 11 with the window): both sides of each are windows to test."""
    out = []
    for rw in range(limit):
        if plan(1, limit + 2, (0, rw), (1, 1))['blocks_v'] != plan(1, limit + 2, (0, rw + 1), (1, 1))['blocks_v']:
            out.append(rw)
    return out


def block_edges_u(limit_h, limit_w):
    """For every number of runs per row, one (Rh, Rw) with 2 Rh + 1 shift rows filling one block exactly and Rh + 1 needing two."""
    out, seen = [], set()
    for rw in range(limit_w):
        runs = plan(limit_h + 1, limit_w + 1, (0, rw), (1, 1))['runs']
        if runs in seen:
            continue
        seen.add(runs)
        for rh in range(limit_h - 1):
            a = plan(limit_h + 1, limit_w + 1, (rh, rw), (1, 1))
            b = plan(limit_h + 1, limit_w + 1, (rh + 1, rw), (1, 1))
            if a['blocks_u'] == 1 and b['blocks_u'] == 2:
                out.append((rh, rw))
                break
    return out


def max_lds_bytes():
    """The roof over every window: the header states 56992."""
    return max(plan(2 ** 12, 2 ** 12, (rh, rw), (1, 1))['lds_bytes'] for rh in range(0, 70) for rw in range(0, 200))
