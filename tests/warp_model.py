"""A float64 numpy model of StaticVolume.warp (vt_volume_warp, kernel 20), written from the definition in include/voltools_hip.h and
the header of vt_kernels_warp.hip and sharing nothing with the library:

  * s(v) = a(v) + u(v):  a by the fma chain fma(m0, d, fma(m1, h, fma(m2, w, t))), u by r_k = (g_k - 1) / (o_k - 1), q_k = v_k r_k,
    c_k = min(floor(q_k), g_k - 2), f_k = q_k - c_k and lerps fma(f, b - a, a) along axis 2, then 1, then 0 on the float32 grid widened to
    float64 (fma emulated as box_index_model does: the longdouble product-sum rounded to float64 -- exact for the chain's integer
    factors; for the lerps' 53-bit factors it can differ from a true fma by a double rounding, one ulp of u at most);
  * floor / fraction, eight (trilinear) or sixty-four (cubic B-spline) taps of the volume with a border of zeros;
  * the skirt rule -0.5 <= s_r < dim_r - 0.5 on those coordinates;
  * for filt_* the coefficients of prefilter_model.prefilter_f64;
  * the planning rule: per output tile the node sub-block, its per-component range, the staged dims (extract_box_dims' formula with the
    extent grown by umax - umin), the origin, and whether the tile stages (box <= BOX_CAP, hull bound granted) or gathers;
  * which voxels the kernel samples (kernel_inside: 'zero' tiles none, `whole` tiles all, the others by the skirt rule), with the
    switches of three wrong kernels that tests/test_warp_lattice_host.py argues with.

The interpolation arithmetic is float64 throughout; what the library does in float32 is covered by the tolerances of the tests."""
import numpy as np

import box_index_model as bim
import prefilter_model as pm

_LD = np.longdouble
CUBIC = bim.CUBIC
FILTERED = ('filt_bspline', 'filt_bspline_simple')
BOX_CAP = 96 * 1024                 # kWarpBoxCap
HULL_LIMIT = 1048576.0              # kWarpHullLimit
SCRATCH_FLOATS = 32                 # kWarpScratchFloats
BOX_MARGIN = bim.BOX_MARGIN
TILE_MARGIN = bim.TILE_MARGIN


def _fma(a, x, c):
    return (np.asarray(a, _LD) * np.asarray(x, _LD) + np.asarray(c, _LD)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------
# coordinates
# ---------------------------------------------------------------------------------------------------
def ratio(g, o):
    return (g - 1) / (o - 1) if g > 1 else 0.0


def split(o, g):
    """(cell, fraction) of every output index 0..o-1 on an axis with g nodes."""
    x = np.arange(o, dtype=np.float64)
    if g == 1:
        return np.zeros(o, np.int64), np.zeros(o, np.float64)
    q = x * ratio(g, o)
    c = np.minimum(np.floor(q).astype(np.int64), g - 2)
    return c, q - c.astype(np.float64)


def displacement(grid, shape):
    """u(v), float64 (oD, oH, oW, 3)."""
    u = np.asarray(grid, np.float32).astype(np.float64)
    assert u.ndim == 4 and u.shape[3] == 3
    for axis in (2, 1, 0):
        g, o = u.shape[axis], shape[axis]
        c, f = split(o, g)
        up = c + 1 if g > 1 else c
        a, b = np.take(u, c, axis=axis), np.take(u, up, axis=axis)
        f = f.reshape([-1 if k == axis else 1 for k in range(4)])
        u = _fma(f, b - a, a)
    return u


def affine_coords(m, shape):
    m = np.asarray(m, np.float64)
    d = np.arange(shape[0]).reshape(-1, 1, 1)
    h = np.arange(shape[1]).reshape(1, -1, 1)
    w = np.arange(shape[2]).reshape(1, 1, -1)
    return np.stack([np.broadcast_to(_fma(m[r, 0], d, _fma(m[r, 1], h, _fma(m[r, 2], w, m[r, 3]))), shape) for r in range(3)])


def coords(m, grid, shape):
    """s(v), float64 (3, oD, oH, oW); m None = identity."""
    m = np.eye(4) if m is None else m
    return affine_coords(m, shape) + np.moveaxis(displacement(grid, shape), 3, 0)


def inside(s, src_shape):
    ins = np.ones(s.shape[1:], bool)
    for r in range(3):
        ins &= (s[r] >= -0.5) & (s[r] < src_shape[r] - 0.5)
    return ins


def skirt_distance(s, src_shape):
    """Per voxel the distance of the nearest coordinate to a skirt face."""
    dist = np.full(s.shape[1:], np.inf)
    for r in range(3):
        dist = np.minimum(dist, np.minimum(np.abs(s[r] + 0.5), np.abs(s[r] - (src_shape[r] - 0.5))))
    return dist


# ---------------------------------------------------------------------------------------------------
# sampling
# ---------------------------------------------------------------------------------------------------
def _weights(f):
    g = 1.0 - f
    return [g * g * g / 6.0, 2.0 / 3.0 - 0.5 * f * f * (2.0 - f), 2.0 / 3.0 - 0.5 * g * g * (2.0 - g), f * f * f / 6.0]


def _tap(vol, iz, iy, ix):
    D, H, W = vol.shape
    ok = (iz >= 0) & (iz < D) & (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    return np.where(ok, vol[np.clip(iz, 0, D - 1), np.clip(iy, 0, H - 1), np.clip(ix, 0, W - 1)], 0.0)


def sample(vol, s, interp):
    """The 3-D interpolation of float64 volume `vol` at coordinates s (3, ...), zero border, no skirt rule."""
    fl = np.floor(s)
    f = s - fl
    i = fl.astype(np.int64)
    if interp == 'linear':
        val = np.zeros(s.shape[1:], np.float64)
        for a in (0, 1):
            for b in (0, 1):
                for c in (0, 1):
                    wgt = (f[0] if a else 1.0 - f[0]) * (f[1] if b else 1.0 - f[1]) * (f[2] if c else 1.0 - f[2])
                    val += wgt * _tap(vol, i[0] + a, i[1] + b, i[2] + c)
        return val
    wz, wy, wx = _weights(f[0]), _weights(f[1]), _weights(f[2])
    # the 64 taps of _tap, fetched from a copy of the volume inside a shell of zeros: an index that leaves the volume is clipped onto
    # the shell (the same values as _tap's select, with one index computation per axis and offset instead of one per tap)
    D, H, W = vol.shape
    shell = np.zeros((D + 2, H + 2, W + 2), np.float64)
    shell[1:-1, 1:-1, 1:-1] = vol
    flat = shell.reshape(-1)
    iz = [np.clip(i[0] + a, 0, D + 1) * ((H + 2) * (W + 2)) for a in range(4)]          # (i - 1 + a) + 1: the shell's offset
    iy = [np.clip(i[1] + b, 0, H + 1) * (W + 2) for b in range(4)]
    ix = [np.clip(i[2] + c, 0, W + 1) for c in range(4)]
    val = np.zeros(s.shape[1:], np.float64)
    for a in range(4):
        for b in range(4):
            row = np.zeros(s.shape[1:], np.float64)
            zy = iz[a] + iy[b]
            for c in range(4):
                row += wx[c] * flat[zy + ix[c]]
            val += (wz[a] * wy[b]) * row
    return val


def source(vol, interp):
    v = np.asarray(vol, np.float32).astype(np.float64)
    return pm.prefilter_f64(v) if interp in FILTERED else v


def taps_inside(s, src_shape, interp):
    """Voxels whose taps all lie inside the volume."""
    lo, hi = (1, 2) if interp in CUBIC else (0, 1)
    fl = np.floor(s)
    ok = np.ones(s.shape[1:], bool)
    for r in range(3):
        ok &= (fl[r] - lo >= 0) & (fl[r] + hi <= src_shape[r] - 1)
    return ok


def warp(vol, m, grid, shape, interp):
    """(values float64, inside mask, coordinates)."""
    s = coords(m, grid, shape)
    ins = inside(s, vol.shape)
    return np.where(ins, sample(source(vol, interp), s, interp), 0.0), ins, s


# ---------------------------------------------------------------------------------------------------
# the planning rule
# ---------------------------------------------------------------------------------------------------
def cells(first, last, r, g):
    if g == 1:
        return 0, 1
    a, b = int(np.floor(float(first) * r)), int(np.floor(float(last) * r))
    c_lo, c_hi = min(a, g - 2), min(b, g - 2)
    return c_lo, c_hi - c_lo + 2


def tile_box(ext_affine, umin, umax, halo2, gm1_max):
    """Staged dims of a tile, or None when it gathers from global memory."""
    U = float(max(np.abs(umin).max(), np.abs(umax).max()))
    if not U * gm1_max <= HULL_LIMIT:
        return None
    L = []
    for r in range(3):
        ext = ext_affine[r] + (float(umax[r]) - float(umin[r]))
        if not ext < 4096.0:
            return None
        L.append(int(np.floor(ext + 2.0 * BOX_MARGIN)) + 3 + halo2)
    L[2] = (L[2] + 3 + 3) & ~3
    return tuple(L) if L[0] * L[1] * L[2] * 4 <= BOX_CAP else None


class Plan:
    pass


def plan(m, grid, out_shape, interp, force_direct=False, origin_without_umin=False):
    """The launch plan: .cfg, .tile, .nT, .staged (bool per tile), .dims / .origin (int per tile x 3; zeros where not staged), .cells /
    .nodes (first cell / node count per tile x 3), .lds_dims (the launch's last_lds_dims), .node_floats, .lds_bytes.
    `origin_without_umin` is a MUTATION (tests/test_warp_lattice_host.py): the origin a wrong kernel would take from base + neg alone."""
    m = np.eye(4) if m is None else np.asarray(m, np.float64)
    grid = np.asarray(grid, np.float32)
    g = grid.shape[:3]
    cubic = interp in CUBIC
    halo = 1 if cubic else 0
    p = Plan()
    p.cfg = bim.extract_pick_tile(cubic, out_shape)[0]
    T = p.tile = bim.TILES[p.cfg]
    nT = p.nT = tuple((out_shape[k] + T[k] - 1) // T[k] for k in range(3))
    r = [ratio(g[k], out_shape[k]) for k in range(3)]
    neg, pos, ext = [], [], []
    for row in range(3):
        n = q = e = 0.0
        for k in range(3):
            x = float(m[row][k]) * (T[k] - 1)
            if x < 0:
                n += x
            else:
                q += x
            e += abs(float(m[row][k])) * (T[k] - 1)
        neg.append(n)
        pos.append(q)
        ext.append(e)
    p.neg, p.pos = neg, pos
    tiled = (not force_direct) and all(e < 4096.0 for e in ext)
    gm1_max = p.gm1_max = max(g) - 1
    p.staged = np.zeros(nT, bool)
    p.dims = np.zeros(nT + (3,), np.int64)
    p.origin = np.zeros(nT + (3,), np.int64)
    p.cells = np.zeros(nT + (3,), np.int64)
    p.nodes = np.zeros(nT + (3,), np.int64)
    p.umin = np.zeros(nT + (3,), np.float32)
    p.umax = np.zeros(nT + (3,), np.float32)
    nodes_max, best = 0, 0
    p.lds_dims = (0, 0, 0)
    for a in range(nT[0]):
        for b in range(nT[1]):
            for c in range(nT[2]):
                t0 = (a * T[0], b * T[1], c * T[2])
                cl, nn = zip(*[cells(t0[k], min(t0[k] + T[k], out_shape[k]) - 1, r[k], g[k]) for k in range(3)])
                p.cells[a, b, c], p.nodes[a, b, c] = cl, nn
                nodes_max = max(nodes_max, nn[0] * nn[1] * nn[2])
                sub = grid[cl[0]:cl[0] + nn[0], cl[1]:cl[1] + nn[1], cl[2]:cl[2] + nn[2]].reshape(-1, 3)
                umin, umax = sub.min(axis=0), sub.max(axis=0)
                p.umin[a, b, c], p.umax[a, b, c] = umin, umax
                L = tile_box(ext, umin, umax, 2 * halo, gm1_max) if tiled else None
                if L is None:
                    continue
                p.staged[a, b, c] = True
                p.dims[a, b, c] = L
                o = []
                for row in range(3):
                    base = float(_fma(m[row, 0], t0[0], _fma(m[row, 1], t0[1], _fma(m[row, 2], t0[2], m[row, 3]))))
                    lo = base + neg[row] + (0.0 if origin_without_umin else float(umin[row]))
                    o.append(int(np.floor(lo - BOX_MARGIN)) - halo)
                o[2] &= ~3
                p.origin[a, b, c] = o
                if L[0] * L[1] * L[2] * 4 > best:
                    best, p.lds_dims = L[0] * L[1] * L[2] * 4, L
    p.node_floats = (3 * nodes_max + 3) & ~3
    p.lds_bytes = (SCRATCH_FLOATS + p.node_floats) * 4 + best
    return p


def tile_outcome(p, m, src_shape):
    """Per tile: 'zero' (classified wholly outside), 'stage' or 'direct' -- what the kernel does with it for a source of src_shape."""
    m = np.eye(4) if m is None else np.asarray(m, np.float64)
    T = p.tile
    out = np.empty(p.nT, dtype=object)
    for idx in np.ndindex(*p.nT):
        t0 = [idx[k] * T[k] for k in range(3)]
        U = float(max(np.abs(p.umin[idx]).max(), np.abs(p.umax[idx]).max()))
        hull = U * p.gm1_max <= HULL_LIMIT
        any_valid = True
        for row in range(3):
            base = float(_fma(m[row, 0], t0[0], _fma(m[row, 1], t0[1], _fma(m[row, 2], t0[2], m[row, 3]))))
            lo = base + p.neg[row] + float(p.umin[idx][row])
            hi = base + p.pos[row] + float(p.umax[idx][row])
            any_valid = any_valid and hi >= -0.5 - TILE_MARGIN and lo < src_shape[row] - 0.5 + TILE_MARGIN
        out[idx] = 'zero' if (hull and not any_valid) else ('stage' if p.staged[idx] else 'direct')
    return out


def whole_tiles(p, m, src_shape, margin=TILE_MARGIN):
    """Per tile: staged AND [base + neg + umin, base + pos + umax] inside the valid interval by `margin` on every axis -- the tiles whose
    voxels skip the per-voxel inside test.  margin=0.0 is a MUTATION: `whole` by a bare comparison."""
    m = np.eye(4) if m is None else np.asarray(m, np.float64)
    T = p.tile
    out = np.zeros(p.nT, bool)
    for idx in np.ndindex(*p.nT):
        if not p.staged[idx]:
            continue
        t0 = [idx[k] * T[k] for k in range(3)]
        ok = True
        for row in range(3):
            base = float(_fma(m[row, 0], t0[0], _fma(m[row, 1], t0[1], _fma(m[row, 2], t0[2], m[row, 3]))))
            lo = base + p.neg[row] + float(p.umin[idx][row])
            hi = base + p.pos[row] + float(p.umax[idx][row])
            ok = ok and lo >= -0.5 + margin and hi < src_shape[row] - 0.5 - margin
        out[idx] = ok
    return out


def kernel_inside(p, m, s, src_shape, out_shape, margin=TILE_MARGIN, s_test=None):
    """The mask of voxels the kernel SAMPLES under plan p: none in a 'zero' tile, all in a whole tile, elsewhere the skirt rule on
    `s_test` (default s, the definition).  With the defaults it must equal inside(s, src_shape) -- that is what kTileMargin and the hull
    bound are for; `margin` and `s_test` are the switches of two wrong kernels."""
    T = p.tile
    mask = inside(s if s_test is None else s_test, src_shape).copy()
    what = tile_outcome(p, m, src_shape)
    whole = whole_tiles(p, m, src_shape, margin)
    for idx in np.ndindex(*p.nT):
        sl = tuple(slice(idx[k] * T[k], min((idx[k] + 1) * T[k], out_shape[k])) for k in range(3))
        if what[idx] == 'zero':
            mask[sl] = False
        elif whole[idx]:
            mask[sl] = True
    return mask


def violations(p, s, out_shape, interp):
    """Staging safety: [(tile, axis, lowest tap, highest tap, L)] over the staged tiles -- every tap index of every voxel of the tile
    that lies in the output (the kernel gathers before it masks) must lie in [0, L) of the tile's box; on axis 2 the cubic gather's
    aligned pairs count as read."""
    cubic = interp in CUBIC
    T = p.tile
    bad = []
    fl = np.floor(s).astype(np.int64)
    for idx in np.ndindex(*p.nT):
        if not p.staged[idx]:
            continue
        sl = tuple(slice(idx[k] * T[k], min((idx[k] + 1) * T[k], out_shape[k])) for k in range(3))
        for r in range(3):
            i = fl[r][sl] - int(p.origin[idx][r])
            if cubic and r == 2:
                x1 = i - 1
                par = x1 & 1
                lo, hi = int((x1 - par).min()), int((x1 - par + np.where(par == 1, 5, 3)).max())
            elif cubic:
                lo, hi = int(i.min()) - 1, int(i.max()) + 2
            else:
                lo, hi = int(i.min()), int(i.max()) + 1
            if lo < 0 or hi >= int(p.dims[idx][r]):
                bad.append((idx, r, lo, hi, int(p.dims[idx][r])))
    return bad
