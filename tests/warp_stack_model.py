"""A float64 numpy model of StaticVolume.warp_stack (vt_volume_warp_stack, kernel 22), written from the definition in
include/voltools_hip.h and sharing nothing with the library:

  * (y, x) of output pixel (h, w) of entry i: the fma chain fma(m1, h, fma(m2, w, t)) on rows 1 and 2 of M_i plus the bilinear
    interpolation of grid G_i -- warp_model.split on the two in-plane axes (r_k = (g_k - 1) / (o_k - 1), q_k = v_k r_k, c_k =
    min(floor(q_k), g_k - 2), f_k = q_k - c_k) and lerps fma(f, b - a, a) along axis 2, then axis 1, on the float32 grid widened to
    float64 (warp_model._fma: the longdouble product-sum rounded to float64);
  * sampling and the skirt rule from backproject_model.sample / inside, the prefilter from backproject_model.images;
  * the planning rule: per (entry, tile) the node block, its per-component range, the patch dims (the affine patch with each extent
    grown by umax - umin), whether the tile stages, and the launch's LDS bytes by the host's sizing rule -- the node block from the tile
    rows and tile columns, the patch allocation from the range of each entry's whole grid, clamped to the cap.

The interpolation arithmetic is float64 throughout; what the library does in float32 is covered by the tolerances of the tests."""
import numpy as np

import backproject_model as bm
import warp_model as wm

CUBIC = bm.CUBIC
PATCH_CAP = 32 * 1024               # kStackAffinePatchCap
CAP_DIMS = (1, 64, 128)             # what last_lds_dims reports when the allocation is the cap itself
HULL_LIMIT = wm.HULL_LIMIT
SCRATCH_BYTES = 4 * wm.SCRATCH_FLOATS
BOX_MARGIN = wm.BOX_MARGIN
TILE_MARGIN = wm.TILE_MARGIN
TILES = ((32, 32), (16, 16))
SKIRT_EPS = 1e-9


# ---------------------------------------------------------------------------------------------------
# coordinates and values
# ---------------------------------------------------------------------------------------------------
def displacement(grid, out):
    """u(h, w), float64 (Ho, Wo, 2)."""
    u = np.asarray(grid, np.float32).astype(np.float64)
    assert u.ndim == 3 and u.shape[2] == 2
    for axis in (1, 0):
        g, o = u.shape[axis], out[axis]
        c, f = wm.split(o, g)
        up = c + 1 if g > 1 else c
        a, b = np.take(u, c, axis=axis), np.take(u, up, axis=axis)
        f = f.reshape([-1 if k == axis else 1 for k in range(3)])
        u = wm._fma(f, b - a, a)
    return u


def affine_coords(m, out):
    m = np.eye(4) if m is None else np.asarray(m, np.float64)
    h = np.arange(out[0]).reshape(-1, 1)
    w = np.arange(out[1]).reshape(1, -1)
    return [np.broadcast_to(wm._fma(m[r, 1], h, wm._fma(m[r, 2], w, m[r, 3])), out) for r in (1, 2)]


def coords(m, grid, out):
    """(y, x), float64 (Ho, Wo) each; m None = identity."""
    ay, ax = affine_coords(m, out)
    u = displacement(grid, out)
    return ay + u[..., 0], ax + u[..., 1]


def grid_of(grids, i):
    grids = np.asarray(grids, np.float32)
    return grids if grids.ndim == 3 else grids[i]


def warp_stack(stack, ms, grids, planes, out, interp):
    """(per-entry float64 B_i (n, Ho, Wo), 0 outside the skirt; inside masks; distance of every pixel to the nearest skirt face)."""
    img = bm.images(stack, interp)
    T, H, W = img.shape
    n = len(ms) if ms is not None else (len(grids) if np.ndim(grids) == 4 else T)
    planes = range(n) if planes is None else planes
    vols, masks, dist = [], [], []
    for i, k in zip(range(n), planes):
        assert 0 <= int(k) < T
        y, x = coords(None if ms is None else ms[i], grid_of(grids, i), out)
        ins = bm.inside(y, x, H, W)
        with np.errstate(invalid='ignore'):
            far = ~(np.isfinite(y) & np.isfinite(x) & (np.abs(y) < 2.0 ** 30) & (np.abs(x) < 2.0 ** 30))
        ys, xs = np.where(far, -10.0, y), np.where(far, -10.0, x)
        vols.append(np.where(ins, bm.sample(img[int(k)], ys, xs, interp), 0.0))
        masks.append(ins)
        dist.append(np.minimum(np.minimum(np.abs(y + 0.5), np.abs(y - (H - 0.5))), np.minimum(np.abs(x + 0.5), np.abs(x - (W - 0.5)))))
    return np.stack(vols), np.stack(masks), np.stack(dist)


def skirt_share(dist):
    """Share of pixels within SKIRT_EPS of a skirt face: there float64 rounding may decide the inside test differently."""
    with np.errstate(invalid='ignore'):
        return float((dist <= SKIRT_EPS).mean())


# ---------------------------------------------------------------------------------------------------
# the planning rule
# ---------------------------------------------------------------------------------------------------
def patch_formula(ext, halo2):
    L = [int(np.floor(e + 2.0 * BOX_MARGIN)) + 3 + halo2 for e in ext]
    return L[0], (L[1] + 3 + 3) & ~3


def pick_tile(cubic, out):
    best, best_cost = 0, np.inf
    for cfg, (th, tw) in enumerate(TILES):
        ext = 0.5 * (th - 1) + 0.5 * (tw - 1)
        Ly, Lx = patch_formula((ext, ext), 2 if cubic else 0)
        cost = float(Ly) * Lx * -(-out[0] // th) * -(-out[1] // tw)
        if cost < best_cost:
            best, best_cost = cfg, cost
    return best


def tile_patch(ext_affine, umin, umax, halo2):
    """(Ly, Lx) of a tile whose nodes span [umin, umax] per component, or None: extent absurd or patch beyond the cap."""
    ext = [ext_affine[k] + (float(umax[k]) - float(umin[k])) for k in range(2)]
    if not all(e < 4096.0 for e in ext):
        return None
    L = patch_formula(ext, halo2)
    return L if L[0] * L[1] * 4 <= PATCH_CAP else None


class Plan:
    pass


def plan(ms, grids, n, out, interp, force_direct=False):
    """.cfg, .tile, .nT; per (entry, tile row, tile column): .staged, .dims (Ly, Lx; zeros where not staged), .origin (staged tiles; for
    a source of any shape), .cells / .nodes (first cell / node count per axis), .umin / .umax, .hull; per entry .flag; the launch's
    .node_floats, .lds_dims, .lds_bytes."""
    grids = np.asarray(grids, np.float32)
    g = grids.shape[-3:-1]
    cubic = interp in CUBIC
    halo = 1 if cubic else 0
    p = Plan()
    p.cfg = pick_tile(cubic, out)
    T = p.tile = TILES[p.cfg]
    nT = p.nT = tuple(-(-out[k] // T[k]) for k in range(2))
    r = [wm.ratio(g[k], out[k]) for k in range(2)]
    p.gm1_max = max(g) - 1
    cells = [[wm.cells(a * T[k], min((a + 1) * T[k], out[k]) - 1, r[k], g[k]) for a in range(nT[k])] for k in range(2)]
    nodes_max = max(c[1] for c in cells[0]) * max(c[1] for c in cells[1])
    assert nodes_max <= (T[0] + 1) * (T[1] + 1)
    p.node_floats = (2 * nodes_max + 3) & ~3
    shp = (n,) + nT
    p.staged = np.zeros(shp, bool)
    p.hull = np.zeros(shp, bool)
    p.dims = np.zeros(shp + (2,), np.int64)
    p.origin = np.zeros(shp + (2,), np.int64)
    p.cells = np.zeros(shp + (2,), np.int64)
    p.nodes = np.zeros(shp + (2,), np.int64)
    p.umin = np.zeros(shp + (2,), np.float32)
    p.umax = np.zeros(shp + (2,), np.float32)
    p.flag = np.zeros(n, bool)
    p.neg = np.zeros((n, 2))
    p.pos = np.zeros((n, 2))
    best, capped = 0, False
    p.lds_dims = (0, 0, 0)
    for i in range(n):
        m = np.eye(4) if ms is None else np.asarray(ms[i], np.float64)
        G = grid_of(grids, i)
        ext = []
        for k, row in enumerate((1, 2)):
            xs = [float(m[row, 1]) * (T[0] - 1), float(m[row, 2]) * (T[1] - 1)]
            p.neg[i, k] = sum(x for x in xs if x < 0)
            p.pos[i, k] = sum(x for x in xs if not x < 0)
            ext.append(abs(float(m[row, 1])) * (T[0] - 1) + abs(float(m[row, 2])) * (T[1] - 1))
        small = all(abs(float(m[row, 1])) * out[0] + abs(float(m[row, 2])) * out[1] + abs(float(m[row, 3])) < 16777216.0 for row in (1, 2))
        p.flag[i] = (not force_direct) and small and all(e < 4096.0 for e in ext)
        if p.flag[i] and not capped:
            flat = G.reshape(-1, 2)
            L = tile_patch(ext, flat.min(axis=0), flat.max(axis=0), 2 * halo)
            if L is None:
                capped = True
            elif L[0] * L[1] * 4 > best:
                best, p.lds_dims = L[0] * L[1] * 4, (1,) + L
        for a in range(nT[0]):
            for b in range(nT[1]):
                (c1, n1), (c2, n2) = cells[0][a], cells[1][b]
                sub = G[c1:c1 + n1, c2:c2 + n2].reshape(-1, 2)
                umin, umax = sub.min(axis=0), sub.max(axis=0)
                idx = (i, a, b)
                p.cells[idx], p.nodes[idx], p.umin[idx], p.umax[idx] = (c1, c2), (n1, n2), umin, umax
                U = float(max(np.abs(umin).max(), np.abs(umax).max()))
                p.hull[idx] = U * p.gm1_max <= HULL_LIMIT
                L = tile_patch(ext, umin, umax, 2 * halo) if (p.flag[i] and p.hull[idx]) else None
                if L is None:
                    continue
                p.staged[idx], p.dims[idx] = True, L
                o = []
                for k, row in enumerate((1, 2)):
                    base = float(wm._fma(m[row, 1], a * T[0], wm._fma(m[row, 2], b * T[1], m[row, 3])))
                    o.append(int(np.floor(base + p.neg[i, k] + float(umin[k]) - BOX_MARGIN)) - halo)
                o[1] &= ~3
                p.origin[idx] = o
    if capped:
        best, p.lds_dims = PATCH_CAP, CAP_DIMS
    p.patch_bytes = best
    p.lds_bytes = SCRATCH_BYTES + 4 * p.node_floats + best
    return p


def tile_outcome(p, ms, src_hw):
    """Per (entry, tile): 'zero' (classified wholly outside), 'stage' or 'direct' for images of src_hw."""
    T = p.tile
    out = np.empty(p.staged.shape, dtype=object)
    for idx in np.ndindex(*p.staged.shape):
        i, a, b = idx
        m = np.eye(4) if ms is None else np.asarray(ms[i], np.float64)
        any_valid = True
        for k, row in enumerate((1, 2)):
            base = float(wm._fma(m[row, 1], a * T[0], wm._fma(m[row, 2], b * T[1], m[row, 3])))
            lo = base + p.neg[i, k] + float(p.umin[idx][k])
            hi = base + p.pos[i, k] + float(p.umax[idx][k])
            any_valid = any_valid and hi >= -0.5 - TILE_MARGIN and lo < src_hw[k] - 0.5 + TILE_MARGIN
        out[idx] = 'zero' if (p.hull[idx] and not any_valid) else ('stage' if p.staged[idx] else 'direct')
    return out


def violations(p, ms, grids, out, interp):
    """Staging safety: [(entry, tile, axis, lowest tap, highest tap, L)] over the staged tiles -- every tap index of every pixel of the
    tile inside the output must lie in [0, L) of the tile's patch; on x the cubic gather's aligned pairs count as read."""
    cubic = interp in CUBIC
    T = p.tile
    bad = []
    for i in range(p.staged.shape[0]):
        if not p.staged[i].any():
            continue
        y, x = coords(None if ms is None else ms[i], grid_of(grids, i), out)
        fl = [np.floor(y).astype(np.int64), np.floor(x).astype(np.int64)]
        for a, b in np.ndindex(*p.nT):
            if not p.staged[i, a, b]:
                continue
            sl = (slice(a * T[0], min((a + 1) * T[0], out[0])), slice(b * T[1], min((b + 1) * T[1], out[1])))
            for k in range(2):
                t = fl[k][sl] - int(p.origin[i, a, b][k])
                if cubic and k == 1:
                    x1 = t - 1
                    par = x1 & 1
                    lo, hi = int((x1 - par).min()), int((x1 - par + np.where(par == 1, 5, 3)).max())
                elif cubic:
                    lo, hi = int(t.min()) - 1, int(t.max()) + 2
                else:
                    lo, hi = int(t.min()), int(t.max()) + 1
                if lo < 0 or hi >= int(p.dims[i, a, b][k]):
                    bad.append((i, (a, b), k, lo, hi, int(p.dims[i, a, b][k])))
    return bad
