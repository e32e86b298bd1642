"""Host model of the tap indices of the three general-matrix kernels: affine_tiled (kind 2, vt_kernels_affine.hip), the lane-block kernel
(kind 9, vt_kernels_block.hip) and the packed-footprint kernel (kind 6, vt_kernels_packed.hip).  Plain numpy, no GPU, no pytest.

All three place a staged LDS box by the float64 bounding box of a tile (`lo = base + neg`), give it dims `L` the host planner worked
out from the matrix alone, and form tap coordinates in Q32.32 that advance with ROUNDED increments.  Whether every tap lands inside
what was staged is decided by that chain; this file repeats it step for step:

  * the planner: `pick_box_tile` / `finish_box` (kind 2), `plan_block_th` with its row and plane strides and the bank model that picks
    the plane padding (kind 9), `pick_packed_tile` with `invert3`, `PackGeom` and `packed_row_span` (kind 6; the lane-block kernel
    trims its staging by the same spans), `plan_prepare`'s depth increments, `set_tile_reach`;
  * the device chains: tile base, `lo`, `o` (with `o[2] &= ~3`), `b = base - o`; kind 2: `to_fx` of the column's fma chain and TD steps
    (interior and cut tiles read the same taps: the select comes after the gather); kind 9: `to_fx((base - o) + toff)` and the thread's
    NS voxels in Gray order with the increment table; kind 6: the general loop as kind 2 and the fast trilinear loop, whose start is
    `b + coff` where a thread serves one column and whose steps are single 64-bit adds.

A Q32.32 coordinate is held here as ONE int64 (hi * 2^32 + lo): fx_step's add-with-carry of two 32-bit words and the fast loop's
64-bit add are the same arithmetic modulo 2^64, and n steps are `c + n * inc`.  fma is emulated as box_index_model does.

`model(kind, m, out_shape, interp, ...)` returns a Result; `violations(res)` lists what left the staged image.  `PARAMS_BEFORE` is
the bare `floor(lo)` / `floor(ext)` the three kernels had before kBoxMargin reached them, `PARAMS` what they have now.
`reoriented()` repeats try_general_reorient (vt_api.hip): which resident copy a general launch samples, and with which matrix.
`inplane_origin_check()` is the few-line check of the kernels that form their in-plane coordinate once per pixel (kinds 8, 3, 4, 5).
"""
import collections

import numpy as np

from box_index_model import (_fma, _TWO32, Params, PARAMS, PARAMS_BEFORE, BOX_MARGIN, TILE_MARGIN, LDS_CAP, is_cubic,      # noqa: F401
                             fx_inc, to_fx)

AFFINE_TILES = ((16, 16, 16), (8, 16, 32), (8, 16, 16), (8, 8, 32), (4, 8, 32))      # kTiles (vt_kernels_affine.hip)
PACK_TILES = ((8, 16, 32), (16, 16, 16), (8, 8, 32))                                 # kPack (vt_kernels_packed.hip)
PACK_MAX_IT, PACK_ROWS_MAX = 16, 1024                                                # kPackMaxIt, kPackRowsMax
BLK_TD, BLK_TW = 8, 16                                                               # kBlkTD, kBlkTW
BLK_RS = (28, 36, 32, 12, 20, 16, 24)                                                # kBlkRS
BLK_ORDER = {16: (0, 1, 2), 8: (3, 4, 0, 1, 5, 6, 2)}                                # kOrder16, kOrder8
BLK_MAX_IT = {16: 20, 8: 13}                                                         # block_max_it
EXT_CAP = {2: 4096.0, 9: 256.0, 6: 1000.0}                                           # the planners' bounds on a tile's extent
PAD = 3                                                                              # the occupancy grid's rim (taps reach at most 2 beyond a box)


# ---------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------
def box_dims(m, T, halo2, params, ext_cap):
    """L[r] = floor(ext + extent margin) + 3 + halo2 (vt_plan.hip: pick_box_tile, plan_block_th, pick_packed_tile), before the
    alignment of L[2]; None when the extent is beyond the planner's bound."""
    L = []
    for r in range(3):
        ext = 0.0
        for k in range(3):
            ext += abs(float(m[r][k])) * (T[k] - 1)
        if not ext < ext_cap:
            return None
        L.append(int(np.floor(ext + params.extent_margin)) + 3 + halo2)
    return L


def tile_reach(m, T):
    """(neg, pos) of set_tile_reach."""
    neg, pos = [], []
    for r in range(3):
        n = p = 0.0
        for k in range(3):
            e = float(m[r][k]) * (T[k] - 1)
            if e < 0:
                n += e
            else:
                p += e
        neg.append(n)
        pos.append(p)
    return neg, pos


def _inc64(step):
    hi, lo = fx_inc(step)
    return hi * (1 << 32) + lo


def plan_box(m, cubic, params=PARAMS, lds_limit=LDS_CAP, cfg=None):
    """pick_box_tile + finish_box for a general (not axis-0-separable) matrix: the tile with the fewest staged bytes per voxel."""
    best, best_cost = None, 1e300
    for c, T in enumerate(AFFINE_TILES):
        if cfg is not None and c != cfg:
            continue
        L = box_dims(m, T, 2 if cubic else 0, params, EXT_CAP[2])
        if L is None:
            continue
        L[2] = (L[2] + 3 + 3) & ~3
        nbytes = L[0] * L[1] * L[2] * 4
        if nbytes > lds_limit:
            continue
        wg = min(8, (160 * 1024) // nbytes)
        cost = nbytes / float(T[0] * T[1] * T[2]) * (1.0 if wg >= 3 else (1.25 if wg == 2 else 2.0))
        if cost < best_cost:
            best_cost = cost
            best = dict(kind=2, cfg=c, tile=T, L=tuple(L), reported=tuple(L), lds_bytes=nbytes, alloc=L[0] * L[1] * L[2],
                        strides=(L[1] * L[2], L[2]), used=tuple(L))
    return best


def block_conflicts(m, RS, PS, cubic):
    """vt_plan.hip: block_conflicts with lane map 0."""
    kbase = ((8.13, 8.27, 8.41), (8.44, 8.50, 8.78), (8.71, 8.09, 8.33), (8.92, 8.66, 8.05))
    lanes = np.arange(32)
    t = (lanes >> 4, (lanes >> 2) & 3, lanes & 3)
    tot = 0.0
    for b in range(4):
        f = []
        for r in range(3):
            v = kbase[b][r] + 24.0
            for k in range(3):
                v = v + float(m[r][k]) * t[k]
            f.append(np.floor(v).astype(np.int64))
        a = f[0] * PS + f[1] * RS + ((((f[2] - 1) & ~1) >> 1) * 2 if cubic else f[2])
        words = np.unique((a >> 1) if cubic else a)
        tot += np.bincount(words % 32, minlength=32).max()
    return tot / 4.0


def invert3(m):
    A = [float(m[r][k]) for r in range(3) for k in range(3)]
    det = A[0] * (A[4] * A[8] - A[5] * A[7]) - A[1] * (A[3] * A[8] - A[5] * A[6]) + A[2] * (A[3] * A[7] - A[4] * A[6])
    amax = max(abs(a) for a in A)
    if not (abs(det) > 1e-6 * amax * amax * amax and amax < 64.0):
        return None
    d = 1.0 / det
    return [(A[4] * A[8] - A[5] * A[7]) * d, (A[2] * A[7] - A[1] * A[8]) * d, (A[1] * A[5] - A[2] * A[4]) * d,
            (A[5] * A[6] - A[3] * A[8]) * d, (A[0] * A[8] - A[2] * A[6]) * d, (A[2] * A[3] - A[0] * A[5]) * d,
            (A[3] * A[7] - A[4] * A[6]) * d, (A[1] * A[6] - A[0] * A[7]) * d, (A[0] * A[4] - A[1] * A[3]) * d]


def pack_geom(inv, neg, ext, T, halo, Lxbox, Lybox):
    cst = [inv[3 * c] * neg[0] + inv[3 * c + 1] * neg[1] + inv[3 * c + 2] * neg[2] for c in range(3)]
    return dict(inv=inv, cst=cst, ext=list(ext), T=tuple(T), halo=halo, Lxbox=Lxbox, Lybox=Lybox)


def packed_row_spans(g, Lz):
    """packed_row_span (vt_internal.h) for every row (Z, Y) of the box at once: (used[Lz, Ly], mn, mx)."""
    Ly, halo = g['Lybox'], g['halo']
    Z = np.arange(Lz, dtype=np.float64)[:, None]
    Y = np.arange(Ly, dtype=np.float64)[None, :]
    zlo, zhi = (Z - 2 - 2 * halo) - 1e-6, (Z + 1) + 1e-6
    ylo, yhi = (Y - 2 - 2 * halo) - 1e-6, (Y + 1) + 1e-6
    shape = (Lz, Ly)
    reach = ~np.broadcast_to((zhi < 0.0) | (zlo > g['ext'][0]) | (yhi < 0.0) | (ylo > g['ext'][1]), shape)
    LB = np.zeros(shape)
    UB = np.full(shape, float(g['ext'][2]))
    for c in range(3):
        gz, gy, gx = g['inv'][3 * c], g['inv'][3 * c + 1], g['inv'][3 * c + 2]
        if -1e-9 < gx < 1e-9:
            continue
        inv_gx = 1.0 / gx
        top = float(g['T'][c] - 1)
        lo_min = np.full(shape, 1e30)
        hi_max = np.full(shape, -1e30)
        for k in range(4):
            uz = zhi if (k & 1) else zlo
            uy = yhi if (k & 2) else ylo
            s = gz * uz + gy * uy + g['cst'][c]
            xa, xb = (0.0 - s) * inv_gx, (top - s) * inv_gx
            lo_min = np.minimum(lo_min, np.minimum(xa, xb))
            hi_max = np.maximum(hi_max, np.maximum(xa, xb))
        LB = np.maximum(LB, lo_min)
        UB = np.minimum(UB, hi_max)
    ok = reach & ~(LB > UB + 1e-6)
    a = np.maximum(np.floor(LB - 1e-6).astype(np.int64), 0)
    b = np.minimum(np.floor(UB + 1e-6 + float(halo) + 4.0).astype(np.int64) + 1 + halo, g['Lxbox'] - 1)
    used = ok & (a <= b)
    return used, np.where(used, a, 0), np.where(used, b, -1)


def plan_block(m, cubic, params=PARAMS, lds_limit=LDS_CAP, th=None, trim=True):
    """plan_block / plan_block_th: the half-height tile first (VT_BLOCK_TH's default), else the full-height one; `th` forces one."""
    for h in ((8, 16) if th is None else (th,)):
        T = (BLK_TD, h, BLK_TW)
        L = box_dims(m, T, 2 if cubic else 0, params, EXT_CAP[9])
        if L is None:
            return None
        lx_used = (L[2] + 3 + 3) & ~3
        maxvec = 256 * BLK_MAX_IT[h]
        got = None
        for idx in BLK_ORDER[h]:
            rs = BLK_RS[idx]
            if rs < lx_used:
                continue
            best_pad, best_f = 0, 1e300
            for pad in range(0, 64, 4):
                if L[0] * (L[1] * rs + pad) // 4 > maxvec:
                    break
                f = block_conflicts(m, rs, L[1] * rs + pad, cubic) * (1.0 + 0.002 * pad)
                if f < best_f - 1e-9:
                    best_f, best_pad = f, pad
            ps = L[1] * rs + best_pad
            vec = L[0] * ps // 4
            if vec > maxvec:
                continue
            got = (idx, rs, ps, vec)
            break
        if got is None:
            continue
        idx, rs, ps, vec = got
        box_bytes = (vec + 63) // 64 * 64 * 16
        if box_bytes + 16 > lds_limit:
            continue
        neg, pos = tile_reach(m, T)
        plan = dict(kind=9, cfg=idx, tile=T, L=tuple(L), reported=(L[0], L[1], rs), lds_bytes=box_bytes + 16, alloc=box_bytes // 4,
                    strides=(ps, rs), used=(L[0], L[1], lx_used), geom=None)
        inv = invert3(m)
        if trim and inv is not None:
            plan['geom'] = pack_geom(inv, neg, [pos[r] - neg[r] for r in range(3)], T, 1 if cubic else 0, lx_used, L[1])
        return plan
    return None


def plan_packed(m, cubic, params=PARAMS, lds_limit=LDS_CAP, cfg=None):
    """pick_packed_tile for the kernel of vt_kernels_packed.hip (cubic launches, and trilinear ones of a handle made under VT_SPAN=0),
    as VT_FORCE_PACKED plans it: no minimum tile count."""
    inv = invert3(m)
    if inv is None:
        return None
    best, best_cost = None, 1e300
    for c, T in enumerate(PACK_TILES):
        if cfg is not None and c != cfg:
            continue
        L = box_dims(m, T, 2 if cubic else 0, params, EXT_CAP[6])
        if L is None:
            continue
        L[2] = (L[2] + 3 + 3) & ~3
        rows = L[0] * L[1]
        if rows > PACK_ROWS_MAX or L[2] > 4000 or L[1] > 1023 or L[0] > 511:
            continue
        neg, pos = tile_reach(m, T)
        ext = [sum(abs(float(m[r][k]) * (T[k] - 1)) for k in range(3)) for r in range(3)]
        g = pack_geom(inv, neg, ext, T, 1 if cubic else 0, L[2], L[1])
        used, mn, mx = packed_row_spans(g, L[0])
        nvec = int(np.where(used, ((mx - (mn & ~3)) >> 2) + 1, 0).sum())
        cap_vec = nvec + rows // 16 + 8
        if cap_vec > 256 * PACK_MAX_IT:
            continue
        table_floats = (2 * rows + 8 + 3) & ~3
        nbytes = (table_floats + cap_vec * 4) * 4
        if nbytes > lds_limit:
            continue
        wg = min(2 if cubic else 3, (160 * 1024) // nbytes)
        cost = nbytes / float(T[0] * T[1] * T[2]) * (1.0 if wg >= 3 else (1.2 if wg == 2 else 2.0))
        if cost < best_cost:
            best_cost = cost
            best = dict(kind=6, cfg=c, tile=T, L=tuple(L), reported=(L[0], L[1], cap_vec * 4), lds_bytes=nbytes, alloc=cap_vec * 4,
                        strides=None, used=tuple(L), geom=g, nvec=nvec)
    return best


def staged_mask(plan):
    """bool[Lz, Ly, Lx_used]: the box cells a tile stages (from the source, or as border zeros).  Kind 2 stages the whole box; kind 6 the
    16-byte vectors that cover each row's span; kind 9 the vectors cx in [mn >> 2, mx >> 2] of each row when it trims."""
    Lz, Ly, Lx = plan['used']
    g = plan.get('geom')
    if g is None:
        return np.ones((Lz, Ly, Lx), bool)
    used, mn, mx = packed_row_spans(g, Lz)
    x = np.arange(Lx)[None, None, :]
    return used[:, :, None] & (x >= (mn & ~3)[:, :, None]) & (x <= ((mx >> 2) * 4 + 3)[:, :, None])


def packed_rowbase(plan):
    """Float offset of column 0 of every row inside the footprint buffer (the kernel's rowbase table after its set-up)."""
    Lz = plan['used'][0]
    used, mn, mx = packed_row_spans(plan['geom'], Lz)
    x0 = np.where(used, mn & ~3, 0).ravel()
    nv = np.where(used, ((mx - (mn & ~3)) >> 2) + 1, 0).ravel()
    first = np.concatenate(([0], np.cumsum(nv)[:-1]))
    return 4 * first - x0


PLANNERS = {2: plan_box, 9: plan_block, 6: plan_packed}
_PLAN_MEMO = {}


def plan_of(kind, m, cubic, params=PARAMS, **force):
    """PLANNERS[kind](...), remembered: a plan depends on the linear part alone, and the tables hold few distinct ones."""
    key = (kind, np.asarray(m, np.float64)[:3, :3].tobytes(), bool(cubic), tuple(params), tuple(sorted(force.items())))
    if key not in _PLAN_MEMO:
        _PLAN_MEMO[key] = PLANNERS[kind](m, cubic, params, **force)
    return _PLAN_MEMO[key]


def reoriented(m, shape, n_out=None, forced=True):
    """try_general_reorient: (matrix with its rows permuted, source dims of the copy, source axis of each copy axis).  Under
    VT_FORCE_TILED the exchanged copy is built at the first call that asks for it."""
    m = np.asarray(m, np.float64)
    c = [abs(m[0][2]), abs(m[1][2]), abs(m[2][2])]
    a = 2
    if c[1] > 1.15 * c[2] and c[1] >= c[0]:
        a = 1
    if c[0] > 1.15 * c[2] and c[0] > c[1]:
        a = 0
    pi = {2: (0, 1, 2), 1: (0, 2, 1), 0: (2, 1, 0)}[a]
    return m[list(pi) + [3]] if m.shape[0] == 4 else m[list(pi)], tuple(shape[k] for k in pi), pi


def resident_pitch(W):
    return (W + 4 + 31) & ~31


# ---------------------------------------------------------------------------------------------------
# the device chains
# ---------------------------------------------------------------------------------------------------
def _tiles(m, out_shape, T, neg, pos, src_shape, params, halo):
    """Per tile (flat, d slowest): d0, h0, w0, base[3], o[3], any_valid, all_valid."""
    oD, oH, oW = out_shape
    d0, h0, w0 = np.meshgrid(np.arange((oD + T[0] - 1) // T[0], dtype=np.int64) * T[0], np.arange((oH + T[1] - 1) // T[1], dtype=np.int64) * T[1],
                             np.arange((oW + T[2] - 1) // T[2], dtype=np.int64) * T[2], indexing='ij')
    d0, h0, w0 = d0.ravel(), h0.ravel(), w0.ravel()
    any_valid = np.ones(d0.shape, bool)
    all_valid = np.ones(d0.shape, bool)
    base, o = [], []
    for r in range(3):
        b = _fma(m[r][0], d0, _fma(m[r][1], h0, _fma(m[r][2], w0, float(m[r][3]))))
        lo, hi = b + neg[r], b + pos[r]
        vlo, vhi = -0.5, float(src_shape[r]) - 0.5
        any_valid &= (hi >= vlo - TILE_MARGIN) & (lo < vhi + TILE_MARGIN)
        all_valid &= (lo >= vlo + TILE_MARGIN) & (hi < vhi - TILE_MARGIN)
        orr = np.floor(lo - params.origin_margin).astype(np.int64) - halo
        if r == 2:
            orr &= ~np.int64(3)
        base.append(b)
        o.append(orr)
    return d0, h0, w0, base, o, any_valid, all_valid


def _fx64(s):
    hi, lo = to_fx(s)
    return hi * np.int64(1 << 32) + lo.astype(np.int64)


def _chain_columns(kind, m, out_shape, plan, tl, fast_linear):
    """Kinds 2 and 6: (idx[3] as int64 [tiles, TH, TW, TD], active mask, (d, h, w) of every entry, tiles on the fast path)."""
    TD, TH, TW = plan['tile']
    oD, oH, oW = out_shape
    d0, h0, w0, base, o, any_valid, all_valid = tl
    sel = np.flatnonzero(any_valid)
    d0, h0, w0 = d0[sel], h0[sel], w0[sel]
    j = np.arange(TH, dtype=np.int64)[None, :, None]
    kw = np.arange(TW, dtype=np.int64)[None, None, :]
    nd = np.minimum(TD, oD - d0)
    fast = np.zeros(sel.shape, bool)
    NJ = TH // (256 // TW)
    if kind == 6 and fast_linear:
        fast = all_valid[sel] & (nd == TD) & (h0 + TH <= oH) & (w0 + TW <= oW)
    steps = np.arange(TD, dtype=np.int64)
    idx = []
    for r in range(3):
        b = (base[r][sel] - o[r][sel].astype(np.float64))[:, None, None]
        s = _fma(m[r][1], j, _fma(m[r][2], kw, b))
        if fast.any() and NJ == 1:
            coff = _fma(m[r][1], j, float(m[r][2]) * kw.astype(np.float64))          # per thread, once per launch
            s = np.where(fast[:, None, None], b + coff, s)
        c = _fx64(s)[..., None] + np.int64(_inc64(m[r][0])) * steps
        idx.append(c >> np.int64(32))
    act = ((h0[:, None, None] + j < oH) & (w0[:, None, None] + kw < oW))[..., None] & (steps[None, None, None, :] < nd[:, None, None, None])
    act = act | fast[:, None, None, None]
    shape = idx[0].shape
    vox = (np.broadcast_to(d0[:, None, None, None] + steps, shape), np.broadcast_to((h0[:, None, None] + j)[..., None], shape),
           np.broadcast_to((w0[:, None, None] + kw)[..., None], shape))
    return idx, act, vox, sel, int(fast.sum())


def _chain_block(m, out_shape, plan, tl):
    """Kind 9: (idx[3] [tiles, 256 threads, NS], active mask (every voxel of a staged tile gathers), (d, h, w), staged tiles)."""
    TD, TH, TW = plan['tile']
    d0, h0, w0, base, o, any_valid, _ = tl
    sel = np.flatnonzero(any_valid)
    d0, h0, w0 = d0[sel], h0[sel], w0[sel]
    tid = np.arange(256, dtype=np.int64)
    lane, wv = tid & 63, tid >> 6
    vd, vh, vw = lane >> 4, 4 * (wv >> 1) + ((lane >> 2) & 3), 4 * (wv & 1) + (lane & 3)
    if TH == 16:
        sd, sh, sw, which = (0, 0, 0, 0, 4, 4, 4, 4), (0, 0, 8, 8, 8, 8, 0, 0), (0, 8, 8, 0, 0, 8, 8, 0), (0, 1, 2, 3, 0, 4, 2)
    else:
        sd, sh, sw, which = (0, 0, 4, 4), (0, 0, 0, 0), (0, 8, 8, 0), (0, 3, 2)
    col, mul, neg_of = (2, 1, 2, 0, 1), (8.0, 8.0, -8.0, 4.0, -8.0), (-1, -1, 0, -1, 1)
    idx = []
    for r in range(3):
        binc = [0] * 5
        for s in range(5):
            binc[s] = -binc[neg_of[s]] if neg_of[s] >= 0 else _inc64(float(m[r][col[s]]) * mul[s])
        toff = _fma(m[r][0], vd, _fma(m[r][1], vh, float(m[r][2]) * vw.astype(np.float64)))
        c0 = _fx64((base[r][sel] - o[r][sel].astype(np.float64))[:, None] + toff[None, :])
        offs = np.concatenate(([0], np.cumsum([binc[w] for w in which], dtype=np.int64))).astype(np.int64)
        idx.append((c0[..., None] + offs) >> np.int64(32))
    shape = idx[0].shape
    vox = (np.broadcast_to(d0[:, None, None] + vd[None, :, None] + np.asarray(sd)[None, None, :], shape),
           np.broadcast_to(h0[:, None, None] + vh[None, :, None] + np.asarray(sh)[None, None, :], shape),
           np.broadcast_to(w0[:, None, None] + vw[None, :, None] + np.asarray(sw)[None, None, :], shape))
    return idx, np.ones(shape, bool), vox, sel, 0


# ---------------------------------------------------------------------------------------------------
# what the taps read
# ---------------------------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'kind plan tiled tile reported lds_bytes lo hi flat_lo flat_hi alloc tiles staged fast outside unstaged '
                                          'table below origin', defaults=(None,))
Below = collections.namedtuple('Below', 'voxel index origin reads')      # output (d, h, w); box index of floor; tile origin; [(cell, flat address)] of the taps below the box


def _stencil(cubic):
    r = range(-1, 3) if cubic else range(0, 2)
    return [(a, b, c) for a in r for b in r for c in r]


def _flat(plan, rowbase, Z, Y, X):
    """Flat float address of box cell (Z, Y, X) as the gather forms it, and whether a row-table entry exists for it (kind 6)."""
    if plan['kind'] == 6:
        Ly = plan['used'][1]
        row = Z * Ly + Y
        ok = (row >= 0) & (row < rowbase.size)
        return rowbase[np.clip(row, 0, rowbase.size - 1)] + X, ok
    ps, rs = plan['strides']
    return Z * ps + Y * rs + X, np.ones(np.shape(Z), bool)


def model(kind, m, out_shape, interp, src_shape=None, params=PARAMS, fast_linear=True, origins=False, **force):
    """One launch of kernel `kind` (2, 9 or 6) with pull matrix m on an output of out_shape, sampling a source of src_shape (default:
    out_shape).  `force`: cfg= (kinds 2, 6), th= / trim= (kind 9).  origins=True: Result.origin is int64 [3, D, H, W], the SOURCE index
    (of the copy the launch samples) of the floor tap of every output voxel of a staged tile, the smallest int64 elsewhere."""
    m = np.asarray(m, np.float64)
    cubic = is_cubic(interp)
    halo = 1 if cubic else 0
    src_shape = tuple(out_shape) if src_shape is None else tuple(src_shape)
    plan = plan_of(kind, m, cubic, params, **force)
    if plan is None:
        return Result(kind, None, False, None, None, 0, None, None, None, None, 0, 0, 0, 0, [], [], [], [])
    T = plan['tile']
    neg, pos = tile_reach(m, T)
    tl = _tiles(m, out_shape, T, neg, pos, src_shape, params, halo)
    if kind == 9:
        idx, act, vox, sel, fast = _chain_block(m, out_shape, plan, tl)
    else:
        idx, act, vox, sel, fast = _chain_columns(kind, m, out_shape, plan, tl, fast_linear and not cubic)
    ntiles = int(tl[0].size)
    if sel.size == 0 or not act.any():
        return Result(kind, plan, True, T, plan['reported'], plan['lds_bytes'], None, None, None, None, plan['alloc'], ntiles, 0, 0, [], [], [], [])
    a = np.flatnonzero(act.ravel())
    z, y, x = (i.ravel() if a.size == act.size else i.ravel()[a] for i in idx)
    used = plan['used']
    lo = [int(v.min()) - halo for v in (z, y, x)]
    hi = [int(v.max()) + 1 + halo for v in (z, y, x)]
    # occupancy of the box cells (floor indices), on a grid with a rim of PAD cells; a coordinate beyond the rim is clipped onto it
    dims = tuple(u + 2 * PAD for u in used)
    within = all(lo[r] + halo >= -PAD and hi[r] - 1 - halo < used[r] + PAD for r in range(3))
    zc, yc, xc = (v + PAD if within else np.clip(v + PAD, 0, dd - 1) for v, dd in zip((z, y, x), dims))
    occ = np.zeros(dims, bool)
    occ.ravel()[(zc * dims[1] + yc) * dims[2] + xc] = True
    cells = np.argwhere(occ) - PAD                                    # distinct floor cells
    # taps: the stencil around every floor cell
    tapped = np.zeros(dims, bool)
    for dz, dy, dx in _stencil(cubic):
        src = occ[max(0, -dz):dims[0] - max(0, dz), max(0, -dy):dims[1] - max(0, dy), max(0, -dx):dims[2] - max(0, dx)]
        tapped[max(0, dz):dims[0] - max(0, -dz), max(0, dy):dims[1] - max(0, -dy), max(0, dx):dims[2] - max(0, -dx)] |= src
    staged = np.zeros(dims, bool)
    staged[PAD:PAD + used[0], PAD:PAD + used[1], PAD:PAD + used[2]] = staged_mask(plan)
    inbox = np.zeros(dims, bool)
    inbox[PAD:PAD + used[0], PAD:PAD + used[1], PAD:PAD + used[2]] = True
    outside = [tuple(int(v) for v in c) for c in np.argwhere(tapped & ~inbox) - PAD]
    unstaged = [tuple(int(v) for v in c) for c in np.argwhere(tapped & inbox & ~staged) - PAD]
    # addresses actually read, per floor cell: trilinear two floats per tap row, cubic the aligned pairs (4 or 6 floats per tap row)
    rowbase = packed_rowbase(plan) if kind == 6 else None
    Z, Y, X = cells[:, 0], cells[:, 1], cells[:, 2]
    flat_lo = flat_hi = None
    table = []
    if cubic:
        x1 = X - 1
        par = x1 & 1
        first_x, last_x = x1 - par, x1 - par + np.where((par == 1) | (kind == 9), 5, 3)
        rows = [(dz, dy) for dz in range(-1, 3) for dy in range(-1, 3)]
    else:
        first_x, last_x = X, X + 1
        rows = [(dz, dy) for dz in range(2) for dy in range(2)]
    for dz, dy in rows:
        fa, ok = _flat(plan, rowbase, Z + dz, Y + dy, first_x)
        fz, _ = _flat(plan, rowbase, Z + dz, Y + dy, last_x)
        if not ok.all():
            table += [tuple(int(v) for v in c) for c in np.stack((Z + dz, Y + dy), 1)[~ok]]
        if ok.any():
            flat_lo = int(fa[ok].min()) if flat_lo is None else min(flat_lo, int(fa[ok].min()))
            flat_hi = int(fz[ok].max()) if flat_hi is None else max(flat_hi, int(fz[ok].max()))
    if kind == 6 and not cubic:
        # the row-pair read at entry (z, y) also fetches entry (z, y) + 1
        bad = ~((Z * used[1] + Y >= 0) & (Z * used[1] + Y + 1 < rowbase.size))
        table += [tuple(int(v) for v in c) for c in np.stack((Z, Y), 1)[bad]]
    below = []
    if min(lo) < 0:
        bm = (z < halo) | (y < halo) | (x < halo)
        if True:
            st = _stencil(cubic)
            o = tl[4]
            tile_of = np.broadcast_to(sel.reshape((-1,) + (1,) * (act.ndim - 1)), act.shape).ravel()[a][bm]
            vd, vh, vw = (v.ravel()[a][bm] for v in vox)
            for n, (bz, by, bx) in enumerate(zip(z[bm], y[bm], x[bm])):
                reads = []
                for dz, dy, dx in st:
                    cz, cy, cx = int(bz) + dz, int(by) + dy, int(bx) + dx
                    if cz < 0 or cy < 0 or cx < 0:
                        f, ok = _flat(plan, rowbase, np.int64(cz), np.int64(cy), np.int64(cx))
                        reads.append(((cz, cy, cx), int(f) if bool(ok) else None))
                t = int(tile_of[n])
                below.append(Below((int(vd[n]), int(vh[n]), int(vw[n])), (int(bz), int(by), int(bx)), (int(o[0][t]), int(o[1][t]), int(o[2][t])), reads))
    origin = None
    if origins:
        origin = np.full((3,) + tuple(out_shape), np.iinfo(np.int64).min, np.int64)
        ok = act & (vox[0] < out_shape[0]) & (vox[1] < out_shape[1]) & (vox[2] < out_shape[2])
        at = tuple(v[ok] for v in vox)
        for r in range(3):
            origin[r][at] = (idx[r] + tl[4][r][sel].reshape((-1,) + (1,) * (act.ndim - 1)))[ok]
    return Result(kind, plan, True, T, plan['reported'], plan['lds_bytes'], lo, hi, flat_lo, flat_hi, plan['alloc'], ntiles, int(sel.size), fast,
                  outside, unstaged, sorted(set(table)), below, origin)


def violations(res):
    """What left the staged image: ('axis', r, lowest, highest, L) per axis with a tap outside [0, L); ('flat', lowest, highest, floats
    allocated) when an address that is actually read lies outside the allocation; ('unstaged', cells) for taps inside the box on cells
    the footprint did not stage; ('table', rows) for row-table entries that do not exist (kind 6)."""
    out = []
    if not res.tiled or res.lo is None:
        return out
    used = res.plan['used']
    for r in range(3):
        if res.lo[r] < 0 or res.hi[r] >= used[r]:
            out.append(('axis', r, res.lo[r], res.hi[r], used[r]))
    if res.flat_lo is not None and (res.flat_lo < 0 or res.flat_hi >= res.alloc):
        out.append(('flat', res.flat_lo, res.flat_hi, res.alloc))
    if res.unstaged:
        out.append(('unstaged', res.unstaged[:4], len(res.unstaged)))
    if res.table:
        out.append(('table', res.table[:4], len(res.table)))
    return out


def wrapped_source_voxels(res, src_shape):
    """For the voxels of res.below: {output voxel: [source voxel]} of the zero-weight taps below the box whose flat address falls INSIDE
    the allocation on a cell the tile staged from a source voxel inside the volume (kinds 2 and 9: the address decodes through the
    box strides; kind 6: through the row table)."""
    plan = res.plan
    out = {}
    mask = staged_mask(plan)
    if plan['kind'] == 6:
        rowbase = packed_rowbase(plan)
        Lz, Ly, Lx = plan['used']
        used, mn, mx = packed_row_spans(plan['geom'], Lz)
        x0 = np.where(used, mn & ~3, 0).ravel()
        nv = np.where(used, ((mx - (mn & ~3)) >> 2) + 1, 0).ravel()
        start = rowbase + x0                                            # first float of each row in the buffer
    for b in res.below:
        for cell, f in b.reads:
            if f is None or f < 0 or f >= res.alloc:
                continue
            if plan['kind'] == 6:
                rows = np.flatnonzero((start <= f) & (f < start + 4 * nv))
                if rows.size != 1:
                    continue
                row = int(rows[0])
                c = (row // Ly, row % Ly, int(f - rowbase[row]))
            else:
                ps, rs = plan['strides']
                c = (f // ps, (f % ps) // rs, (f % ps) % rs)
            if not all(0 <= c[k] < plan['used'][k] for k in range(3)) or not mask[c]:
                continue
            s = tuple(b.origin[k] + c[k] for k in range(3))
            if all(0 <= s[k] < src_shape[k] for k in range(3)):
                out.setdefault(b.voxel, []).append(s)
    return out


# ---------------------------------------------------------------------------------------------------
# kinds 8, 3, 4, 5: the in-plane origin is a bare floor(lo) too, but the coordinate is formed ONCE per pixel from the float64 chain
# ---------------------------------------------------------------------------------------------------
def inplane_origin_check(m, out_shape, th, tw, cubic, origin_margin=0.0):
    """Pixels of an axis-0-separable launch whose in-plane floor index is below the halo: floor(chain coordinate) - o < HALO with
    o = floor(base + neg - origin_margin) - HALO, base and the per-pixel coordinate as vt_kernels_quad.hip / vt_kernels_march.hip /
    affine_tiled_zsep form them (rows 1 and 2; tile reach over the in-plane axes only).  No Q32.32 stepping here: only double rounding -- of
    `base + neg`, a sum of ROUNDED products, against the pixel's own fma chain -- can put a pixel there.  [(h, w, axis, floor index - HALO,
    the float32 fraction)]."""
    m = np.asarray(m, np.float64)
    halo = 1 if cubic else 0
    oH, oW = out_shape[1], out_shape[2]
    h0 = (np.arange((oH + th - 1) // th, dtype=np.int64) * th)[:, None, None, None]
    w0 = (np.arange((oW + tw - 1) // tw, dtype=np.int64) * tw)[None, :, None, None]
    j = np.arange(th, dtype=np.int64)[None, None, :, None]
    kw = np.arange(tw, dtype=np.int64)[None, None, None, :]
    bad = []
    for r in (1, 2):
        neg = 0.0
        for k, t in ((1, th), (2, tw)):
            e = float(m[r][k]) * (t - 1)
            if e < 0:
                neg += e
        base = _fma(m[r][1], h0, _fma(m[r][2], w0, float(m[r][3])))
        o = np.floor(base + neg - origin_margin) - halo
        s = _fma(m[r][1], j, _fma(m[r][2], kw, base - o))
        live = (h0 + j < oH) & (w0 + kw < oW)
        fl = np.floor(s)
        for hit in np.argwhere((fl < halo) & live):
            at = tuple(hit)
            bad.append((int(h0.ravel()[hit[0]] + hit[2]), int(w0.ravel()[hit[1]] + hit[3]), r, int(fl[at]) - halo, float(np.float32(s[at] - fl[at]))))
    return bad


# ---------------------------------------------------------------------------------------------------
# the poisoned-neighbour cases of tests/test_gpu_affine_index.py
# ---------------------------------------------------------------------------------------------------
def lead_cases(shape):
    """Dedicated one-axis leads, placed as test_box_index_model.lead_matrix does (identity, one row replaced, integer offsets): every row
    with a negative entry of every 3-4-5 and thirds part, on every axis it can drive.  (name, m64)."""
    import lattice_cases as lc
    parts = lc.linear_parts()
    out = []
    for label, L in parts['rot345'] + parts['thirds']:
        for r in range(3):
            for ri, row in enumerate(L):
                if row[r] == 0.0 or not (row < 0).any():
                    continue
                m = np.eye(4)
                m[r, :3] = row
                m[:3, 3] = np.floor(np.asarray(shape, np.float64) / 3.0)
                m[r, 3] = np.floor(shape[r] / 2.0)
                out.append((f'lead_{label}_ax{r}_row{ri}', m))
    return out


# (kernel, interpolation class) -> [(index into the two shapes, case name)]: cases whose PARAMS_BEFORE model lists voxels below the box with
# a wrapped read inside the allocation on a staged source voxel inside the volume.  From the lattice tables where they hold one; the
# lane-block kernel's tables hold none (a wrapped read of its trimmed, stride-padded image lands on a slot the tile did not stage), its
# trilinear form has one among the dedicated leads and its cubic form none at all: no poisoned node for (9, cubic).
# tests/test_affine_index_model.py holds every entry to its condition.
POISON_CASES = {
    (2, 'linear'): [(0, '057_lattice_r345q_ax1'), (0, '074_lattice_r345_ax1'), (1, '064_lattice_r345q_ax0')],
    (2, 'cubic'): [(0, '064_lattice_r345q_ax0'), (0, '060_lattice_r345_ax0'), (1, '154_lattice_r345q_ax0')],
    (6, 'linear'): [(0, '057_lattice_r345q_ax1'), (0, '074_lattice_r345_ax1'), (0, '162_lattice_r345q_ax1')],
    (6, 'cubic'): [(0, '126_lattice_thirds'), (0, '130_lattice_thirds'), (1, '126_lattice_thirds')],
    (9, 'linear'): [(1, 'lead_r345q_ax0_ax2_row1')],
}
MAX_POISON = 24


def launch_geometry(kind, m, shape, interp, params=PARAMS):
    """The model of the launch the library makes for kind's flag set: on the axis-permuted copy try_general_reorient picks when the
    planner serves the permuted matrix with this kernel, else on the plain copy.  (Result, source dims of the copy, source axis of each
    copy axis)."""
    mr, sshape, pi = reoriented(m, shape)
    res = model(kind, mr, shape, interp, src_shape=sshape, params=params)
    if not res.tiled and pi != (0, 1, 2):
        mr, sshape, pi = np.asarray(m, np.float64), tuple(shape), (0, 1, 2)
        res = model(kind, mr, shape, interp, src_shape=sshape, params=params)
    return res, sshape, pi


def poison_plan(kind, m, shape, interp):
    """What the poisoned-neighbour test needs of one case: `listed` output voxels (n, 3) whose lowest tap is below the box under
    PARAMS_BEFORE, `poison` source voxels (k, 3) their wrapped reads land on -- none of them within the stencil, widened by one voxel per
    axis on the low side, of ANY listed voxel --, and `allowed`: the output voxels whose widened stencil holds a poisoned voxel."""
    import lattice_cases as lc
    m = np.asarray(m, np.float64)
    halo = 1 if is_cubic(interp) else 0
    res, sshape, pi = launch_geometry(kind, m, shape, interp, PARAMS_BEFORE)
    empty = dict(listed=np.zeros((0, 3), np.int64), poison=np.zeros((0, 3), np.int64), allowed=np.zeros(shape, bool), pi=pi)
    if not res.tiled or not res.below:
        return empty
    wraps = {}
    for vox, cells in wrapped_source_voxels(res, sshape).items():
        for c in cells:
            s = [0, 0, 0]
            for r in range(3):
                s[pi[r]] = c[r]
            wraps.setdefault(vox, set()).add(tuple(s))
    wraps = {v: w for v, w in wraps.items() if all(v[k] < shape[k] for k in range(3))}
    if not wraps:
        return empty
    f = np.floor(lc.chain_coords(m, shape)).astype(np.int64)          # [3, D, H, W]
    lv = np.asarray(sorted(wraps), np.int64)
    flo = np.stack([f[r][lv[:, 0], lv[:, 1], lv[:, 2]] for r in range(3)], 1) - halo - 1
    fhi = flo + 2 * halo + 2
    cand = np.asarray(sorted(set().union(*wraps.values())), np.int64)
    clear = np.array([not np.any(np.all((p >= flo) & (p <= fhi), axis=1)) for p in cand], bool)
    cand = cand[clear]
    # The drift goes EITHER way (vt_device.h, struct Fx): a coordinate within 2^-24 BELOW an integer k may arrive as k with fraction 0, and its
    # zero-weight tap is then the one ABOVE the float64 stencil.  The rule "widened on the low side" cannot judge such a voxel, so no
    # poisoned voxel is placed on the extra high-side taps of any of them: the rule stays decidable on every output voxel.
    s = lc.chain_coords(m, shape)
    amb = (s - f) > 1.0 - 2.0 ** -24                                    # [3, D, H, W]
    av = np.flatnonzero(amb.any(axis=0).ravel())
    if av.size and cand.size:
        fa = np.stack([f[r].ravel()[av] for r in range(3)], 1)
        aa = np.stack([amb[r].ravel()[av] for r in range(3)], 1).astype(np.int64)
        keep = []
        for p in cand[:8 * MAX_POISON]:
            wide = np.all((p >= fa - halo - 1) & (p <= fa + halo + 1 + aa), axis=1)
            low = np.all((p >= fa - halo - 1) & (p <= fa + halo + 1), axis=1)
            keep.append(not np.any(wide & ~low))
        cand = cand[:8 * MAX_POISON][np.asarray(keep, bool)]
    cand = cand[:MAX_POISON]
    chosen = set(map(tuple, cand.tolist()))
    listed = np.asarray([v for v in sorted(wraps) if wraps[v] & chosen], np.int64).reshape(-1, 3)
    allowed = np.zeros(shape, bool)
    for p in cand:
        hit = np.ones(shape, bool)
        for r in range(3):
            hit &= (p[r] >= f[r] - halo - 1) & (p[r] <= f[r] + halo + 1)
        allowed |= hit
    return dict(listed=listed, poison=cand.reshape(-1, 3), allowed=allowed, pi=pi)
