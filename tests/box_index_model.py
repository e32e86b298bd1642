"""Host model of the tap indices of the box kernels (kinds 11-16): plain numpy, no GPU, no pytest.

The six kernels (extract_tiled, project_tiled, extract_sum, extract_dot, extract_dot_multi, extract_sum_multi) repeat one geometry:
a float64 bounding box per tile, an integer origin `o` of the staged LDS box, box dims `L` from the host planner, and Q32.32 tap
coordinates that restart at every tile column and advance along the tile's depth by `fx_step` with a ROUNDED increment.  Whether every
tap lands inside [0, L) is decided by that chain and by nothing else; this file repeats it step for step:

  * the planner: `extract_pick_tile`, `extract_box_dims`, `extract_fill_entry` (vt_kernels_extract.hip) and
    `project_batch_shape_plan` (vt_kernels_projbatch.hip);
  * the device chain: tile base, `lo` / `hi`, `o` with `o[2] &= ~3`, `b = base - o`, `to_fx` per column and lane group, `fx_step` over
    the depth.

fma is emulated as `lattice_cases.chain_coords` does (longdouble product-sum rounded to float64).  `model(m, box, interp)` returns the
tile, the staged dims and, per axis, the lowest and highest box index any tap of any voxel of any tile reads -- a voxel of a cut tile
reads its taps whether or not it is inside, the select comes after the gather.  `PARAMS` holds the two places a fix can touch (where
the origin goes, how the extent is rounded); `PARAMS_BEFORE` are the values the kernels had before the origin margin was introduced,
kept so that the test can show what the model said then.
"""
import collections

import numpy as np

TILES = ((16, 16, 16), (8, 16, 16), (8, 8, 16))          # kExtractTiles
LDS_CAP = 160 * 1024                                       # the handle's lds_limit on gfx950
TILE_MARGIN = 1.0e-6                                       # kTileMargin
BOX_MARGIN = 2.0 ** -24                                    # kBoxMargin (vt_device.h)
CUBIC = ('bspline', 'bspline_simple', 'filt_bspline', 'filt_bspline_simple')

Params = collections.namedtuple('Params', 'origin_margin extent_margin')
PARAMS = Params(BOX_MARGIN, 2 * BOX_MARGIN)                # o = floor(lo - kBoxMargin) - HALO;  L = floor(ext + 2 kBoxMargin) + 3 + halo2
PARAMS_BEFORE = Params(0.0, 0.0)                           # o = floor(lo) - HALO;               L = floor(ext) + 3 + halo2

_LD = np.longdouble
_TWO32 = 4294967296.0


def _fma(a, x, c):
    """a * x + c with one rounding, a float64 scalar, x integers below 2^11 (exact longdouble products)."""
    return (_LD(a) * np.asarray(x, _LD) + np.asarray(c, _LD)).astype(np.float64)


def is_cubic(interp):
    return interp in CUBIC


# ---------------------------------------------------------------------------------------------------
# Q32.32 (vt_device.h: Fx, to_fx, fx_step; the host's split of a step: plan_prepare, extract_fill_entry)
# ---------------------------------------------------------------------------------------------------
def fx_inc(step):
    """(inc_hi, inc_lo) of a float64 step: floor and the fraction ROUNDED to the nearest unit of 2^-32."""
    step = float(step)
    fl = np.floor(step)
    hi = int(fl) if abs(step) < 2.0e9 else 0
    scaled = (step - fl) * _TWO32 + 0.5
    lo = int(min(4294967295.0, np.floor(scaled)))
    if scaled >= _TWO32:
        lo, hi = 0, hi + 1
    return hi, lo


def to_fx(s):
    """(hi as int64, lo as uint64) of float64 coordinates: floor and the fraction TRUNCATED, as the device's (unsigned) conversion."""
    fl = np.floor(s)
    return fl.astype(np.int64), ((s - fl) * _TWO32).astype(np.uint64)


def fx_step(hi, lo, inc_hi, inc_lo):
    """One step: the low words add modulo 2^32, the carry goes to the high word."""
    lo = lo + np.uint64(inc_lo)
    return hi + inc_hi + (lo >> np.uint64(32)).astype(np.int64), lo & np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------
# the planner
# ---------------------------------------------------------------------------------------------------
def extract_box_dims(m, T, halo2, params=PARAMS):
    """Staged box (Lz, Ly, Lx) of tile T under the 3x4 matrix m, or None when the extent is absurd."""
    L = []
    for r in range(3):
        ext = 0.0
        for k in range(3):
            ext += abs(float(m[r][k])) * (T[k] - 1)
        if not ext < 4096.0:
            return None
        L.append(int(np.floor(ext + params.extent_margin)) + 3 + halo2)
    L[2] = (L[2] + 3 + 3) & ~3
    return tuple(L)


def extract_pick_tile(cubic, box, params=PARAMS):
    """(index into TILES, workgroups per CU) of a (box shape, interpolation class) pair."""
    typical = [[0.5, 0.5, 0.5, 0.0]] * 3
    best, best_wg, best_cost = 0, 1, 1e300
    for cfg, T in enumerate(TILES):
        L = extract_box_dims(typical, T, 2 if cubic else 0, params)
        if L is None:
            continue
        nbytes = L[0] * L[1] * L[2] * 4
        wg = min(8, LDS_CAP // nbytes)
        tiles = 1.0
        for k in range(3):
            tiles *= (box[k] + T[k] - 1) // T[k]
        cost = nbytes * tiles / (float(box[0]) * box[1] * box[2]) * (1.0 if wg >= 3 else (1.25 if wg == 2 else 2.0))
        if cost < best_cost:
            best, best_wg, best_cost = cfg, wg, cost
    return best, best_wg


def extract_fill_entry(m, cfg, cubic, lds_cap=LDS_CAP, params=PARAMS):
    """dict(neg, pos, inc_hi, inc_lo, L, tiled) of one matrix: the ExtractEntry."""
    T = TILES[cfg]
    neg, pos, inc_hi, inc_lo = [], [], [], []
    for r in range(3):
        n = p = 0.0
        for k in range(3):
            x = float(m[r][k]) * (T[k] - 1)
            if x < 0:
                n += x
            else:
                p += x
        neg.append(n)
        pos.append(p)
        hi, lo = fx_inc(m[r][0])
        inc_hi.append(hi)
        inc_lo.append(lo)
    L = extract_box_dims(m, T, 2 if cubic else 0, params)
    tiled = L is not None and L[0] * L[1] * L[2] * 4 <= lds_cap
    return dict(neg=neg, pos=pos, inc_hi=inc_hi, inc_lo=inc_lo, L=L if tiled else None, tiled=tiled)


def project_batch_shape_plan(cubic, shape, params=PARAMS):
    """(cfg, segments, depth tiles per segment) of a projection stack's output shape."""
    cfg, _ = extract_pick_tile(cubic, shape, params)
    T = TILES[cfg]
    ntd = (shape[0] + T[0] - 1) // T[0]
    inplane = ((shape[1] + T[1] - 1) // T[1]) * ((shape[2] + T[2] - 1) // T[2])
    want = max(1, (1024 + inplane - 1) // inplane)
    seg = min(ntd, want)
    per = (ntd + seg - 1) // seg
    return cfg, (ntd + per - 1) // per, per


def segments_of(cubic, shape):
    return project_batch_shape_plan(cubic, shape)[1]


# ---------------------------------------------------------------------------------------------------
# the device chain
# ---------------------------------------------------------------------------------------------------
Result = collections.namedtuple('Result', 'cfg tile L lds_bytes tiled lo hi flat_lo flat_hi tiles staged whole one_below')


def _march(m, box, T, entry, cubic, src_shape, params, td_range):
    """Tap extremes over the depth tiles td_range of every in-plane tile.  Returns (lo[3], hi[3], flat_lo, flat_hi, tiles, staged tiles,
    whole tiles, voxels whose lowest tap is below the box)."""
    TD, TH, TW = T
    oD, oH, oW = box
    npos = TH * TW
    DG = 1 if npos >= 256 else 256 // npos
    DPT = TD // DG
    halo = 1 if cubic else 0
    Lz, Ly, Lx = entry['L']
    vlo = (-0.5, -0.5, -0.5)
    vhi = tuple(float(s) - 0.5 for s in src_shape) if src_shape is not None else None

    tds = np.asarray(list(td_range), np.int64)
    d0 = (tds * TD)[:, None, None]
    h0 = (np.arange((oH + TH - 1) // TH, dtype=np.int64) * TH)[None, :, None]
    w0 = (np.arange((oW + TW - 1) // TW, dtype=np.int64) * TW)[None, None, :]
    tshape = np.broadcast_shapes(d0.shape, h0.shape, w0.shape)
    any_valid = np.ones(tshape, bool)
    all_valid = np.ones(tshape, bool)
    o, b = [], []
    for r in range(3):
        base = _fma(m[r][0], d0, _fma(m[r][1], h0, _fma(m[r][2], w0, float(m[r][3]))))
        base = np.broadcast_to(base, tshape)
        lo = base + entry['neg'][r]
        hi = base + entry['pos'][r]
        if vhi is not None:
            any_valid &= (hi >= vlo[r] - TILE_MARGIN) & (lo < vhi[r] + TILE_MARGIN)
            all_valid &= (lo >= vlo[r] + TILE_MARGIN) & (hi < vhi[r] - TILE_MARGIN)
        orr = np.floor(lo - params.origin_margin).astype(np.int64) - halo
        if r == 2:
            orr &= ~np.int64(3)
        o.append(orr)
        b.append(base - orr.astype(np.float64))
    whole = all_valid & np.broadcast_to(oD - d0 >= TD, tshape)

    # columns: (lane group, tile row, tile column) of every tile
    g = np.arange(DG, dtype=np.int64)[:, None, None]
    j = np.arange(TH, dtype=np.int64)[None, :, None]
    kw = np.arange(TW, dtype=np.int64)[None, None, :]
    i0 = g * DPT
    T5 = tshape + (1, 1, 1)
    live = any_valid.reshape(T5) & ((h0.reshape(h0.shape + (1, 1, 1)) + j) < oH) & ((w0.reshape(w0.shape + (1, 1, 1)) + kw) < oW)
    # planes this column's thread samples: DPT on whole tiles, min(DPT, oD - d0 - i0) otherwise
    nd = np.where(whole.reshape(T5), DPT, np.clip(oD - d0.reshape(d0.shape + (1, 1, 1)) - i0, 0, DPT))
    full = np.broadcast_shapes(live.shape, nd.shape)
    live = np.broadcast_to(live, full)
    nd = np.broadcast_to(nd, full)
    c_hi, c_lo = [], []
    for r in range(3):
        s = _fma(m[r][0], i0, _fma(m[r][1], j, _fma(m[r][2], kw, b[r].reshape(T5))))
        s = np.broadcast_to(s, full)
        hi, lo = to_fx(s)
        c_hi.append(hi)
        c_lo.append(lo)
    ext_lo = [None] * 3
    ext_hi = [None] * 3
    flat_lo, flat_hi = None, None
    below = 0
    LyLx = Ly * Lx
    for i in range(DPT):
        act = live & (i < nd)
        if act.any():
            idx = [c[act] for c in c_hi]
            for r in range(3):
                a, z = int(idx[r].min()) - halo, int(idx[r].max()) + 1 + halo
                ext_lo[r] = a if ext_lo[r] is None else min(ext_lo[r], a)
                ext_hi[r] = z if ext_hi[r] is None else max(ext_hi[r], z)
            below += int(((idx[0] < halo) | (idx[1] < halo) | (idx[2] < halo)).sum())
            # the addresses actually read: the cubic gather fetches aligned pairs, one or two columns beyond the four taps
            if cubic:
                x1 = idx[2] - 1
                par = x1 & 1
                first = (idx[0] - 1) * LyLx + (idx[1] - 1) * Lx + (x1 - par)
                last = (idx[0] + 2) * LyLx + (idx[1] + 2) * Lx + (x1 - par) + np.where(par == 1, 5, 3)
            else:
                first = idx[0] * LyLx + idx[1] * Lx + idx[2]
                last = first + LyLx + Lx + 1
            fa, fz = int(first.min()), int(last.max())
            flat_lo = fa if flat_lo is None else min(flat_lo, fa)
            flat_hi = fz if flat_hi is None else max(flat_hi, fz)
        for r in range(3):
            c_hi[r], c_lo[r] = fx_step(c_hi[r], c_lo[r], entry['inc_hi'][r], entry['inc_lo'][r])
    return ext_lo, ext_hi, flat_lo, flat_hi, int(np.prod(tshape)), int(any_valid.sum()), int(whole.sum()), below


def _merge(parts):
    lo, hi = [None] * 3, [None] * 3
    flo = fhi = None
    tiles = staged = whole = below = 0
    for plo, phi, pflo, pfhi, t, s, w, bl in parts:
        tiles, staged, whole, below = tiles + t, staged + s, whole + w, below + bl
        if pflo is None:
            continue
        for r in range(3):
            lo[r] = plo[r] if lo[r] is None else min(lo[r], plo[r])
            hi[r] = phi[r] if hi[r] is None else max(hi[r], phi[r])
        flo = pflo if flo is None else min(flo, pflo)
        fhi = pfhi if fhi is None else max(fhi, pfhi)
    return lo, hi, flo, fhi, tiles, staged, whole, below


def model(m, box, interp, src_shape=None, cfg=None, params=PARAMS, project=False):
    """Tap extremes of kernels 11 and 13-16 (project=False) or of kernel 12 (project=True: `box` is the output shape, marched segment
    by segment) for one pull matrix.  `src_shape` gives the valid interval (tiles that clear it are never staged; None: stage all);
    `cfg` overrides the planner's tile.  lo / hi are None when nothing is staged."""
    m = np.asarray(m, np.float64)
    cubic = is_cubic(interp)
    box = tuple(int(x) for x in box)
    picked = extract_pick_tile(cubic, box, params)[0]
    cfg = picked if cfg is None else cfg
    T = TILES[cfg]
    entry = extract_fill_entry(m, cfg, cubic, LDS_CAP, params)
    if not entry['tiled']:
        return Result(cfg, T, None, 0, False, None, None, None, None, 0, 0, 0, 0)
    ntd = (box[0] + T[0] - 1) // T[0]
    if project:
        _, nseg, per = project_batch_shape_plan(cubic, box, params)
        ranges = [range(s * per, min(s * per + per, ntd)) for s in range(nseg)]
    else:
        ranges = [range(ntd)]
    lo, hi, flo, fhi, tiles, staged, whole, below = _merge([_march(m, box, T, entry, cubic, src_shape, params, r) for r in ranges])
    L = entry['L']
    return Result(cfg, T, L, L[0] * L[1] * L[2] * 4, True, lo if flo is not None else None, hi if flo is not None else None, flo, fhi,
                  tiles, staged, whole, below)


def violations(res):
    """The axes on which a tap leaves [0, L), as (axis, lowest, highest, L); plus ('flat', ...) when an address that is actually read
    leaves the staged box."""
    out = []
    if not res.tiled or res.lo is None:
        return out
    for r in range(3):
        if res.lo[r] < 0 or res.hi[r] >= res.L[r]:
            out.append((r, res.lo[r], res.hi[r], res.L[r]))
    if res.flat_lo < 0 or res.flat_hi >= res.L[0] * res.L[1] * res.L[2]:
        out.append(('flat', res.flat_lo, res.flat_hi, res.L[0] * res.L[1] * res.L[2]))
    return out


# ---------------------------------------------------------------------------------------------------
# what two wrong kernels would do (CPU arguments for tests/test_gpu_box_lattice.py: no broken kernel is ever run)
# ---------------------------------------------------------------------------------------------------
def fx_source_coords(m, box, cfg, cubic=False, params=PARAMS):
    """Per voxel of the box and source axis the coordinate the taps are formed from, as exact (integer part, units of 2^-32) pairs in
    SOURCE coordinates: origin + Fx.hi, Fx.lo.  Every tile, whether or not it meets the valid interval."""
    m = np.asarray(m, np.float64)
    T = TILES[cfg]
    TD, TH, TW = T
    entry = extract_fill_entry(m, cfg, cubic, 1 << 40, params)
    DG = 1 if TH * TW >= 256 else 256 // (TH * TW)
    DPT = TD // DG
    halo = 1 if cubic else 0
    hi_out = np.zeros((3,) + tuple(box), np.int64)
    lo_out = np.zeros((3,) + tuple(box), np.int64)
    for d0 in range(0, box[0], TD):
        for h0 in range(0, box[1], TH):
            for w0 in range(0, box[2], TW):
                j = np.arange(min(TH, box[1] - h0), dtype=np.int64)[:, None]
                kw = np.arange(min(TW, box[2] - w0), dtype=np.int64)[None, :]
                for r in range(3):
                    base = float(_fma(m[r][0], d0, _fma(m[r][1], h0, _fma(m[r][2], w0, float(m[r][3])))))
                    o = int(np.floor(base + entry['neg'][r] - params.origin_margin)) - halo
                    if r == 2:
                        o &= ~3
                    b = base - float(o)
                    for g in range(DG):
                        i0 = g * DPT
                        s = np.broadcast_to(_fma(m[r][0], i0, _fma(m[r][1], j, _fma(m[r][2], kw, b))), (j.shape[0], kw.shape[1]))
                        fl = np.floor(s)
                        chi = fl.astype(np.int64)
                        clo = ((s - fl) * _TWO32).astype(np.int64)
                        for i in range(DPT):
                            d = d0 + i0 + i
                            if d < box[0]:
                                hi_out[r, d, h0:h0 + j.shape[0], w0:w0 + kw.shape[1]] = chi + o
                                lo_out[r, d, h0:h0 + j.shape[0], w0:w0 + kw.shape[1]] = clo
                            clo = clo + entry['inc_lo'][r]
                            chi = chi + entry['inc_hi'][r] + (clo >> 32)
                            clo = clo & 0xFFFFFFFF
    return hi_out, lo_out


def inside_by_fixed_point(m, box, cfg, src_shape, cubic=False):
    """The inside mask a kernel would get that tested its Q32.32 coordinate (exact comparison with -0.5 and dim - 0.5) instead of the
    canonical float64 chain."""
    hi, lo = fx_source_coords(m, box, cfg, cubic)
    ins = np.ones(tuple(box), bool)
    half = 1 << 31
    for r in range(3):
        ins &= (hi[r] > -1) | ((hi[r] == -1) & (lo[r] >= half))                                     # s >= -0.5
        ins &= (hi[r] < src_shape[r] - 1) | ((hi[r] == src_shape[r] - 1) & (lo[r] < half))          # s < dim - 0.5
    return ins


def tiles_whole_without_margin(m, box, cfg, src_shape):
    """[(d0, h0, w0)]: depth-complete tiles whose float64 bounding box lies inside the valid interval by a bare comparison (no
    kTileMargin) -- a kernel that called them whole would skip the per-voxel test there."""
    m = np.asarray(m, np.float64)
    T = TILES[cfg]
    entry = extract_fill_entry(m, cfg, False)
    out = []
    for d0 in range(0, box[0] - T[0] + 1, T[0]):
        for h0 in range(0, box[1], T[1]):
            for w0 in range(0, box[2], T[2]):
                ok = True
                for r in range(3):
                    base = float(_fma(m[r][0], d0, _fma(m[r][1], h0, _fma(m[r][2], w0, float(m[r][3])))))
                    ok = ok and base + entry['neg'][r] >= -0.5 and base + entry['pos'][r] < src_shape[r] - 0.5
                if ok:
                    out.append((d0, h0, w0))
    return out


def whole_margin_cases(shape, box, cfg):
    """Cases aimed at kTileMargin, as (name, m64, traits) in the form of lattice_cases.box_cases: 3-4-5 and thirds parts placed so that a
    corner voxel of the first tile sits on a face in exact arithmetic.  Kept are those where the tile's float64 bounding box (base +
    reach) says "inside" by a bare comparison while the canonical chain puts a voxel of that tile outside -- the two differ by an ulp
    about the cut.  The margin sends such a tile through the per-voxel test; without it the voxel would come out sampled."""
    import itertools
    import lattice_cases as lc
    parts = lc.linear_parts()
    T = TILES[cfg]
    cb = lc.box_centre_of(box, 'half')
    pos = np.floor((np.asarray(shape, np.float64) - 1.0) / 2.0) + 0.5
    out = []
    for label, L in parts['rot345'] + parts['thirds']:
        for r in range(3):
            for side in ('lo', 'hi'):
                for corner in itertools.product(*[(0, min(T[k], box[k]) - 1) for k in range(3)]):
                    t = pos - L @ cb
                    t[r] = (-0.5 if side == 'lo' else shape[r] - 0.5) - float(L[r] @ np.asarray(corner, np.float64))
                    m = np.eye(4)
                    m[:3, :3] = L
                    m[:3, 3] = t
                    s = lc.chain_coords(m, box)
                    ins = np.ones(tuple(box), bool)
                    for a in range(3):
                        ins &= (s[a] >= -0.5) & (s[a] < shape[a] - 0.5)
                    fooled = sum(int((~ins[d0:d0 + T[0], h0:h0 + T[1], w0:w0 + T[2]]).sum())
                                 for d0, h0, w0 in tiles_whole_without_margin(m, box, cfg, shape))
                    if fooled:
                        face = tuple((side, 0) if a == r else None for a in range(3))
                        traits = dict(index=len(out), group='face_chain', cls='thirds' if label.startswith('thirds') else 'rot345',
                                      family=lc.structure(L), exact=False, f32=False, eps=(0.0, 0.0, 0.0), eps_mag=0.0, eps_axes=(r,),
                                      eps_axis=r, eps_sign=0, share={r: 1.0 / lc.lattice_period(L[r])}, face=face, centre='half',
                                      base=(0, 0, 0), whole=False, fooled=fooled)
                        out.append(('margin%02d_%s_ax%d%s' % (len(out), label, r, side), m, traits))
    return out
