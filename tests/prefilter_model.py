"""Host model of the B-spline prefilter (voltools_amd/csrc/vt_kernels_prefilter.hip): plain numpy, no GPU, no pytest.

Two things live here.

`prefilter_f64` is the reference's recursion (bspline.h:2-54) along axes 2, 1, 0 in float64 -- the true coefficients that the float32
oracle and the kernels both approximate.  Distances to it are quoted in the unit u = 2^-23 * max|c64| (`unit`): the error of a float32
recursion follows the coefficient amplitude, not the data's, so a bound in u holds for unit-range and for signed, scaled data alike.

`route` repeats the dispatch (`run_prefilter` in vt_api.hip; `prefilter_xy_ok`, `prefilter_axis_in_place_ok`, `prefilter_chunk_size`,
`launch_prefilter_axis`, `launch_prefilter_xy` in vt_kernels_prefilter.hip) and says which kernel form serves every pass of a shape,
with how many segments, in place or ping-pong, and which buffer holds the result.  tests/test_prefilter_model.py reads the constants
below out of the sources and routes the case list of tests/test_gpu_prefilter.py through it, so a dispatch change that drops a kernel
form out of the suite fails there.
"""
import collections

import numpy as np

# ---- constants of vt_kernels_prefilter.hip / vt_host.h (compared with the sources by tests/test_prefilter_model.py) ----
K_CHUNK = 64                                  # kChunk: default chunk of the strided passes
K_WARM = 16                                   # kWarm: warm-up samples on each side of a chunk
CHUNK_SIZES = (32, 64, 128)                   # prefilter_chunked<C, kWarm> instantiations
CHUNK_128_FROM = 256                          # lines of >= 256 samples use chunks of 128
BLK_K = 16                                    # kBlkK: warm-up at interior segment ends of the block form
BLK_VARIANTS = {0: (16, 18), 1: (8, 20), 2: (8, 18)}      # VT_PF_BLOCK -> (NW, CW)
BLK_MIN_N = 40                                # block form: lines of >= 40 samples
XY_NW, XY_CW, XY_K = 16, 10, 16               # kXyNW, kXyCW, kXyK
XY_COLS = 512                                 # kXyCols
XY_MIN_W, XY_MIN_H = 64, 40                   # prefilter_xy_ok
X_REG_MAX_W = 2048                            # widest line the X pass holds in registers
IN_PLACE_MAX_N = 32                           # strided lines this short are filtered in place
X_SCAN_NSEG = (1, 2, 4, 8, 16, 32)            # prefilter_x_scan<NSEG>: segments of 64
X_SCAN4_NSEG = (1, 2, 4, 8)                   # prefilter_x_scan4<NSEG>: segments of 256
HORIZON = 12                                  # samples of the causal initialisation

XY_ROWS = XY_NW * XY_CW                       # 160 loaded
XY_NET_ROWS = XY_ROWS - 2 * XY_K              # 128 written
XY_NET_COLS = XY_COLS - 2 * XY_K              # 480 written

Z = np.sqrt(3.0) - 2.0
LAMBDA = (1.0 - Z) * (1.0 - 1.0 / Z)


def resident_pitch(W):
    return (W + 4 + 31) & ~31


# ---------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------
def _filter_axis(c, axis, lo_interior):
    """bspline.h:30-54 along one axis of a float64 array, vectorised across lines."""
    v = np.moveaxis(c, axis, 0)
    n = v.shape[0]
    if lo_interior:
        v[0] = LAMBDA * v[0] / (1.0 - Z)
    else:
        acc = v[0].copy()
        for k in range(min(HORIZON, n)):
            acc += Z ** (k + 1) * v[k]
        v[0] = LAMBDA * acc
    for k in range(1, n):
        v[k] = LAMBDA * v[k] + Z * v[k - 1]
    v[n - 1] = Z / (Z - 1.0) * v[n - 1]
    for k in range(n - 2, -1, -1):
        v[k] = Z * (v[k + 1] - v[k])


def prefilter_f64(vol, lo_interior_axis0=False):
    """Coefficients of `vol` (1-D to 3-D; the last axis is filtered first) in float64.  `lo_interior_axis0` replaces the causal start
    of axis 0 by lambda * s0 / (1 - z), the steady-state start the kernels use for a slab whose first plane is interior."""
    c = np.array(vol, dtype=np.float64)
    for axis in range(c.ndim - 1, -1, -1):
        _filter_axis(c, axis, lo_interior_axis0 and axis == 0 and c.ndim == 3)
    return c


def unit(c64):
    """u = 2^-23 * max|c64|: one float32 ulp at the largest coefficient."""
    return 2.0 ** -23 * float(np.abs(c64).max())


# ---------------------------------------------------------------------------------------------------
# the dispatch
# ---------------------------------------------------------------------------------------------------
# form: 'x_scan' | 'x_scan4' | 'chunked' | 'block' | 'xy';  param: the template parameter(s)
# N: line length;  nseg: segments / chunks along the line (xy: (row segments, column segments));  last: samples of the last one
#   (xy: (rows, columns));  seg: samples a full segment writes
# lanes: extent of the lane axis (x_scan*: lines);  in_place: src == dst;  src / dst: 'a' the caller's buffer, 'b' the partner
# lo_interior: steady-state causal start (axis 0 of a slab window whose first plane is interior)
# wmod4: W % 4 (the block form zeroes the pad columns of the last vector);  ncb: column blocks of 256 (block form)
# cuts: positions along the line where a segment, a chunk or a wave's share starts (xy: (row cuts, column cuts))
Pass = collections.namedtuple('Pass', 'axis form param N nseg last seg lanes in_place src dst lo_interior wmod4 ncb cuts')
Route = collections.namedtuple('Route', 'passes result')     # result: the buffer that holds the coefficients ('a' | 'b')


def chunk_size(N, env):
    variant = int(env['VT_PF_CHUNK']) if 'VT_PF_CHUNK' in env else (128 if N >= CHUNK_128_FROM else K_CHUNK)
    return 128 if variant == 128 else (32 if variant == 32 else K_CHUNK)


def xy_ok(D, H, W, pitch, aligned16, env):
    if not aligned16 or 'VT_PF_NO_XY' in env:
        return False
    return W >= XY_MIN_W and H >= XY_MIN_H and pitch % 4 == 0 and pitch >= ((W + 7) & ~7)


def in_place_ok(axis, D, H, W):
    if axis == 2:
        return W <= X_REG_MAX_W
    return (D if axis == 0 else H) <= IN_PLACE_MAX_N


def _pick(nseg, sizes):
    for s in sizes:
        if nseg <= s:
            return s
    return sizes[-1]


def _block_cuts(N, nw, cw):
    seg = nw * cw - 2 * BLK_K
    cuts = set()
    for s in range((N + seg - 1) // seg):
        a0 = s * seg
        b0 = min(a0 + seg, N)
        la = a0 - BLK_K if s > 0 else 0
        lb = min(b0 + (BLK_K if b0 < N else 0), N)
        cuts.add(a0)
        cuts.update(p for p in range(la, lb, cw))
    return sorted(p for p in cuts if 0 < p < N)


def _axis_pass(axis, D, H, W, pitch, aligned16, in_place, src, dst, lo_interior, env):
    vec_rows = aligned16 and pitch % 4 == 0 and pitch >= ((W + 3) & ~3)
    common = dict(axis=axis, in_place=in_place, src=src, dst=dst, lo_interior=lo_interior, wmod4=W % 4, ncb=0)
    if axis == 2 and W <= X_REG_MAX_W:
        step, sizes, form = (256, X_SCAN4_NSEG, 'x_scan4') if vec_rows else (64, X_SCAN_NSEG, 'x_scan')
        nseg = (W + step - 1) // step
        return Pass(form=form, param=_pick(nseg, sizes), N=W, nseg=nseg, last=W - (nseg - 1) * step, seg=step, lanes=D * H,
                    cuts=list(range(step, W, step)), **common)
    N = (D, H, W)[axis]
    if 'VT_PF_NO_BLOCK' not in env and axis != 2 and not in_place and vec_rows and N >= BLK_MIN_N:
        nw, cw = BLK_VARIANTS.get(int(env.get('VT_PF_BLOCK', 0)), BLK_VARIANTS[0])
        seg = nw * cw - 2 * BLK_K
        nseg = (N + seg - 1) // seg
        common['ncb'] = (((W + 3) & ~3) // 4 + 63) // 64
        return Pass(form='block', param=(nw, cw), N=N, nseg=nseg, last=N - (nseg - 1) * seg, seg=seg, lanes=W,
                    cuts=_block_cuts(N, nw, cw), **common)
    C = chunk_size(N, env)
    nseg = (N + C - 1) // C
    return Pass(form='chunked', param=C, N=N, nseg=nseg, last=N - (nseg - 1) * C, seg=C, lanes=H if axis == 2 else W,
                cuts=list(range(C, N, C)), **common)


def _xy_pass(H, W, src, dst):
    nsy = 1 if H <= XY_ROWS else (H + XY_NET_ROWS - 1) // XY_NET_ROWS
    nsx = 1 if W <= XY_COLS else (W + XY_NET_COLS - 1) // XY_NET_COLS
    rows, cols = set(), set()
    for sy in range(nsy):
        ra = 0 if nsy == 1 else sy * XY_NET_ROWS
        rb = H if nsy == 1 else min(ra + XY_NET_ROWS, H)
        lra = 0 if nsy == 1 else max(ra - XY_K, 0)
        lrb = H if nsy == 1 else min(rb + XY_K, H)
        rows.add(ra)
        rows.update(range(lra, lrb, XY_CW))
    for sx in range(nsx):
        na = 0 if nsx == 1 else sx * XY_NET_COLS
        la = 0 if nsx == 1 else max(na - XY_K, 0)
        cols.update((na, la, la + 8, la + 16))                # the segment, its first loaded column, the first two lane shares
    last = (H if nsy == 1 else H - (nsy - 1) * XY_NET_ROWS, W if nsx == 1 else W - (nsx - 1) * XY_NET_COLS)
    return Pass(axis=(2, 1), form='xy', param=(XY_NW, XY_CW), N=(H, W), nseg=(nsy, nsx), last=last, seg=(XY_NET_ROWS, XY_NET_COLS),
                lanes=W, in_place=False, src=src, dst=dst, lo_interior=False, wmod4=W % 4, ncb=0,
                cuts=(sorted(p for p in rows if 0 < p < H), sorted(p for p in cols if 0 < p < W)))


def route(D, H, W, pitch, aligned16, lo_interior=False, env=None):
    """The passes `run_prefilter` launches for a (D, H, W) volume whose rows are `pitch` floats apart, and the buffer that holds the
    result.  `aligned16`: both buffers start on a 16-byte boundary.  `env`: the VT_PF_* knobs that are set."""
    env = env or {}
    cur, oth = 'a', 'b'
    passes = []
    axes = (2, 1, 0)
    if xy_ok(D, H, W, pitch, aligned16, env):
        passes.append(_xy_pass(H, W, cur, oth))
        cur, oth = oth, cur
        axes = (0,)
    for axis in axes:
        interior = lo_interior and axis == 0
        if in_place_ok(axis, D, H, W):
            passes.append(_axis_pass(axis, D, H, W, pitch, aligned16, True, cur, cur, interior, env))
        else:
            passes.append(_axis_pass(axis, D, H, W, pitch, aligned16, False, cur, oth, interior, env))
            cur, oth = oth, cur
    return Route(passes, cur)


def route_dense(shape, aligned16=True, env=None):
    """`vt_prefilter_inplace`: pitch = W; a result in 'b' is copied back to the caller's buffer."""
    D, H, W = shape
    return route(D, H, W, W, aligned16, False, env)


def route_resident(shape, lo_interior=False, env=None):
    """A resident handle: pitch = resident_pitch(W), aligned buffers; a result in 'b' makes `finalize_resident` swap the buffers."""
    D, H, W = shape
    return route(D, H, W, resident_pitch(W), True, lo_interior, env)


ONESHOT_MIN_BYTES = 32 << 20


def route_oneshot(shape, separable=True, env=None):
    """The pipelined one-shot call on a filt_* volume (`pipeline_eligible` / `oneshot_pipelined` in vt_api.hip): X and Y per uploaded
    chunk of planes, then `launch_prefilter_axis0_chunks` -- always the chunked form, out of place.  Returns None when the call does
    not qualify and takes the resident route."""
    env = env or {}
    D, H, W = shape
    nbytes = D * H * W * 4
    if nbytes < ONESHOT_MIN_BYTES or D < 32 or W > X_REG_MAX_W or in_place_ok(1, D, H, W) or in_place_ok(0, D, H, W):
        return None
    if not separable and nbytes < (256 << 20):
        return None
    pitch = resident_pitch(W)
    if xy_ok(D, H, W, pitch, True, env):
        passes = [_xy_pass(H, W, 'a', 'b')]
    else:
        passes = [_axis_pass(2, D, H, W, pitch, True, True, 'a', 'a', False, env),
                  _axis_pass(1, D, H, W, pitch, True, False, 'a', 'b', False, env)]
    C = chunk_size(D, env)
    nseg = (D + C - 1) // C
    passes.append(Pass(axis=0, form='chunked', param=C, N=D, nseg=nseg, last=D - (nseg - 1) * C, seg=C, lanes=W, in_place=False,
                       src='b', dst='a', lo_interior=False, wmod4=W % 4, ncb=0, cuts=list(range(C, D, C))))
    return Route(passes, 'a')


def forms(r):
    """The (form, template parameter) pairs of a route."""
    return [(p.form, p.param) for p in r.passes]


def all_default_forms():
    """Every (form, template parameter) the dispatch can produce with no knob set."""
    return ([('x_scan', n) for n in X_SCAN_NSEG] + [('x_scan4', n) for n in X_SCAN4_NSEG] + [('chunked', 64), ('chunked', 128)] +
            [('block', BLK_VARIANTS[0]), ('xy', (XY_NW, XY_CW))])


def impulse_positions(r, shape):
    """Voxels on both sides of every cut of every pass of a route: the places where a carry handed to the wrong neighbour shows."""
    pts = set()
    mid = [s // 2 for s in shape]
    k = 0
    for p in r.passes:
        pairs = [(p.axis, p.cuts)] if p.form != 'xy' else [(1, p.cuts[0]), (2, p.cuts[1])]
        for axis, cuts in pairs:
            for c in cuts:
                for pos in (c - 1, c):
                    idx = [(mid[a] + k) % shape[a] for a in range(3)]    # spread over the other axes' lines
                    idx[axis] = pos
                    pts.add(tuple(idx))
                    k += 1
    if not pts:
        pts.add(tuple(mid))
    return sorted(pts)
