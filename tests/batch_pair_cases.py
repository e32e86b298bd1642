"""Cases of tests/test_gpu_batch_pairs.py: every ordered pair of the sixteen batched entry points as neighbours on ONE handle.

The batched calls of a handle share the host staging vector (reinterpreted per family), its device copy (grown, never shrunk), the
float64 partial sums (freed and reallocated when too small) and the result staging buffer.  This module holds, per family, a pool of
concrete calls with fixed, seeded arguments (a Variant: a closure on the handle plus what the host can tell about it without one -- the
length of its table in doubles, the bytes of partials it asks for, its output kind), an Eulerian circuit of the complete directed graph
on the families (self-loops included: F^2 + 1 steps, every ordered pair adjacent exactly once), and the seeded draw of a variant per
step, patched until the adjacencies listed in REQUIRED hold.  tests/test_batch_pair_cases_host.py holds the draw to them.

The volume is (6, 97, 151), seeded standard normal, and serves the 3-D calls and the stack calls alike.  (6, 97, 150) would do for all
but one condition: correlate_stack takes references of the images' own shape, n x 97 x 150 floats is even for every n, and an odd count
(half a stale double at the end of the staging vector) needs an odd H x W; 151 is the next width.  correlate_stack_model.plan(97, 151, .,
(1, 1)) still gives 2 x 3 pieces, asserted below.

boxes, weights, field, DeviceF64 and run are those of tests/test_gpu_batch_sequences.py; its places, backproject and projection
builders have that file's (20, 22, 24) volume built in (plane indices up to 19, the map's centre), so their counterparts here are written
for this volume.  Importing that file imports pytest and the package; nothing here needs a GPU until a step runs on a GPU handle.

A refusal that comes after the staging vector was resized and partly written: vt_volume_warp_stack checks, ranges and copies the grids
in one pass, so a NaN node far from the start is found with the entries' grids before it already copied.  StaticVolume.warp_stack
refuses such a grid itself (ValueError) before the library sees it, so on a GPU handle the step calls the C entry point with the
arguments the method would pass and raises ValueError with the library's text; on device='cpu' it is the method's own refusal.  The
other refusal behind begin_tables in vt_api.hip, warp's "the launch needs N bytes of LDS", cannot be reached: warp_plan gathers a tile
whose box does not fit."""
import functools

import numpy as np

import voltools_amd as vt
from voltools_amd import _native

import box_index_model as bim
import correlate_stack_model as csm
import moments_stack_model as msm
import test_gpu_batch_sequences as seq
from test_gpu_batch_sequences import boxes, weights, field, DeviceF64, run, BOX, OUT

VOLUME = (6, 97, 151)
T, H, W = VOLUME
IMG = (37, 45)                       # a stack output with cut 16 x 16 tiles on both axes
IMG_SMALL = (21, 33)
PREFILL = -7.0                       # run()'s host prefill; device outputs of the walk are prefilled with it too
DEFAULT_CAP = 64 << 20               # VT_DOT_PART_CAP's default
ENTRY = 24                           # sizeof(ExtractEntry) / 8
WARP_TABLE, WARP_STACK_HEADER, FILTER_ENTRY, FILTER_CHUNK = 34, 6, 4, 128
SMALL_TABLE, LARGE_TABLE = 40, 900   # doubles: one entry of any family; forty entries of the three-dimensional ones
SUM_MULTI_CHUNK = (2, 4, 8)          # sum_multi_chunk(cfg)

assert (H * W) % 2 == 1
assert (csm.plan(H, W, (2, 7), (1, 1))['pieces_y'], csm.plan(H, W, (2, 7), (1, 1))['pieces_x']) == (2, 3)


def volume():
    v = np.random.default_rng(97151).standard_normal(VOLUME).astype(np.float32)
    v.setflags(write=False)
    return v


def rng_of(seed):
    return np.random.default_rng(seq.RNG_SEED + seed)


# ---- what the host can tell about a call -------------------------------------------------------------------------------------------
def box_tiles(cubic, box):
    cfg, _ = bim.extract_pick_tile(cubic, box)
    return cfg, int(np.prod([-(-b // t) for b, t in zip(box, bim.TILES[cfg])]))


def sum_segments(cubic, box, n):
    """extract_sum_shape_plan's segments."""
    _, tiles = box_tiles(cubic, box)
    seg = max(1, min(n, max(1, (1024 + tiles - 1) // tiles)))
    per = (n + seg - 1) // seg
    return (n + per - 1) // per


class Variant:
    """One concrete call.  call(sv, out) fills `out`; table: doubles of the staging vector; partials(cubic, cap): bytes of float64
    partial sums asked for; truth(got, vol, interp, tol): the family's float64 model and bound (tol: its suite's TOL), or None."""

    def __init__(self, family, tag, call, shape, device, table, f64=False, base=None, partials=None, truth=None, refusal=False,
                 late_refusal=False, odd_refs=False):
        self.family, self.tag, self.call, self.shape, self.device, self.table = family, tag, call, tuple(shape), device, int(table)
        self.f64, self.base, self.truth, self.refusal, self.late_refusal, self.odd_refs = f64, base, truth, refusal, late_refusal, odd_refs
        self.accumulate = base is not None
        self._partials, self._memo = partials, {}
        self.name = f'{family}[{tag},{"device" if device else "host"}]'

    def __repr__(self):
        return self.name

    def partial_bytes(self, cubic=False, cap=DEFAULT_CAP):
        if (cubic, cap) not in self._memo:
            self._memo[cubic, cap] = 0 if self._partials is None else int(self._partials(cubic, cap))
        return self._memo[cubic, cap]

    def refuse(self, sv):
        """The text of the refusal; AssertionError if the call is served."""
        out = np.full(self.shape, PREFILL, np.float64 if self.f64 else np.float32)
        try:
            self.call(sv, out)
        except ValueError as e:
            assert (out == PREFILL).all(), self.name            # a refused call writes nothing
            return str(e)
        raise AssertionError(f'{self.name} was not refused')

    def launch(self, sv, device=None):
        """Make the call; returns fetch() -> the numpy result (a refusal: its text).  A device output is read, and freed, by fetch."""
        if self.refusal:
            msg = self.refuse(sv)
            return lambda: msg
        if not (self.device if device is None else device):
            res = run(lambda o: self.call(sv, o), self.shape, False, self.base, self.f64)
            return lambda: res
        if self.f64:
            out = DeviceF64(self.shape)
            out.buf.set(np.full(self.shape, PREFILL, np.float64).view(np.float32).reshape(-1))
        else:
            out = _native.DeviceArray.from_numpy(self.base if self.base is not None else np.full(self.shape, PREFILL, np.float32))
        self.call(sv, out)

        def fetch():
            res = out.get()
            (out.buf if self.f64 else out).free()
            return res
        return fetch

    def step(self, sv):
        return self.launch(sv)()


# ---- the three-dimensional families (kinds 1, 11-17) -------------------------------------------------------------------------------
def affine_batch(n, seed, device):
    rng = rng_of(seed)
    center = np.divide(np.subtract(VOLUME, 1), 2, dtype=np.float32)
    ms = np.stack([vt.utils.transform_matrix(rotation=tuple(rng.uniform(-180.0, 180.0, 3)), rotation_order='rzxz',
                                             translation=tuple(rng.uniform(-2.0, 2.0, 3)), center=center) for _ in range(n)])
    return Variant('affine_batch', f'n={n}', lambda sv, o: sv.affine_batch(ms, output=o), (n,) + VOLUME, device, 12 * n)


def extract(n, seed, device):
    ms = boxes(n, seed)
    return Variant('extract', f'n={n}', lambda sv, o: sv.extract(ms, BOX, output=o), (n,) + BOX, device, ENTRY * n)


def extract_sum(n, seed, device, w=True):
    ms, ws = boxes(n, seed), weights(n, seed) if w else None

    def partials(cubic, cap):
        nseg = sum_segments(cubic, BOX, n)
        return nseg * int(np.prod(BOX)) * 8 if nseg > 1 else 0
    return Variant('extract_sum', f'n={n}', lambda sv, o: sv.extract_sum(ms, BOX, ws, output=o), BOX, device, (ENTRY + 1) * n, partials=partials)


def extract_sum_multi(n, g, seed, device):
    ms, ws = boxes(n, seed), weights((n, g), seed)

    def partials(cubic, cap):
        nseg, n_box = sum_segments(cubic, BOX, n), int(np.prod(BOX))
        if nseg == 1:
            return 0
        gc = SUM_MULTI_CHUNK[box_tiles(cubic, BOX)[0]]
        chunks = max(1, min(-(-g // gc), cap // (gc * nseg * n_box * 8)))
        return min(g, chunks * gc) * nseg * n_box * 8
    return Variant('extract_sum_multi', f'n={n},g={g}', lambda sv, o: sv.extract_sum_multi(ms, BOX, ws, output=o), (g,) + BOX, device,
                   ENTRY * n + n * g + 8, partials=partials)


def _dot_partials(n, cols):
    def partials(cubic, cap):
        one = box_tiles(cubic, BOX)[1] * cols * 8
        return max(1, min(n, cap // one)) * one
    return partials


def _box_doubles(k=1):
    return (k * int(np.prod(BOX)) + 3) // 4 * 2


def extract_dot(n, seed, device, mask=False):
    ms, t, k = boxes(n, seed), field(BOX, seed), np.abs(field(BOX, seed + 1)) if mask else None
    return Variant('extract_dot', f'n={n}{",mask" if mask else ""}', lambda sv, o: sv.extract_dot(ms, t, k, output=o), (n, 3), device,
                   ENTRY * n + _box_doubles() * (2 if mask else 1), f64=True, partials=_dot_partials(n, 3))


def extract_dot_multi(n, k, seed, device, mask=False):
    ms, t, mk = boxes(n, seed), field((k,) + BOX, seed), np.abs(field(BOX, seed + 1)) if mask else None
    return Variant('extract_dot_multi', f'n={n},k={k}{",mask" if mask else ""}', lambda sv, o: sv.extract_dot_multi(ms, t, mk, output=o),
                   (n, 2 + k), device, ENTRY * n + _box_doubles(k) + (_box_doubles() if mask else 0), f64=True, partials=_dot_partials(n, 2 + k))


def projection_batch(n, shape, seed, device):
    assert max(shape) <= 64                                           # the fused route (kind 12) on every interpolation
    ms = vt.utils.tilt_matrices(rng_of(seed).uniform(-60.0, 60.0, n), 1, shape)
    ms[:, :3, 3] += (np.subtract(VOLUME, 1) / 2 - np.subtract(shape, 1) / 2)[None]      # about the centre of this volume
    n2 = shape[1] * shape[2]

    def partials(cubic, cap):
        nseg = bim.segments_of(cubic, shape)
        if nseg == 1:
            return 0
        image = nseg * n2 * 8
        return image * min(n, max(shape[0] * n2 * 4, image) // image)
    return Variant('projection_batch', f'n={n},{"x".join(map(str, shape))}', lambda sv, o: sv.projection_batch(ms, shape, output=o),
                   (n,) + tuple(shape[1:]), device, ENTRY * n, partials=partials)


def place(n, seed, device, accumulate=False, outside=False):
    rng = rng_of(seed)
    pos = rng.uniform(2.0, 11.0, (n, 3))
    pos[0] = (0.5, 13.0, 1.25)                                        # hangs over two faces of the output
    ms, ws = vt.utils.place_matrices(pos, rng.uniform(-180.0, 180.0, (n, 3)), VOLUME), weights(n, seed)
    if outside:                                                       # no copy can land anywhere: with accumulate nothing is launched
        ms[:, :3, 3] += 1000.0
    base = field(OUT, seed + 2) if accumulate else None
    tag = f'n={n}{",outside" if outside else ""}{",accumulate" if accumulate else ""}'
    return Variant('place', tag, lambda sv, o: sv.place(ms, OUT, ws, output=o, accumulate=accumulate), OUT, device, (ENTRY + 1) * n, base=base)


# ---- the back-projection pair (kinds 18, 19) ----------------------------------------------------------------------------------------
def backproject(n, seed, device, accumulate=False):
    rng = rng_of(seed)
    ms = vt.utils.backproject_matrices(rng.uniform(-60.0, 60.0, n), 1, OUT, VOLUME)
    planes = None if n == T else rng.integers(0, T, n)
    ws, base = weights(n, seed), field(OUT, seed + 2) if accumulate else None
    return Variant('backproject', f'n={n}{",accumulate" if accumulate else ""}',
                   lambda sv, o: sv.backproject(ms, OUT, ws, output=o, planes=planes, accumulate=accumulate), OUT, device, (ENTRY + 1) * n, base=base)


def backproject_boxes(nb, n, seed, device, accumulate=False):
    rng = rng_of(seed)
    ms = np.stack([vt.utils.backproject_matrices(rng.uniform(-60.0, 60.0, n), 1, BOX, VOLUME) for _ in range(nb)])
    shift = rng.uniform(-30.0, 30.0, (nb, 1, 2))
    shift[0] = (2.0 - H / 2, 5.0)                                     # box 0 hangs over the images' low edge
    ms[:, :, 1:3, 3] += shift
    planes = rng.integers(0, T, n)
    ws, base = weights((nb, n), seed), field((nb,) + BOX, seed + 2) if accumulate else None
    return Variant('backproject_boxes', f'{nb}x{n}{",accumulate" if accumulate else ""}',
                   lambda sv, o: sv.backproject_boxes(ms, BOX, ws, output=o, planes=planes, accumulate=accumulate), (nb,) + BOX, device,
                   (ENTRY + 1) * nb * n, base=base)


# ---- warp (kind 20) -----------------------------------------------------------------------------------------------------------------
def warp(grid_shape, out, seed, device, amp=1.5, f32=False):
    import warp_model as wm
    rng = rng_of(seed)
    grid = (amp * rng.uniform(-1.0, 1.0, tuple(grid_shape) + (3,))).astype(np.float32)
    m = vt.utils.transform_matrix(rotation=tuple(rng.uniform(-20.0, 20.0, 3)), rotation_order='rzxz', translation=tuple(rng.uniform(-1.0, 1.0, 3)),
                                  center=np.divide(np.subtract(out, 1), 2)).astype(np.float64)
    m[:3, 3] += np.subtract(VOLUME, 1) / 2 - np.subtract(out, 1) / 2
    m = m.astype(np.float32) if f32 else m

    def truth(got, vol, interp, tol):
        vals, ins, s = wm.warp(vol, m.astype(np.float64), grid, out, interp)
        keep = wm.skirt_distance(s, VOLUME) > 1e-9
        assert (~keep).sum() <= 0.001 * keep.size
        err = float(np.abs(got.astype(np.float64) - vals)[keep].max())
        print(f'warp[{tag}] {interp}: max|hip - model| {err:.3e}  bound {tol:.3e}  inside {int(ins.sum())}')
        assert ins.any() and err <= tol, (tag, interp, err)
        outside = keep & ~ins
        assert not got.view(np.uint32)[outside].any(), tag            # exact +0 outside
    tag = f'grid={"x".join(map(str, grid_shape))},out={"x".join(map(str, out))}{",f32" if f32 else ""}'
    return Variant('warp', tag, lambda sv, o: sv.warp(grid, m, out, output=o), out, device, WARP_TABLE + (grid.size + 1) // 2, truth=truth)


# ---- the stack families (kinds 21-25) ----------------------------------------------------------------------------------------------
def _stack_matrices(rng, n, out):
    ms = vt.utils.stack_matrices(rng.uniform(-6.0, 6.0, (n, 2)), rng.uniform(-180.0, 180.0, n), rng.uniform(0.7, 1.4, n), VOLUME, out)
    m4 = np.zeros((n, 4, 4))
    m4[:, 0, 0] = 1
    m4[:, 1:, 1:] = ms
    return ms, m4


def _planes(rng, n):
    return None if n == T else rng.integers(0, T, n)


def affine_stack(n, out, seed, device, f32=False):
    import backproject_model as bm
    rng = rng_of(seed)
    ms, m4 = _stack_matrices(rng, n, out)
    planes, ws = _planes(rng, n), weights(n, seed)
    if f32:
        ms = ms.astype(np.float32)
        m4 = m4.astype(np.float32).astype(np.float64)
    tag = f'n={n},out={out[0]}x{out[1]}{",f32" if f32 else ""}'

    def truth(got, vol, interp, tol):
        vols, masks = bm.per_entry(vol, m4, planes, (1,) + tuple(out), interp)
        assert masks.any()
        for i in range(n):
            err = float(np.abs(got[i].astype(np.float64) - ws[i] * vols[i, 0]).max())
            print(f'affine_stack[{tag}] {interp} entry {i}: max|hip - model| {err:.3e}  bound {abs(ws[i]) * tol:.3e}')
            assert err <= abs(ws[i]) * tol, (tag, interp, i, err)
    return Variant('affine_stack', tag, lambda sv, o: sv.affine_stack(ms, out, ws, output=o, planes=planes), (n,) + tuple(out), device,
                   (ENTRY + 1) * n, truth=truth)


def _warp_stack_table(n, grid_floats):
    return ENTRY * n + ((n + 1) & ~1) + WARP_STACK_HEADER + (grid_floats + 1) // 2


def warp_stack(n, grid_shape, shared, out, seed, device, matrices=True, amp=1.5):
    import warp_stack_model as wsm
    assert n % 2 == 1                                                 # the pad weight w[n] exists
    rng = rng_of(seed)
    grids = (amp * rng.uniform(-1.0, 1.0, (() if shared else (n,)) + tuple(grid_shape) + (2,))).astype(np.float32)
    ms, m4 = _stack_matrices(rng, n, out) if matrices else (None, None)
    planes, ws = _planes(rng, n), weights(n, seed)
    tag = f'n={n},{"shared" if shared else "own"} {grid_shape[0]}x{grid_shape[1]},out={out[0]}x{out[1]}'

    def truth(got, vol, interp, tol):
        vols, masks, dist = wsm.warp_stack(vol, m4, grids, planes, tuple(out), interp)
        with np.errstate(invalid='ignore'):
            kept = ~(dist <= wsm.SKIRT_EPS)
        assert kept.mean() >= 0.999 and masks.any()
        for i in range(n):
            err = float(np.abs(got[i].astype(np.float64) - ws[i] * vols[i])[kept[i]].max()) if kept[i].any() else 0.0
            print(f'warp_stack[{tag}] {interp} entry {i}: max|hip - model| {err:.3e}  bound {abs(ws[i]) * tol:.3e}')
            assert err <= abs(ws[i]) * tol, (tag, interp, i, err)
    return Variant('warp_stack', tag, lambda sv, o: sv.warp_stack(grids, ms, out, ws, output=o, planes=planes), (n,) + tuple(out), device,
                   _warp_stack_table(n, grids.size), truth=truth)


def warp_stack_refused(n, grid_shape, shared, out, nan_node, seed):
    """A grid with one NaN node, `nan_node` nodes from the start of the grids: refused inside the pass that copies the grids into the
    staging vector, with every piece before the node's already copied.  (Pieces are 32768 nodes, or a whole grid if smaller.)"""
    rng = rng_of(seed)
    grids = rng.uniform(-1.0, 1.0, (() if shared else (n,)) + tuple(grid_shape) + (2,)).astype(np.float32)
    nodes = grid_shape[0] * grid_shape[1]
    assert nan_node >= min(nodes, 32768) and nan_node < grids.size // 2
    grids.reshape(-1, 2)[nan_node, 1] = np.nan
    planes, ws = rng.integers(0, T, n).astype(np.int32), weights(n, seed)

    def call(sv, o):
        if sv.device == 'cpu':
            return sv.warp_stack(grids, None, out, ws, output=o, planes=planes)
        rc = sv._lib.vt_volume_warp_stack(sv._handle, n, None, grids.ctypes.data, 1 if shared else n, grid_shape[0], grid_shape[1],
                                          planes.ctypes.data, ws.ctypes.data, out[0], out[1], o.ctypes.data, 0)
        if rc:
            raise ValueError(f'vt_volume_warp_stack (code {rc}): {sv._lib.vt_last_error().decode()}')
    tag = f'refused: NaN at node {nan_node},n={n},{"shared" if shared else "own"} {grid_shape[0]}x{grid_shape[1]}'
    return Variant('warp_stack', tag, call, (n,) + tuple(out), False, _warp_stack_table(n, grids.size), refusal=True, late_refusal=True)


ZEROS9 = np.array([0.1, 0.0, -0.3, 0.0, 1.0, 0.0, 0.25, 0.0, -0.05])          # interior zeros: 5 compacted taps, a dense row of 9


def filter_stack(n, taps, axis, pad, seed, device):
    import filter_stack_model as fm
    rng = rng_of(seed)
    taps = np.asarray(taps, np.float64)
    assert (taps == 0).any() and taps.shape[0] in (n, taps.size)
    planes, ws = _planes(rng, n), weights(n, seed)
    rows = 1 if taps.ndim == 1 else n
    tag = f'n={n},{"shared" if taps.ndim == 1 else "rows"} K={taps.shape[-1]},axis{axis},{pad}'

    def truth(got, vol, interp, tol):
        fm.check(got, *fm.model(vol, taps, axis, pad, planes, ws), tag)
    table = FILTER_ENTRY * n + 2 * int(np.count_nonzero(taps)) + rows * (taps.shape[-1] + FILTER_CHUNK)
    return Variant('filter_stack', tag, lambda sv, o: sv.filter_stack(taps, axis, ws, pad, output=o, planes=planes), (n, H, W), device, table,
                   truth=truth)


def tap_rows(n, k, seed):
    """n rows of k taps, a third of them zero, the centre never."""
    rng = rng_of(seed)
    t = rng.uniform(-1.0, 1.0, (n, k))
    t[rng.uniform(size=(n, k)) < 0.34] = 0.0
    t[:, 0] = 0.0
    t[:, k // 2] = 1.0
    return t


def correlate_stack(n, refs, max_shift, grid, seed, device):
    """refs: 'shared', 'own' (n host references) or 'planes' (reference_planes)."""
    rng = rng_of(seed)
    planes = _planes(rng, n)
    references = {'shared': lambda: field((H, W), seed + 1), 'own': lambda: field((n, H, W), seed + 1), 'planes': lambda: None}[refs]()
    ref_planes = rng.integers(0, T, n) if refs == 'planes' else None
    floats = 0 if references is None else references.size
    shape = (n,) + tuple(grid) + (2 * max_shift[0] + 1, 2 * max_shift[1] + 1)
    tag = f'n={n},{refs}{" odd-refs" if floats % 2 else ""},grid {grid[0]}x{grid[1]},window {max_shift[0]}x{max_shift[1]}'

    def partials(cubic, cap):
        return csm.launches(H, W, max_shift, grid, n, cap)[0] * csm.plan(H, W, max_shift, grid)['unit_part_bytes']

    def truth(got, vol, interp, tol):
        csm.check(got, *csm.model(vol, references, max_shift, grid, planes, ref_planes), tag)
    v = Variant('correlate_stack', tag,
                lambda sv, o: sv.correlate_stack(references, max_shift, grid, output=o, planes=planes, reference_planes=ref_planes),
                shape, device, n + (floats + 1) // 2, f64=True, partials=partials, truth=truth, odd_refs=floats % 2 == 1)
    v.launch_plan, v.ref_floats = (max_shift, grid, n), floats
    return v


def moments_stack(n, max_shift, grid, seed, device):
    planes = _planes(rng_of(seed), n)
    shape = (n,) + tuple(grid) + (2 * max_shift[0] + 1, 2 * max_shift[1] + 1, 2)
    tag = f'n={n},grid {grid[0]}x{grid[1]},window {max_shift[0]}x{max_shift[1]}'

    def partials(cubic, cap):
        return msm.launches(H, W, max_shift, grid, n, cap)[0] * msm.plan(H, W, max_shift, grid)['unit_part_bytes']

    def truth(got, vol, interp, tol):
        msm.check(got, *msm.model(vol, max_shift, grid, planes), tag)
    v = Variant('moments_stack', tag, lambda sv, o: sv.moments_stack(max_shift, grid, output=o, planes=planes), shape, device, n, f64=True,
                partials=partials, truth=truth)
    v.launch_plan = (max_shift, grid, n)
    return v


def refused_on_filt(family, device=False):
    """The three families that need samples, on a filt_* handle: refused before anything is touched."""
    if family == 'filter_stack':
        v = filter_stack(T, ZEROS9, 2, 'zero', 90, device)
    elif family == 'correlate_stack':
        v = correlate_stack(T, 'shared', (1, 1), (1, 1), 91, device)
    else:
        v = moments_stack(T, (1, 1), (1, 1), 92, device)
    return Variant('refused', f'{family} on filt_*', v.call, v.shape, False, 0, f64=v.f64, refusal=True)


# ---- pools ----------------------------------------------------------------------------------------------------------------------------
DEV, HOST = True, False


@functools.lru_cache(maxsize=None)
def all_pools():
    p = {
        'affine_batch': [affine_batch(1, 1, DEV), affine_batch(40, 2, HOST), affine_batch(3, 3, HOST), affine_batch(2, 4, DEV)],
        'extract': [extract(1, 5, DEV), extract(40, 6, HOST), extract(2, 7, HOST), extract(41, 8, DEV)],
        'extract_sum': [extract_sum(1, 9, DEV, w=False), extract_sum(40, 10, HOST), extract_sum(1, 11, HOST), extract_sum(40, 12, DEV)],
        'extract_sum_multi': [extract_sum_multi(1, 1, 13, HOST), extract_sum_multi(12, 9, 14, HOST), extract_sum_multi(40, 1, 15, DEV),
                              extract_sum_multi(12, 9, 16, DEV), extract_sum_multi(1, 3, 17, DEV)],
        'extract_dot': [extract_dot(1, 18, DEV), extract_dot(40, 19, HOST, mask=True), extract_dot(1, 20, HOST), extract_dot(40, 21, DEV)],
        'extract_dot_multi': [extract_dot_multi(1, 1, 22, HOST), extract_dot_multi(40, 5, 23, HOST, mask=True), extract_dot_multi(1, 2, 24, DEV),
                              extract_dot_multi(40, 5, 25, DEV)],
        'projection_batch': [projection_batch(1, (7, 13, 15), 26, DEV), projection_batch(7, (20, 22, 24), 27, HOST),
                             projection_batch(40, (10, 12, 14), 28, HOST), projection_batch(7, (20, 22, 24), 29, DEV)],
        'place': [place(1, 30, DEV), place(40, 31, HOST, accumulate=True), place(9, 32, HOST), place(3, 33, HOST, accumulate=True, outside=True),
                  place(9, 34, DEV, accumulate=True)],
        'backproject': [backproject(T, 35, DEV), backproject(40, 36, HOST, accumulate=True), backproject(1, 37, HOST), backproject(5, 38, DEV, accumulate=True)],
        'backproject_boxes': [backproject_boxes(1, 3, 39, DEV), backproject_boxes(5, 8, 40, HOST, accumulate=True), backproject_boxes(2, 3, 41, HOST),
                              backproject_boxes(3, 4, 42, DEV, accumulate=True)],
        'warp': [warp((2, 3, 4), (5, 37, 45), 43, HOST), warp((1, 1, 1), (4, 21, 33), 44, DEV), warp((6, 40, 50), (6, 40, 50), 45, DEV, f32=True),
                 warp((3, 5, 7), (6, 37, 45), 46, HOST, amp=6.0)],
        'affine_stack': [affine_stack(1, IMG, 47, DEV), affine_stack(40, IMG, 48, HOST), affine_stack(T, (H, W), 49, DEV, f32=True),
                         affine_stack(5, IMG_SMALL, 50, HOST)],
        'warp_stack': [warp_stack(1, (3, 5), True, IMG, 51, DEV), warp_stack(41, (2, 2), False, IMG_SMALL, 52, HOST),
                       warp_stack(7, (3, 5), False, IMG, 53, DEV, matrices=False), warp_stack(5, (4, 1), True, IMG, 54, HOST, amp=6.0),
                       warp_stack_refused(3, (20, 30), False, IMG, 2 * 600 + 431, 55), warp_stack_refused(T, (200, 200), True, (200, 200), 39000, 56)],
        'filter_stack': [filter_stack(T, ZEROS9, 2, 'zero', 57, HOST), filter_stack(40, tap_rows(40, 61, 58), 1, 'edge', 58, DEV),
                         filter_stack(1, ZEROS9, 1, 'edge', 59, DEV), filter_stack(T, tap_rows(T, 21, 60), 2, 'zero', 60, HOST)],
        'correlate_stack': [correlate_stack(T, 'shared', (1, 2), (3, 5), 61, DEV), correlate_stack(40, 'planes', (2, 3), (3, 5), 62, HOST),
                            correlate_stack(7, 'own', (2, 7), (1, 1), 63, DEV), correlate_stack(1, 'planes', (0, 0), (3, 5), 64, HOST),
                            correlate_stack(3, 'own', (1, 1), (2, 3), 65, HOST), correlate_stack(7, 'planes', (2, 7), (1, 1), 66, HOST)],
        'moments_stack': [moments_stack(1, (0, 0), (3, 5), 67, DEV), moments_stack(40, (2, 7), (1, 1), 68, HOST), moments_stack(T, (1, 2), (2, 3), 69, HOST),
                          moments_stack(5, (2, 7), (1, 1), 70, DEV)],
        'refused': [refused_on_filt('filter_stack'), refused_on_filt('correlate_stack'), refused_on_filt('moments_stack')],
    }
    for fam, pool in p.items():
        assert all(v.family == fam for v in pool) and len({v.name for v in pool}) == len(pool), fam
    return p


FAMILIES = ['affine_batch', 'extract', 'projection_batch', 'extract_sum', 'extract_dot', 'extract_dot_multi', 'extract_sum_multi', 'place',
            'backproject', 'backproject_boxes', 'warp', 'affine_stack', 'warp_stack', 'filter_stack', 'correlate_stack', 'moments_stack']
BACK = ['affine_stack', 'warp_stack', 'backproject', 'backproject_boxes']
THREE_D = FAMILIES[:8] + ['warp']
USES_PARTIALS = ['extract_sum', 'extract_sum_multi', 'extract_dot', 'extract_dot_multi', 'projection_batch', 'correlate_stack', 'moments_stack']
TAKES_N = [f for f in FAMILIES if f not in ('warp', 'backproject_boxes')]       # a pool holds n = 1 and an n >= 40 (boxes: nb x n)


def split_cap():
    """VT_DOT_PART_CAP of the `linear_split` handle: two units of the correlate variant with the largest partials per launch."""
    return 2 * max(csm.plan(H, W, v.launch_plan[0], v.launch_plan[1])['unit_part_bytes'] for v in all_pools()['correlate_stack'])


class Handle:
    def __init__(self, name, interpolation, stack, families, cap, seed):
        self.name, self.interpolation, self.stack, self.families, self.cap, self.seed = name, interpolation, stack, families, cap, seed
        self.cubic = bim.is_cubic(interpolation)

    def partial_bytes(self, v):
        return v.partial_bytes(self.cubic, self.cap or DEFAULT_CAP)

    def create(self, setenv=None, delenv=None):
        """A GPU handle on the volume.  With a lowered cap the environment holds VT_DOT_PART_CAP around the creation only (setenv, delenv:
        monkeypatch's)."""
        if self.cap:
            setenv('VT_DOT_PART_CAP', str(self.cap))
        try:
            return vt.StaticVolume(volume(), interpolation=self.interpolation, device='gpu:0', stack=self.stack)
        finally:
            if self.cap:
                delenv('VT_DOT_PART_CAP')


HANDLES = {h.name: h for h in (
    Handle('linear', 'linear', False, FAMILIES, 0, 1),
    Handle('linear_split', 'linear', False, FAMILIES, split_cap(), 2),
    Handle('filt_stack', 'filt_bspline', True, BACK + ['refused'], 0, 3),
    Handle('filt_3d', 'filt_bspline', False, THREE_D, 0, 4),
)}

# the adjacencies a handle's walk must hold at least once (a condition whose two sides the handle's families cannot supply is left out)
_TABLES = ['large table after small', 'small table after large']
_KINDS = ['host after device', 'device after host', 'accumulate after plain']
_PARTS = ['largest partials after none', 'none after largest partials', 'float64 after float32', 'float32 after float64']
_LATE = ['served call after a late refusal']
_LINEAR = _TABLES + _KINDS + _PARTS + _LATE + ['odd references after a longer table', 'correlate_stack after a late refusal',
                                                'filter_stack after a late refusal', 'extract_dot after a late refusal']
REQUIRED = {'linear': _LINEAR, 'linear_split': _LINEAR, 'filt_3d': _TABLES + _KINDS + _PARTS,
            'filt_stack': _TABLES + _KINDS + _LATE + ['warp_stack after a call refused on filt_*', 'a call refused on filt_* after warp_stack']}


# ---- the circuit and the draw ------------------------------------------------------------------------------------------------------------
def circuit(families, seed):
    """An Eulerian circuit of the complete directed graph on `families`, self-loops included: len(families)^2 + 1 names, every ordered
    pair (a, b) adjacent exactly once.  Hierholzer's walk over successor lists shuffled by `seed`."""
    fam = list(families)
    rng = np.random.default_rng(seed)
    succ = {a: [fam[i] for i in rng.permutation(len(fam))] for a in fam}
    stack, path = [fam[0]], []
    while stack:
        if succ[stack[-1]]:
            stack.append(succ[stack[-1]].pop())
        else:
            path.append(stack.pop())
    return path[::-1]


def _served(a, b):
    return not a.refusal and not b.refusal


# condition -> does the pair of neighbours (a, b) meet it?  p: the handle's partial bytes of a variant; largest: their maximum
CONDITIONS = {
    'large table after small': lambda a, b, p, largest: _served(a, b) and a.table <= SMALL_TABLE and b.table >= LARGE_TABLE,
    'small table after large': lambda a, b, p, largest: _served(a, b) and a.table >= LARGE_TABLE and b.table <= SMALL_TABLE,
    'host after device': lambda a, b, p, largest: _served(a, b) and a.device and not b.device,
    'device after host': lambda a, b, p, largest: _served(a, b) and not a.device and b.device,
    'accumulate after plain': lambda a, b, p, largest: _served(a, b) and not a.accumulate and b.accumulate,
    'largest partials after none': lambda a, b, p, largest: _served(a, b) and largest > 0 and p(a) == 0 and p(b) == largest,
    'none after largest partials': lambda a, b, p, largest: _served(a, b) and largest > 0 and p(a) == largest and p(b) == 0,
    'float64 after float32': lambda a, b, p, largest: _served(a, b) and not a.f64 and b.f64,
    'float32 after float64': lambda a, b, p, largest: _served(a, b) and a.f64 and not b.f64,
    'odd references after a longer table': lambda a, b, p, largest: _served(a, b) and b.odd_refs and a.table > b.table,
    'served call after a late refusal': lambda a, b, p, largest: a.late_refusal and not b.refusal,
    'correlate_stack after a late refusal': lambda a, b, p, largest: a.late_refusal and b.family == 'correlate_stack',
    'filter_stack after a late refusal': lambda a, b, p, largest: a.late_refusal and b.family == 'filter_stack',
    'extract_dot after a late refusal': lambda a, b, p, largest: a.late_refusal and b.family == 'extract_dot',
    'warp_stack after a call refused on filt_*': lambda a, b, p, largest: a.family == 'refused' and b.family == 'warp_stack' and not b.refusal,
    'a call refused on filt_* after warp_stack': lambda a, b, p, largest: a.family == 'warp_stack' and not a.refusal and b.family == 'refused',
}


def adjacencies(handle, steps):
    """{condition: the step index of its first occurrence} over the neighbours of `steps`."""
    h = HANDLES[handle] if isinstance(handle, str) else handle
    largest = max(h.partial_bytes(v) for f in h.families for v in all_pools()[f])
    found = {}
    for i in range(1, len(steps)):
        for k, met in CONDITIONS.items():
            if k not in found and met(steps[i - 1], steps[i], h.partial_bytes, largest):
                found[k] = i
    return found


REGRESSIONS = {name: [] for name in HANDLES}       # named steps in front of the circuit: pairs that once differed from a fresh handle


@functools.lru_cache(maxsize=None)
def steps(handle):
    """The walk of a handle: REGRESSIONS[handle], then one variant per step of circuit(families, seed), drawn by a seeded generator.
    The draw is then patched, in a fixed order: for every adjacency of REQUIRED[handle] that it misses, the first pair of neighbouring
    steps whose families can supply it is set to the first two variants that do, and pinned; every variant of the pools that does not
    appear yet takes the first step of its family that is not pinned (a family that occurs less often than its pool is long cannot
    show them all)."""
    h = HANDLES[handle]
    fams = circuit(h.families, h.seed)
    pools = all_pools()
    largest = max(h.partial_bytes(v) for f in h.families for v in pools[f])
    rng = np.random.default_rng(h.seed)
    walk = [pools[f][int(rng.integers(len(pools[f])))] for f in fams]
    pinned = set()
    for k in REQUIRED[handle]:
        if k in adjacencies(h, walk):
            pinned.update(i for i in (adjacencies(h, walk)[k] - 1, adjacencies(h, walk)[k]))
            continue
        for i in range(1, len(walk)):
            firsts = [walk[i - 1]] if i - 1 in pinned else pools[fams[i - 1]]
            seconds = [walk[i]] if i in pinned else pools[fams[i]]
            pair = next(((a, b) for a in firsts for b in seconds if CONDITIONS[k](a, b, h.partial_bytes, largest)), None)
            if pair:
                walk[i - 1], walk[i] = pair
                pinned.update((i - 1, i))
                break
    for f in h.families:
        for v in pools[f]:
            if v not in walk:
                at = next((i for i, g in enumerate(fams) if g == f and i not in pinned), None)
                if at is not None:
                    walk[at] = v
                    pinned.add(at)
    missing = [k for k in REQUIRED[handle] if k not in adjacencies(h, walk)]
    assert not missing, (handle, missing)
    return tuple(REGRESSIONS[handle]) + tuple(walk)


def affine_check_matrix():
    """A general rotation about the volume's centre for the plain affine() between the steps of the two linear walks."""
    return vt.utils.transform_matrix(rotation=(25.0, -40.0, 63.0), rotation_order='rzxz', translation=(0.4, -1.3, 2.2),
                                     center=np.divide(np.subtract(VOLUME, 1), 2, dtype=np.float32))
