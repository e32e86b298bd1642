"""Seeded sequences of mixed calls on ONE vt_volume handle, and the stateless model they are held to.

A handle carries state from call to call (voltools_amd/csrc/vt_host.h: launch_no, reorient_asked, the lazy copy table with its budget,
the shared tile counters d_queue, the staging plans and their epoch, the cached plane sum of the projection helper, staging buffers sized by
the largest call so far, the output shape) and sits on a per-device recycler of the buffers of destroyed handles.  The per-call suites
(parity, lattice, fuzz, extract) use a handle for a few calls of one kind; the sequences here interleave every kind of call.

Plain numpy, no GPU, no pytest.  A sequence is a tuple of `Op` records; every record that transforms carries everything its expected
value depends on (volume spec, interpolation, boundary contract, slab window, output shape, matrices, flags), so `expected(op)` needs no
handle and no history: that is the model.  tests/test_handle_sequences.py asserts the coverage conditions and the order independence
of `expected`; tests/test_gpu_sequences.py runs the sequences on the GPU.

Families
  P  "pure": VT_REORIENT=0, no budget, no set_max_resident: the route of a call is a function of (source shape, output shape, matrix,
     flags) alone, so every op can be repeated alone on a fresh handle and must give the same kernel, tile, grid and bits.
  S  "stateful policy": default VT_REORIENT, budgets, release_copies, device_trim: routes depend on history, results must not.
  E  one edge='scipy' handle (reference: scipy.ndimage.affine_transform, the package's device='cpu' path).
  L  one slab handle with both interior flags.

Pairs of persistent-queue families: the three kernels that share d_queue are the lane-block kernel (kind 9), the packed-span kernel
(kind 6, trilinear) and round 1's packed kernel (kind 6, cubic, VT_FORCE_PACKED).  Which of span / packed serves kind 6 is fixed by the
handle's interpolation (vt_api.hip: launch_planned), and d_queue is per handle: span -> packed and packed -> span CANNOT occur on one
handle.  QUEUE_PAIRS lists what can: block <-> packed on a cubic handle, block <-> span on a trilinear handle created with
VT_BLOCK_LINEAR=1; IMPOSSIBLE_QUEUE_PAIRS lists the other two.

recreate: the recycler (vt_api.hip: cached_malloc / cached_free) hands out a parked buffer of EXACTLY the requested size, and a resident
copy takes D * H * pitch(W) * 4 bytes with pitch(W) = (W + 35) & ~31.  `dirty_shape` gives, for every source shape used here, another
shape with the same D * H, the same pitch and a larger width: a `recreate` destroys the handle, creates one from a volume of that
shape holding values of magnitude 1e3 (its rows reach into what will be the pad columns of the next handle), transforms once into a
host array of the next handle's output size (so the recycled host-output staging holds 1e3 values too), destroys it and creates the
next unit-range handle, whose resident copy, prefilter partner and staging are then the recycled ones -- provided the recycler holds no
other buffer of that size (it returns the first match): the scripted recreates of `_coda` call vt_device_trim first, the random ones do not.
"""
import dataclasses
from typing import Optional, Tuple

import numpy as np

import lattice_cases as lc
import voltools_amd as vt
from voltools_amd import _native as N
from conftest import interior_mask
from test_gpu_fuzz import FLAG_SETS as FUZZ_FLAG_SETS, random_matrix, KINDS as FUZZ_KINDS

SEED = 20261017
FT = N.FORCE_TILED
ALL_INTERPS = ('linear', 'bspline', 'bspline_simple', 'filt_bspline', 'filt_bspline_simple')
# the flag sets of tests/test_gpu_parity.py::test_tiled_and_direct_match_oracle
PARITY_FLAG_SETS = (FT | N.FORCE_XSWAP, FT | N.FORCE_XSWAP | N.NO_ZPAIR, FT | N.FORCE_XSWAP | N.NO_QUAD, FT | N.NO_QUAD | N.NO_RSWAP, FT, FT | N.NO_RSWAP,
                    FT | N.NO_MARCH, FT | N.NO_ZSEP, FT | N.NO_ZSEP | N.NO_BLOCK, FT | N.NO_ZSEP | N.FORCE_PACKED, FT | N.NO_ZSEP | N.NO_PACKED, N.FORCE_DIRECT)
EXTRA_FLAG_SETS = (FT | N.NO_PLANSHARE, FT | N.NO_ZFIR, FT | N.NO_ROWS, FT | N.NO_REORIENT, N.NO_REORIENT, N.NO_PLANSHARE | N.NO_ZFIR)
FLAG_POOL = tuple(dict.fromkeys(tuple(int(f) for f in FUZZ_FLAG_SETS) + PARITY_FLAG_SETS + EXTRA_FLAG_SETS))
PACKED = FT | N.NO_ZSEP | N.FORCE_PACKED
BOXES_FLAGS = FT | N.NO_ZSEP | N.NO_PACKED

SMALL_SHAPES = ((41, 70, 133), (64, 64, 64))
MEDIUM_SHAPE = (176, 200, 232)
SMALL_OUT = {(41, 70, 133): {'larger': (50, 81, 140), 'smaller': (30, 44, 90)}, (64, 64, 64): {'larger': (72, 80, 96), 'smaller': (33, 50, 47)}}
# medium: `smaller` still exceeds 96^3 (queued batch launches) and leaves the lane-block kernel more tiles (13 * 13 * 8) than workgroups
MEDIUM_OUT = {'larger': (180, 208, 240), 'smaller': (100, 104, 120)}
OTHER_SHAPE = (33, 47, 50)
BOXES = ((12, 9, 20), (24, 24, 24))
SENTINEL = np.float32(-77.0)          # no interpolated value of unit-range data gets there (cubic overshoot stays within a few units)
SENTINEL_KEEP = SENTINEL

TRANSFORMS = ('affine', 'affine_batch', 'extract', 'project')
P_KINDS = ('affine', 'affine_batch', 'extract', 'project', 'set_output_shape', 'release_copies', 'device_trim', 'recreate', 'other_handle')
# no ordered pair of these kinds is impossible on a whole-volume handle: every op leaves a usable handle behind
IMPOSSIBLE_KIND_PAIRS = ()
QUEUE_PAIRS = (('block', 'packed'), ('packed', 'block'), ('block', 'span'), ('span', 'block'))
IMPOSSIBLE_QUEUE_PAIRS = (('span', 'packed'), ('packed', 'span'))


def resident_pitch(W):
    return (W + 4 + 31) & ~31


def resident_bytes(shape):
    return shape[0] * shape[1] * resident_pitch(shape[2]) * 4


def dirty_shape(shape):
    """Another shape whose resident copy has the same size in bytes: D and H exchanged (or, for a square plane, D halved and H doubled) and
    the widest width of the same pitch."""
    D, H, W = shape
    wide = resident_pitch(W) - 4            # pitch(w) == pitch(W) for every w in (pitch - 36, pitch - 4]
    d2, h2 = (H, D) if D != H else (D // 2, H * 2)
    out = (d2, h2, wide)
    assert resident_bytes(out) == resident_bytes(shape) and wide > W and (d2, h2) != (D, H), (shape, out)
    return out


@dataclasses.dataclass(frozen=True)
class Vol:
    shape: Tuple[int, int, int]
    seed: int
    scale: float = 1.0

    def make(self):
        v = np.random.RandomState(self.seed).random_sample(self.shape).astype(np.float32)
        return v if self.scale == 1.0 else (v * np.float32(self.scale)).astype(np.float32)


@dataclasses.dataclass(frozen=True)
class Op:
    kind: str                                   # one of TRANSFORMS, 'set_output_shape', 'set_max_resident', 'release_copies', 'device_trim', 'recreate'
    handle: str = 'main'                        # 'main' | 'other' (kind 'other_handle' of the coverage conditions = any op with handle 'other')
    cls: str = ''                               # matrix class (vocabulary of the parity / fuzz / lattice suites) or a label
    m: Tuple[Tuple[float, ...], ...] = ()       # matrices, 16 entries each (already rounded to float32 where f64 is False)
    f64: bool = False
    flags: int = 0
    device_out: bool = False
    keep: bool = False
    out_shape: Optional[Tuple[int, int, int]] = None      # output grid of the call (boxes: the box)
    vol: Optional[Vol] = None                   # the source the handle holds at this point
    interp: str = ''
    edge: str = 'texture'
    window: Optional[Tuple[int, int, int, int]] = None    # slabs: (w0, w1, G, g0): resident planes [w0, w1) of G, output plane 0 is global plane g0
    arg: Tuple = ()                             # set_output_shape: the shape; set_max_resident: ('0' | 'plain' | '2.6',); recreate: (dirty Vol, new Vol)
    qfam: str = ''                              # persistent-queue family the flags select ('block' | 'packed' | 'span'), '' otherwise
    exempt: bool = False                        # class 'far': the output may be empty

    @property
    def transforms(self):
        return self.kind in TRANSFORMS

    @property
    def cov_kind(self):
        return 'other_handle' if self.handle == 'other' else self.kind

    def matrices(self):
        return [np.asarray(m, np.float64).reshape(4, 4) for m in self.m]


@dataclasses.dataclass(frozen=True)
class Sequence:
    family: str
    name: str
    interp: str
    vol: Vol
    env: Tuple[Tuple[str, str], ...]
    ops: Tuple[Op, ...]
    edge: str = 'texture'
    window: Optional[Tuple[int, int, int, int, int]] = None   # slabs: (w0, w1, G, g0, g1)
    other_interp: str = ''
    other_vol: Optional[Vol] = None
    medium: bool = False


# ---------------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------------
def _parity_matrices():
    from test_gpu_parity import MATRICES
    return MATRICES


LATTICE_PICKS = (0, 7, 31, 64, 90, 151, 170, 200)          # a few entries of lattice_cases.SPECS (texture groups)


def inside_share(m, out_shape, src_shape):
    """Share of output voxels whose source coordinate lies inside the source (conftest.interior_mask, margin 0), on every voxel of a
    small grid and on every k-th voxel per axis of a large one (the matrix columns scaled accordingly)."""
    m = np.asarray(m, np.float64).reshape(4, 4)
    k = max(1, int(round((np.prod(out_shape) / 2.5e4) ** (1.0 / 3.0))))
    sub = tuple((s + k - 1) // k for s in out_shape)
    ms = m.copy()
    ms[:3, :3] = m[:3, :3] * k
    return float(interior_mask(ms, sub, src_shape, 0).mean())


def follows_axis(m):
    """The source axis the output's w direction follows, by the rule of vt_api.hip: try_general_reorient (ties and near-ties stay on axis
    2, the plain copy).  A general-matrix launch (kinds 2, 6, 9) whose answer is 0 or 1 samples an axis-permuted copy once the handle has
    built it -- at the fourth request, or never when the budget has no room -- and the plain copy before: the same kernel on the same tile
    then adds its taps in another order, so its bits depend on the handle's history (to rounding: ~2e-7)."""
    m = np.asarray(m, np.float64).reshape(4, 4)
    c = np.abs(m[:3, 2])
    a = 2
    if c[1] > 1.15 * c[2] and c[1] >= c[0]:
        a = 1
    if c[0] > 1.15 * c[2] and c[0] > c[1]:
        a = 0
    return a


def _rot(axis, deg):
    a = np.deg2rad(deg)
    i, j = [x for x in range(3) if x != axis]
    R = np.eye(3)
    R[i, i] = R[j, j] = np.cos(a)
    R[i, j], R[j, i] = -np.sin(a), np.sin(a)
    return R


def about_centre(L, shape, t=(0.0, 0.0, 0.0)):
    c = (np.asarray(shape, np.float64) - 1) / 2
    m = np.eye(4)
    m[:3, :3] = L
    m[:3, 3] = c - L @ c + np.asarray(t, np.float64)
    return m


MATRIX_CLASSES = tuple('parity:' + k for k in ('identity', 'shift_int', 'shift_frac', 'rot_inplane45', 'rot_inplane100', 'rot_inplane260', 'rot_general',
                                               'rot_scale_shift', 'shear', 'magnify3', 'minify', 'minify_big', 'far_outside', 'mirror', 'rot_axis2',
                                               'rot_axis2_shift', 'rot_axis1', 'rot_axis1_shift')) + \
    tuple('fuzz:' + k for k in FUZZ_KINDS) + tuple('lattice:%d' % i for i in LATTICE_PICKS)
FAR_CLASSES = ('fuzz:far', 'parity:far_outside')


def draw_matrix(rs, cls, src_shape, out_shape):
    """A float64 4x4 of class `cls` with at least 10 % of the output inside the source (class 'far' excepted); falls back to a small
    fractional shift after 40 draws (singular matrices and magnifications about the centre of another grid can stay outside)."""
    for attempt in range(40):
        if cls.startswith('parity:'):
            m = np.asarray(_parity_matrices()[cls[7:]](src_shape), np.float64)
        elif cls.startswith('fuzz:'):
            m = np.asarray(random_matrix(rs, src_shape, cls[5:]), np.float64)
        elif cls.startswith('lattice:'):
            _, m, _ = lc.place(lc.SPECS[int(cls[8:])], tuple(src_shape))
        elif cls == 'axis0_int':            # in-plane rotation, integer axis-0 offset: cubic launches share staging plans (KIND 4)
            m = about_centre(_rot(0, rs.uniform(5, 40)), src_shape)
            m[0, 3] = float(rs.randint(-2, 3))
        elif cls == 'general':
            # (the output's w axis keeps following source axis 2: no reoriented copy is ever asked for, whatever the handle's history)
            m = about_centre(_rot(2, rs.uniform(15, 40)) @ _rot(1, rs.uniform(10, 30)) @ _rot(0, rs.uniform(-30, 30)), src_shape, rs.uniform(-2, 2, 3))
            if follows_axis(m) != 2:
                continue
        elif cls == 'reorient0':            # the output's w axis follows source axis 0 (general: not axis-1-separable)
            m = about_centre(_rot(1, rs.uniform(70, 80)) @ _rot(0, rs.uniform(6, 12)), src_shape, rs.uniform(-1, 1, 3))
        elif cls == 'reorient1':            # ... follows source axis 1
            m = about_centre(_rot(0, rs.uniform(70, 80)) @ _rot(1, rs.uniform(6, 12)), src_shape, rs.uniform(-1, 1, 3))
        elif cls == 'pad_probe':            # taps the first pad column: source x in (W - 1, W - 0.5) for the last output column
            m = np.eye(4)
            m[:3, 3] = (0.25, 0.25, 0.25)
        else:
            raise KeyError(cls)
        if cls in FAR_CLASSES or inside_share(m, out_shape, src_shape) >= 0.10:
            return m, cls
        if cls.startswith('parity:') or cls.startswith('lattice:') or cls == 'pad_probe':
            break                           # deterministic classes: another draw gives the same matrix
    m = np.eye(4)
    m[:3, 3] = (0.5, -1.25, 0.75)
    return m, 'parity:shift_frac*'


def box_matrix(rs, src_shape, box):
    R = vt.utils.rotation_matrix(tuple(rs.uniform(0, 360, 3)), 'deg', 'sxyz', dtype=np.float64)[:3, :3]
    c = (np.asarray(box, np.float64) - 1) / 2
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = rs.uniform(0.3, 0.7, 3) * np.asarray(src_shape, np.float64) - R @ c
    return m


def _freeze(ms, f64):
    out = []
    for m in ms:
        m = np.asarray(m, np.float64).reshape(4, 4)
        if not f64:
            m = m.astype(np.float32).astype(np.float64)
        out.append(tuple(float(x) for x in m.ravel()))
    return tuple(out)


# ---------------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------------
def euler_circuit(k):
    """Closed walk over the complete directed graph with loops on k symbols: every ordered pair occurs once as consecutive symbols."""
    nxt = [0] * k
    stack, out = [0], []
    while stack:
        v = stack[-1]
        if nxt[v] < k:
            nxt[v] += 1
            stack.append(nxt[v] - 1)
        else:
            out.append(stack.pop())
    return out[::-1]


class _Gen:
    def __init__(self, family, name, interp, vol, rs, medium=False, edge='texture', window=None, other_interp='', other_vol=None, flag_start=0):
        self.family, self.name, self.interp, self.vol, self.rs = family, name, interp, vol, rs
        self.medium, self.edge, self.window = medium, edge, window
        self.other_interp, self.other_vol = other_interp, other_vol
        self.base_shape = vol.shape
        self.out = self._native_out(vol.shape)
        self.other_out = other_vol.shape if other_vol else None
        self.ops = []
        self.nflag = flag_start
        self.ncls = flag_start
        self.nmisc = flag_start
        self.proj = (0.0, 20.0)             # (tz, in-plane angle) of the last fused projection
        self.nvol = 0

    def _native_out(self, shape):
        if self.window:
            w0, w1, G, g0, g1 = self.window
            return (g1 - g0, shape[1], shape[2])
        return tuple(shape)

    def _pick(self, seq, counter):
        n = getattr(self, counter)
        setattr(self, counter, n + 1)
        return seq[n % len(seq)]

    def _ctx(self, handle):
        if handle == 'other':
            return self.other_vol, self.other_interp, self.other_out
        return self.vol, self.interp, self.out

    def _op(self, kind, handle, **kw):
        vol, interp, out = self._ctx(handle)
        kw.setdefault('out_shape', out)
        w = self.window[:4] if (self.window and handle == 'main') else None
        op = Op(kind=kind, handle=handle, vol=vol, interp=interp, edge=self.edge if handle == 'main' else 'texture', window=w, **kw)
        self.ops.append(op)
        return op

    def _qfam(self, cls, flags, interp, handle):
        """Which persistent-queue family the flags select for a general matrix (the medium handles run with a low VT_BLOCK_MIN, the
        trilinear one with VT_BLOCK_LINEAR=1)."""
        if not (self.medium and handle == 'main' and cls in ('general', 'reorient0', 'reorient1')):
            return ''
        if flags & N.FORCE_DIRECT or (flags & N.NO_PACKED and not flags & N.FORCE_PACKED):
            return ''
        if flags & N.FORCE_PACKED:
            return 'span' if interp == 'linear' else 'packed'
        if flags & N.NO_BLOCK:
            return ''
        return 'block'

    # ---- ops ----
    def affine(self, handle='main', cls=None, flags=None, keep=None, f64=None, device_out=None):
        rs = self.rs
        vol, interp, out = self._ctx(handle)
        cls = cls or self._pick(MATRIX_CLASSES, 'ncls')
        flags = self._pick(FLAG_POOL, 'nflag') if flags is None else flags
        m, cls = draw_matrix(rs, cls, vol.shape, out)
        f64 = bool(rs.randint(2)) if f64 is None else f64
        if cls.startswith('lattice:'):
            f64 = True                      # (their point is the float64 offset)
        keep = (rs.randint(4) == 0) if keep is None else keep
        if flags & N.FORCE_XSWAP or self.edge == 'scipy':
            keep = False                    # (the exchange path declines keep_outside; scipy has no such mode)
        device_out = (rs.randint(3) == 0) if device_out is None else device_out
        return self._op('affine', handle, cls=cls, m=_freeze([m], f64), f64=f64, flags=int(flags), keep=bool(keep), device_out=bool(device_out),
                        qfam=self._qfam(cls, flags, interp, handle), exempt=cls in FAR_CLASSES)

    def affine_batch(self, handle='main', n=None, flags=0):
        rs = self.rs
        vol, interp, out = self._ctx(handle)
        n = n or self._pick((1, 3, 7), 'nmisc')
        ms = [draw_matrix(rs, ('fuzz:general', 'fuzz:axis0', 'fuzz:affine', 'parity:identity')[i % 4], vol.shape, out)[0] for i in range(n)]
        keep = self.edge != 'scipy' and rs.randint(3) == 0
        return self._op('affine_batch', handle, cls='batch%d' % n, m=_freeze(ms, False), flags=int(flags), keep=bool(keep), device_out=bool(rs.randint(2)))

    def extract(self, handle='main', n=None, box=None, flags=None, f64=None):
        rs = self.rs
        vol, interp, out = self._ctx(handle)
        n = n or self._pick((1, 5), 'nmisc')
        box = box or self._pick(BOXES, 'nmisc')
        flags = self._pick((0, N.FORCE_TILED, N.FORCE_DIRECT), 'nmisc') if flags is None else flags
        f64 = bool(rs.randint(2)) if f64 is None else f64
        ms = []
        for _ in range(n):
            for attempt in range(40):
                m = box_matrix(rs, vol.shape, box)
                if inside_share(m, box, vol.shape) >= 0.10:
                    break
            ms.append(m)
        return self._op('extract', handle, cls='boxes%d' % n, m=_freeze(ms, f64), f64=f64, flags=int(flags), device_out=bool(rs.randint(2)), out_shape=tuple(box))

    def project(self, handle='main', how=None, flags=0):
        """how: 'hit' (new in-plane map, the tz of the last projection: the cached plane sum serves it), 'new_tz' (the same in-plane map,
        another tz), 'new_inplane' (the same tz; the map changes by more than a quarter turn), 'general' (transform, then sum)."""
        rs = self.rs
        vol, interp, out = self._ctx(handle)
        how = how or self._pick(('hit', 'new_tz', 'new_inplane', 'general', 'hit'), 'nmisc')
        tz, ang = self.proj
        if how == 'general':
            m, _ = draw_matrix(rs, 'general', vol.shape, out)
        else:
            if how == 'hit':
                ang = ang + float(rs.uniform(5, 30))
            elif how == 'new_tz':
                tz = tz + float(rs.choice([1.25, -0.75, 2.0, -1.5]))
                if abs(tz) > 4:
                    tz = 0.5
            else:
                ang = ang + 100.0
            m = about_centre(_rot(0, ang), vol.shape, (0.0, 1.0, -2.5))
            m[0, 3] = tz
            if handle == 'main':
                self.proj = (tz, ang)
        f64 = bool(rs.randint(2))
        return self._op('project', handle, cls='proj_' + how, m=_freeze([m], f64), f64=f64, flags=int(flags), device_out=bool(rs.randint(3) == 0),
                        out_shape=tuple(out))

    def set_output_shape(self, which=None):
        table = MEDIUM_OUT if self.medium else SMALL_OUT[self.base_shape]
        which = which or self._pick(('larger', 'smaller', 'source'), 'nmisc')
        shape = self._native_out(self.base_shape) if which == 'source' else table[which]
        if shape == self.out:               # (always a change)
            shape = table['smaller'] if which != 'smaller' else self._native_out(self.base_shape)
        self.out = tuple(shape)
        return self._op('set_output_shape', 'main', cls=which, arg=tuple(shape))

    def set_max_resident(self, which=None):
        which = which or self._pick(('2.6', 'plain', '0'), 'nmisc')
        return self._op('set_max_resident', 'main', cls=which, arg=(which,))

    def simple(self, kind):
        return self._op(kind, 'main')

    def recreate(self):
        self.nvol += 1
        dirty = Vol(dirty_shape(self.base_shape), self.vol.seed + 1000 + self.nvol, 1.0e3)
        new = Vol(self.base_shape, self.vol.seed + 100 * self.nvol, 1.0)
        op = self._op('recreate', 'main', arg=(dirty, new))
        self.vol = new
        self.out = self._native_out(self.base_shape)        # a new handle starts with its source shape
        self.proj = (0.0, 20.0)
        return op

    def other(self):
        k = self._pick(('affine', 'project', 'extract', 'affine_batch', 'affine'), 'nmisc')
        return getattr(self, k)(handle='other')

    def by_kind(self, kind):
        if kind == 'other_handle':
            return self.other()
        if kind in ('release_copies', 'device_trim'):
            return self.simple(kind)
        return getattr(self, kind)()

    def finish(self, env):
        return Sequence(family=self.family, name=self.name, interp=self.interp, vol=self.first_vol, env=tuple(sorted(env.items())), ops=tuple(self.ops),
                        edge=self.edge, window=self.window, other_interp=self.other_interp, other_vol=self.other_vol, medium=self.medium)


def _gen(family, name, interp, vol, medium=False, **kw):
    # (the seed is a function of the name: sequences do not depend on the order they are built in)
    rs = np.random.RandomState((SEED + sum(ord(c) * (i + 1) for i, c in enumerate(name))) % (2 ** 31))
    g = _Gen(family, name, interp, vol, rs, medium=medium, **kw)
    g.first_vol = vol
    return g


def _coda(g, cubic):
    """The patterns the state bugs need, in every P sequence whatever the random part did: the plane sum reused across a change of the
    output depth and of tz; two consecutive plan-sharing launches on one grid (cubic); a recycled allocation probed at its pad columns."""
    g.set_output_shape('source')
    g.project(how='new_tz')
    g.set_output_shape('smaller')
    g.project(how='hit')                    # same tz, smaller output depth: the sum covers fewer planes
    g.project(how='new_tz')
    g.set_output_shape('source')
    g.project(how='new_inplane')            # same tz, output depth back
    if cubic:
        g.affine(cls='axis0_int', flags=FT, keep=False)
        g.affine(cls='axis0_int', flags=FT, keep=False)
        g.affine(cls='axis0_int', flags=FT | N.NO_PLANSHARE, keep=False)
        g.affine(cls='axis0_int', flags=0, keep=False)
    g.simple('device_trim')                 # nothing else parked: the next handle's buffers are exactly the outgoing ones
    g.recreate()
    # (the kernels that stage whole 16-byte vectors read the pad columns: the general-matrix families; the direct kernel tests every tap)
    g.affine(cls='pad_probe', flags=BOXES_FLAGS, keep=False, device_out=False)
    g.affine(cls='pad_probe', flags=FT | N.NO_ZSEP, keep=False)
    g.affine(cls='pad_probe', flags=0, keep=False)
    g.project(how='hit')


P_ENV = {'VT_REORIENT': '0'}
MEDIUM_ENV = {'VT_BLOCK_MIN': '32'}


def family_p_small():
    circuit = euler_circuit(len(P_KINDS))
    assert len(circuit) == len(P_KINDS) ** 2 + 1
    seqs = []
    i = 0
    for shape in SMALL_SHAPES:
        for interp in ALL_INTERPS:
            name = 'P-small-%s-%s' % ('x'.join(map(str, shape)), interp)
            other_interp = ALL_INTERPS[(ALL_INTERPS.index(interp) + 2) % 5]
            g = _gen('P', name, interp, Vol(shape, 300 + i), other_interp=other_interp, other_vol=Vol(OTHER_SHAPE, 350 + i), flag_start=4 * i)
            start = (9 * i) % (len(circuit) - 1)
            walk = (circuit[:-1] * 2)[start:start + 38]
            for k in walk:
                g.by_kind(P_KINDS[k])
            _coda(g, interp != 'linear')
            seqs.append(g.finish(P_ENV))
            i += 1
    return seqs


def family_p_medium():
    seqs = []
    for i, interp in enumerate(('linear', 'bspline', 'filt_bspline')):
        name = 'P-medium-%s' % interp
        env = dict(P_ENV, **MEDIUM_ENV)
        if interp == 'linear':
            env['VT_BLOCK_LINEAR'] = '1'
        g = _gen('P', name, interp, Vol(MEDIUM_SHAPE, 400 + i), medium=True, other_interp=('bspline', 'linear', 'linear')[i],
                 other_vol=Vol(OTHER_SHAPE, 450 + i), flag_start=5 * i)
        second = PACKED                     # span on the trilinear handle, round 1's packed kernel on the cubic ones
        g.affine(cls='general', flags=FT, keep=False, device_out=True)          # block
        g.affine(cls='general', flags=second, keep=False)                       # span / packed: another grid on the same counters
        g.affine(cls='general', flags=0, keep=True)                             # block
        g.affine(cls='general', flags=BOXES_FLAGS, keep=False)                  # boxes (kind 2): no queue
        g.affine(cls='general', flags=second, keep=True, device_out=True)
        g.set_output_shape('smaller')
        g.affine(cls='general', flags=FT, keep=False)                           # block on a smaller grid
        g.affine_batch(n=7)                                                     # beyond 96^3: queued launches
        g.affine(cls='general', flags=second, keep=False)
        g.extract(n=5)
        g.other()
        g.set_output_shape('source')
        g.affine(cls='parity:rot_axis2', flags=FT, keep=False)                  # row kernel
        g.affine(cls='axis0_int', flags=FT, keep=False)                         # plane-quad
        g.affine(cls='axis0_int', flags=FT, keep=False)
        g.project(how='hit')
        g.simple('release_copies')
        g.project(how='hit')
        g.project(how='general')
        g.simple('device_trim')
        g.affine(cls='parity:rot_inplane100', flags=FT, keep=False)             # the in-plane transposed orientation
        g.affine_batch(n=3)
        g.recreate()
        g.affine(cls='pad_probe', flags=0, keep=False)
        g.affine_batch(n=1)
        g.affine(cls='general', flags=second, keep=False)
        g.affine(cls='general', flags=FT, keep=False)
        seqs.append(g.finish(env))
    return seqs


def family_s():
    seqs = []
    for i, interp in enumerate(('linear', 'filt_bspline')):
        g = _gen('S', 'S-medium-%s' % interp, interp, Vol(MEDIUM_SHAPE, 500 + i), medium=True, other_interp=('bspline', 'linear')[i],
                 other_vol=Vol(OTHER_SHAPE, 550 + i), flag_start=7 * i)
        env = dict(MEDIUM_ENV)
        second = PACKED
        # no budget yet: the copy for general matrices whose w axis follows source axis 0 is built at the fourth request
        for k in range(4):
            g.affine(cls='reorient0', flags=0, keep=False, device_out=bool(k & 1))
        g.affine(cls='axis0_int', flags=FT, keep=False)                         # plane-quad, odd / even launches
        g.affine(cls='axis0_int', flags=FT, keep=False)
        g.set_max_resident('2.6')
        g.affine(cls='parity:rot_axis1', flags=FT, keep=False)                  # another orientation: evictions
        g.affine(cls='parity:rot_inplane100', flags=FT, keep=False)
        g.affine(cls='general', flags=FT, keep=False)                           # block
        g.affine(cls='general', flags=second, keep=False)                       # span / packed
        g.project(how='hit')
        g.affine(cls='parity:rot_axis2_shift', flags=FT, keep=False)
        g.simple('release_copies')
        g.project(how='hit')
        g.affine(cls='axis0_int', flags=FT, keep=False)
        g.set_max_resident('plain')
        g.affine(cls='axis0_int', flags=FT, keep=False)                         # no copy fits: a family on the plain layout
        g.affine(cls='general', flags=0, keep=True)
        g.set_output_shape('smaller')
        g.affine(cls='reorient1', flags=FT, keep=False)
        g.affine_batch(n=3)
        g.simple('device_trim')
        g.other()
        g.set_max_resident('0')
        g.set_output_shape('source')
        for k in range(4):
            g.affine(cls='reorient1', flags=0, keep=False)
        g.extract(n=5)
        g.set_max_resident('2.6')
        g.affine(cls='parity:rot_axis1_shift', flags=FT, keep=False)
        g.affine(cls='axis0_int', flags=FT | N.NO_ZFIR, keep=False)
        g.project(how='new_tz')
        g.recreate()
        g.affine(cls='pad_probe', flags=0, keep=False)
        g.set_max_resident('2.6')
        g.affine(cls='general', flags=second, keep=False)
        g.affine(cls='general', flags=FT, keep=False)
        g.affine(cls='axis0_int', flags=FT, keep=False)
        seqs.append(g.finish(env))
    return seqs


def family_e():
    seqs = []
    for i, interp in enumerate(('linear', 'filt_bspline')):
        g = _gen('E', 'E-%s' % interp, interp, Vol((33, 47, 50), 600 + i), edge='scipy', flag_start=3 * i)
        for k in ('affine', 'project', 'affine_batch', 'extract', 'affine', 'affine', 'extract', 'project', 'affine_batch', 'affine', 'project', 'affine',
                  'extract', 'affine', 'affine_batch', 'project'):
            if k == 'affine':
                # matrices that put nothing on scipy's cut except chain-exact ones (tests/test_gpu_lattice.py on why): the parity / fuzz classes
                g.affine(cls=g._pick(('parity:rot_general', 'parity:shift_int', 'parity:rot_inplane45', 'parity:identity', 'parity:rot_axis2',
                                      'parity:rot_scale_shift', 'fuzz:general', 'parity:rot_axis1_shift'), 'ncls'),
                         flags=g._pick((0, FT, N.FORCE_DIRECT, PACKED, BOXES_FLAGS, FT | N.NO_QUAD), 'nflag'), keep=False)
            elif k == 'project':
                g.project(how=g._pick(('hit', 'general', 'new_tz'), 'nmisc'))
            else:
                g.by_kind(k)
        seqs.append(g.finish({}))
    return seqs


def family_l():
    """The middle slab of three: resident window [10, 86) of 96 planes (halo 10 on either side), output planes [30, 66)."""
    seqs = []
    G, H, W = 96, 40, 46
    for i, interp in enumerate(('linear', 'filt_bspline')):
        window = (10, 86, G, 30, 66)
        g = _gen('L', 'L-%s' % interp, interp, Vol((G, H, W), 700 + i), window=window, flag_start=2 * i)
        g.base_shape = (G, H, W)
        for k in ('affine', 'project', 'affine', 'set_output_shape', 'affine', 'project', 'set_output_shape', 'project', 'affine', 'affine', 'project'):
            if k == 'affine':
                # axis-0 offsets inside the halo (the window holds the planes such a slab is given)
                ang = float(g.rs.uniform(-60, 60))
                m = about_centre(_rot(0, ang), (G, H, W), (0.0, float(g.rs.uniform(-2, 2)), float(g.rs.uniform(-2, 2))))
                m[0, 3] = float(g.rs.choice([0.0, 1.25, -2.0, 0.5]))
                flags = g._pick((0, FT, FT | N.NO_ZSEP, N.FORCE_DIRECT, N.NO_QUAD | FT), 'nflag')
                keep = bool(g.rs.randint(2))
                g._op('affine', 'main', cls='slab_axis0', m=_freeze([m], True), f64=True, flags=int(flags), keep=keep, device_out=bool(g.rs.randint(2)))
            elif k == 'project':
                how = g._pick(('hit', 'new_tz', 'hit'), 'nmisc')
                tz, ang = g.proj
                ang += 17.0
                if how == 'new_tz':
                    tz = 1.25 if tz != 1.25 else -0.75
                g.proj = (tz, ang)
                m = about_centre(_rot(0, ang), (G, H, W), (0.0, 1.0, -2.5))
                m[0, 3] = tz
                g._op('project', 'main', cls='proj_' + how, m=_freeze([m], True), f64=True, flags=0, out_shape=tuple(g.out))
            else:
                # vt_volume_set_output_shape takes any handle (the header makes no exception for slabs; the planes written are
                # [out_plane0, out_plane0 + out_depth) of the global output): fewer planes and another in-plane grid, then back
                shape = (20, 36, 50) if g.out == (36, H, W) else (36, H, W)
                g.out = shape
                g._op('set_output_shape', 'main', cls='slab', arg=shape)
        seqs.append(g.finish({}))
    return seqs


_CACHE = {}


def sequences(family):
    """The sequences of a family ('P-small', 'P-medium', 'P', 'S', 'E', 'L'); generated once per process, deterministic."""
    if family == 'P':
        return sequences('P-small') + sequences('P-medium')
    if family not in _CACHE:
        _CACHE[family] = {'P-small': family_p_small, 'P-medium': family_p_medium, 'S': family_s, 'E': family_e, 'L': family_l}[family]()
    return _CACHE[family]


def without_policy_ops(seq):
    """The twin of an S sequence without set_max_resident / release_copies / device_trim."""
    return dataclasses.replace(seq, ops=tuple(op for op in seq.ops if op.kind not in ('set_max_resident', 'release_copies', 'device_trim')))


# ---------------------------------------------------------------------------------------------------
# the stateless model
# ---------------------------------------------------------------------------------------------------
class Model:
    """expected(op): what a transforming op must return, from the record alone.  Keeps the (prefiltered) volumes it has made; nothing
    else (tests/test_handle_sequences.py evaluates a sequence in two orders and compares bit for bit)."""

    def __init__(self):
        self.vols = {}

    def volume(self, vol):
        if vol not in self.vols:
            if len(self.vols) > 6:
                self.vols.clear()
            self.vols[vol] = (vol.make(), {})
        return self.vols[vol][0]

    def source(self, vol, interp):
        from oracle import oracle
        v = self.volume(vol)
        if not interp.startswith('filt'):
            return v
        cache = self.vols[vol][1]
        if 'filt' not in cache:
            cache['filt'] = oracle.prefilter(v)
        return cache['filt']

    def _one(self, op, m64, init=None):
        from oracle import oracle
        if op.edge == 'scipy':
            from scipy.ndimage import affine_transform
            order, prefilter = (1, False) if op.interp == 'linear' else (3, op.interp.startswith('filt'))
            return affine_transform(self.volume(op.vol), m64, output_shape=tuple(op.out_shape), order=order, prefilter=prefilter).astype(np.float32)
        src = self.source(op.vol, op.interp)
        kind = op.interp[5:] if op.interp.startswith('filt') else op.interp
        plane0, gD, out_plane0 = 0, src.shape[0], 0
        if op.window:
            w0, w1, gD, out_plane0 = op.window
            src = np.ascontiguousarray(src[w0:w1])
            plane0 = w0
        out = np.zeros(tuple(op.out_shape), np.float32) if init is None else init
        m = np.ascontiguousarray(np.asarray(m64, np.float64).reshape(16))
        rc = oracle.lib().vt_oracle_affine_ex(src, *src.shape, plane0, gD, out, *out.shape, out_plane0, m, oracle.INTERP[kind],
                                              oracle.KEEP_OUTSIDE if init is not None else 0)
        assert rc == 0
        return out

    def expected(self, op):
        """affine: (D, H, W); affine_batch / extract: (n, ...); project: (H, W) float64 plane sum.  keep ops: the untouched voxels hold
        SENTINEL."""
        assert op.transforms
        ms = op.matrices()
        if op.kind == 'project':
            return self._one(op, ms[0]).astype(np.float64).sum(axis=0)
        keep = op.keep and op.kind in ('affine', 'affine_batch')
        outs = [self._one(op, m, np.full(tuple(op.out_shape), SENTINEL, np.float32) if keep else None) for m in ms]
        return outs[0] if op.kind == 'affine' else np.stack(outs)


def tolerance(op):
    """The tolerances the project states: tests/test_gpu_parity.py (texture contract), tests/test_gpu_edge_scipy.py (edge='scipy'), times the
    output depth for projections."""
    from test_gpu_parity import TOL
    from test_gpu_edge_scipy import TOL as TOL_SCIPY
    tol = (TOL_SCIPY if op.edge == 'scipy' else TOL)[op.interp]
    return tol * op.out_shape[0] if op.kind == 'project' else tol
