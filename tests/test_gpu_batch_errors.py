"""-m gpu: the refusals of the nine batched C entry points (vt_volume_extract .. vt_volume_backproject_boxes), one table.

Every row is (entry point, handle, precisions, arguments that differ from a valid call, return code, vt_last_error() text); the texts are
written out from the library's source.  The rows cover each function's own refusals, a non-finite value at a chosen matrix entry, weight
or voxel with the index the message names, and inputs that are wrong in two ways at once: the ORDER of the checks is part of the contract.
No row reaches a launch: the handles' last_kernel is still 0 when the table is through.

Handles over a 20 x 22 x 24 volume: linear, filt_bspline, filt_bspline with VT_STACK, linear with VT_EDGE_SCIPY, a linear slab window
and a linear handle that was never finalized.  The float32 entry points run their own first checks before they widen the matrices, so
some rows differ between the precisions (vt_volume_backproject_boxes has no such checks)."""
import ctypes

import numpy as np
import pytest

import voltools_amd as vt
from voltools_amd import _native

pytestmark = pytest.mark.gpu

VT_EINVAL, VT_EUNSUPPORTED = 10001, 10004
SHAPE = (20, 22, 24)
BOTH, F32, F64 = (False, True), (False,), (True,)

NULLARG = 'NULL argument'
INPLANE = "the handle's coefficients are in-plane (VT_STACK with a filt_* interpolation): only vt_volume_backproject samples them"
NOTFINAL = 'handle has not been finalized (vt_volume_finalize)'
AXIS0 = ("the handle's coefficients are prefiltered along axis 0 as well: back-projection with a filt_* interpolation "
         "needs in-plane coefficients (create the handle with VT_STACK)")
NOSCIPY = 'back-projection is not available on VT_EDGE_SCIPY handles'


def slab(op):
    return f'{op} is available for whole-volume handles only (this one holds a slab window)'


# entry point -> (noun of its shape, "too large" text, name of the operation in the slab refusal)
FUNCS = {
    'extract': ('box', 'box too large', 'box extraction'),
    'project_batch': ('output', 'output too large', 'batched projection'),
    'extract_sum': ('box', 'box too large', 'box summation'),
    'extract_dot': ('box', 'box too large', 'box scoring'),
    'extract_dot_multi': ('box', 'box too large', 'box scoring'),
    'extract_sum_multi': ('box', 'box too large', 'box summation'),
    'place': ('output', 'output too large', 'placing copies'),
    'backproject': ('output', 'output too large', 'back-projection'),
    'backproject_boxes': ('box', 'box too large', 'back-projection'),
}
BACK = ('backproject', 'backproject_boxes')


def small(x):
    return x if 1 <= x <= 64 else 1


def call(lib, fn, h, f64, o):
    """One call of entry point `fn`: a valid call (n = 2, box 4 x 5 x 6, host output) with the arguments in `o` replaced.  Arrays are
    sized for the valid call, or for one element where a count or a shape is absurd: such rows are refused before anything is read."""
    n, nb, k, g = o.get('n', 2), o.get('nb', 2), o.get('k', 2), o.get('g', 2)
    box = o.get('box', (4, 5, 6))
    vox = int(np.prod(box)) if all(1 <= b <= 64 for b in box) else 1
    cnt = small(n) * (small(nb) if fn == 'backproject_boxes' else 1)
    m = np.tile(np.eye(4, dtype=np.float64 if f64 else np.float32), (cnt, 1, 1))
    for i, e in o.get('nan_at', ()):
        m.reshape(-1)[16 * i + e] = np.nan
    if 'm' in o:
        m = o['m']
    out = o['out'] if 'out' in o else np.zeros(4096, np.float64)
    w = o.get('w', np.ones((cnt, small(g))) if fn == 'extract_sum_multi' else None)
    w = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    planes = o.get('planes', np.arange(small(n)) if fn in BACK else None)
    planes = None if planes is None else np.ascontiguousarray(planes, dtype=np.int32)
    tmpl = np.ones((small(k) if fn == 'extract_dot_multi' else 1, vox), np.float32)
    for j, i in o.get('tmpl_nan', ()):
        tmpl[j, i] = np.nan
    if 'tmpl' in o:
        tmpl = o['tmpl']
    mask = None
    if 'mask_nan' in o:
        mask = np.ones(vox, np.float32)
        mask[o['mask_nan']] = np.inf

    def p(a):
        return None if a is None else a.ctypes.data

    args = {
        'extract': (n, p(m)),
        'project_batch': (n, p(m)),
        'extract_sum': (n, p(m), p(w)),
        'extract_dot': (n, p(m), p(tmpl), p(mask)),
        'extract_dot_multi': (n, p(m), k, p(tmpl), p(mask)),
        'extract_sum_multi': (n, p(m), g, p(w)),
        'place': (n, p(m), p(w)),
        'backproject': (n, p(m), p(planes), p(w)),
        'backproject_boxes': (nb, n, p(m), p(planes), p(w)),
    }[fn]
    f = getattr(lib, 'vt_volume_' + fn + ('_f64' if f64 else ''))
    rc = f(h, *args, *box, p(out), o.get('flags', 0))
    msg = lib.vt_last_error()
    return rc, (msg.decode() if msg else '')


def common_rows(fn):
    noun, too_large, op = FUNCS[fn]
    boxes = fn == 'backproject_boxes'
    empty32 = 'NULL argument or empty batch' if fn == 'extract' else None
    rows = [
        (fn, 'lin', F64, dict(m=None), VT_EINVAL, NULLARG),
        (fn, 'lin', F32, dict(m=None), VT_EINVAL, empty32 or NULLARG),
        (fn, 'lin', F64, dict(out=None), VT_EINVAL, NULLARG),
        (fn, 'lin', F32, dict(out=None), VT_EINVAL, empty32 or NULLARG),
        (fn, 'lin', F64, dict(n=0), VT_EINVAL, 'batch size 0'),
        (fn, 'lin', F32, dict(n=0), VT_EINVAL, empty32 or 'batch size 0'),
        (fn, 'lin', F64, dict(n=-3), VT_EINVAL, 'batch size -3'),
        (fn, 'lin', BOTH, dict(box=(0, 5, 6)), VT_EINVAL, f'non-positive {noun} dims (0,5,6)'),
        (fn, 'filt' if fn not in BACK else 'stk', BOTH, dict(box=(4, 5, -1)), VT_EINVAL, f'non-positive {noun} dims (4,5,-1)'),
        (fn, 'lin', BOTH, dict(box=(65536, 65536, 4)), VT_EUNSUPPORTED, too_large),
        (fn, 'lin', BOTH, dict(box=(4, 65536, 65536)), VT_EUNSUPPORTED, too_large),
        (fn, 'def', BOTH, {}, VT_EINVAL, NOTFINAL),
        (fn, 'slab', BOTH, {}, VT_EINVAL, slab(op)),
        (fn, 'lin', BOTH, dict(nan_at=[(1, 7)]), VT_EINVAL, 'matrix 1 entry 7 is not finite'),
        (fn, 'filt' if fn not in BACK else 'stk', BOTH, dict(nan_at=[(0, 15)]), VT_EINVAL, 'matrix 0 entry 15 is not finite'),
        (fn, 'lin', BOTH, dict(nan_at=[(1, 0), (0, 3)]), VT_EINVAL, 'matrix 0 entry 3 is not finite'),
        # wrong in two ways: the earlier check answers
        (fn, 'lin', F64, dict(n=0, box=(0, 5, 6)), VT_EINVAL, 'batch size 0'),
        (fn, 'lin', BOTH, dict(box=(0, 65536, 65536)), VT_EINVAL, f'non-positive {noun} dims (0,65536,65536)'),
        (fn, 'def', BOTH, dict(box=(4, 0, 6)), VT_EINVAL, f'non-positive {noun} dims (4,0,6)'),
        (fn, 'def', BOTH, dict(box=(65536, 65536, 4)), VT_EUNSUPPORTED, too_large),
        (fn, 'def', BOTH, dict(nan_at=[(0, 0)]), VT_EINVAL, NOTFINAL),
        (fn, 'slab', BOTH, dict(nan_at=[(0, 0)]), VT_EINVAL, slab(op)),
        (fn, 'slab', F64, dict(n=0), VT_EINVAL, 'batch size 0'),
        (fn, 'slab', F64, dict(out=None, n=0), VT_EINVAL, NULLARG),
    ]
    if fn not in BACK:
        rows += [
            (fn, 'stk', BOTH, {}, VT_EUNSUPPORTED, INPLANE),
            (fn, 'stk', F64, dict(n=0), VT_EUNSUPPORTED, INPLANE),
            (fn, 'stk', F32, dict(n=0), VT_EINVAL, empty32 or 'batch size 0'),
            (fn, 'stk', BOTH, dict(box=(0, 5, 6), nan_at=[(0, 0)]), VT_EUNSUPPORTED, INPLANE),
            (fn, 'stk', F32, dict(out=None), VT_EINVAL, empty32 or NULLARG),
            (fn, 'stk', F64, dict(out=None), VT_EINVAL, NULLARG),
        ]
    if boxes:      # no first checks in the float32 entry point: the precisions agree
        rows = [(f, hd, BOTH, o, rc, text) for (f, hd, prec, o, rc, text) in rows if prec != F32]
    return rows


ROWS = [r for fn in FUNCS for r in common_rows(fn)]

# ---- weights ---------------------------------------------------------------------------------------------------------------------------
for _fn in ('extract_sum', 'place', 'backproject'):
    ROWS += [
        (_fn, 'lin', BOTH, dict(w=[1.0, np.inf]), VT_EINVAL, 'weight 1 is not finite'),
        (_fn, 'lin', BOTH, dict(w=[np.nan, np.inf]), VT_EINVAL, 'weight 0 is not finite'),
        (_fn, 'lin', BOTH, dict(w=[np.nan, 1.0], nan_at=[(1, 11)]), VT_EINVAL, 'matrix 1 entry 11 is not finite'),
        (_fn, 'slab', BOTH, dict(w=[np.nan, 1.0]), VT_EINVAL, slab(FUNCS[_fn][2])),
    ]
ROWS += [
    ('extract_sum_multi', 'lin', BOTH, dict(g=0), VT_EINVAL, 'column count 0'),
    ('extract_sum_multi', 'lin', BOTH, dict(g=-2, w=None), VT_EINVAL, 'column count -2'),
    ('extract_sum_multi', 'lin', BOTH, dict(w=None), VT_EINVAL, 'NULL weights'),
    ('extract_sum_multi', 'lin', F64, dict(n=0, g=0, w=None), VT_EINVAL, 'batch size 0'),
    ('extract_sum_multi', 'lin', BOTH, dict(w=None, box=(0, 5, 6)), VT_EINVAL, 'NULL weights'),
    ('extract_sum_multi', 'def', BOTH, dict(w=None), VT_EINVAL, 'NULL weights'),
    ('extract_sum_multi', 'slab', BOTH, dict(g=0), VT_EINVAL, 'column count 0'),
    ('extract_sum_multi', 'stk', BOTH, dict(g=0, w=None), VT_EUNSUPPORTED, INPLANE),
    ('extract_sum_multi', 'lin', BOTH, dict(g=3, w=[[1, 2, 3], [4, np.inf, np.nan]]), VT_EINVAL, 'weight (1, 1) is not finite'),
    ('extract_sum_multi', 'filt', BOTH, dict(g=3, w=[[1, 2, np.nan], [4, 5, 6]], nan_at=[(1, 2)]), VT_EINVAL,
     'matrix 1 entry 2 is not finite'),
    ('backproject_boxes', 'lin', BOTH, dict(w=[[1.0, 2.0], [3.0, np.inf]]), VT_EINVAL, 'weight 3 is not finite'),
    ('backproject_boxes', 'lin', BOTH, dict(w=[[1.0, np.nan], [3.0, 4.0]], nan_at=[(3, 4)]), VT_EINVAL, 'matrix 3 entry 4 is not finite'),
]

# ---- templates and masks ---------------------------------------------------------------------------------------------------------------
ROWS += [
    ('extract_dot', 'lin', BOTH, dict(tmpl=None), VT_EINVAL, NULLARG),
    ('extract_dot', 'stk', BOTH, dict(tmpl=None), VT_EINVAL, NULLARG),
    ('extract_dot', 'lin', BOTH, dict(box=(2048, 1024, 1024)), VT_EUNSUPPORTED, 'box too large'),      # (bd + 16) bh bw
    ('extract_dot', 'def', BOTH, dict(box=(2048, 1024, 1024)), VT_EUNSUPPORTED, 'box too large'),
    ('extract_dot', 'lin', BOTH, dict(tmpl_nan=[(0, 7)]), VT_EINVAL, 'template voxel 7 is not finite'),
    ('extract_dot', 'lin', BOTH, dict(mask_nan=119), VT_EINVAL, 'mask voxel 119 is not finite'),
    ('extract_dot', 'lin', BOTH, dict(tmpl_nan=[(0, 5)], mask_nan=5), VT_EINVAL, 'template voxel 5 is not finite'),
    ('extract_dot', 'lin', BOTH, dict(tmpl_nan=[(0, 5)], mask_nan=3), VT_EINVAL, 'mask voxel 3 is not finite'),      # one loop over the voxels
    ('extract_dot', 'filt', BOTH, dict(tmpl_nan=[(0, 0)], nan_at=[(1, 5)]), VT_EINVAL, 'matrix 1 entry 5 is not finite'),
    ('extract_dot', 'slab', BOTH, dict(tmpl_nan=[(0, 0)]), VT_EINVAL, slab('box scoring')),
    ('extract_dot_multi', 'lin', BOTH, dict(tmpl=None), VT_EINVAL, NULLARG),
    ('extract_dot_multi', 'lin', BOTH, dict(k=0), VT_EINVAL, 'template count 0'),
    ('extract_dot_multi', 'lin', BOTH, dict(k=-1, box=(0, 5, 6)), VT_EINVAL, 'template count -1'),
    ('extract_dot_multi', 'lin', F64, dict(n=0, k=0), VT_EINVAL, 'batch size 0'),
    ('extract_dot_multi', 'stk', BOTH, dict(k=0), VT_EUNSUPPORTED, INPLANE),
    ('extract_dot_multi', 'def', BOTH, dict(k=0), VT_EINVAL, 'template count 0'),
    ('extract_dot_multi', 'lin', BOTH, dict(box=(2048, 1024, 1024)), VT_EUNSUPPORTED, 'box too large'),
    ('extract_dot_multi', 'lin', BOTH, dict(k=2147483647), VT_EUNSUPPORTED, 'box tiles x (2 + k) = 2147483649 exceeds 2^31 - 1'),
    ('extract_dot_multi', 'lin', BOTH, dict(k=2147483647, nan_at=[(0, 0)]), VT_EUNSUPPORTED,
     'box tiles x (2 + k) = 2147483649 exceeds 2^31 - 1'),                                            # before any array is read
    ('extract_dot_multi', 'slab', BOTH, dict(k=2147483647), VT_EINVAL, slab('box scoring')),
    ('extract_dot_multi', 'lin', BOTH, dict(tmpl_nan=[(1, 7)]), VT_EINVAL, 'template 1 voxel 7 is not finite'),
    ('extract_dot_multi', 'lin', BOTH, dict(mask_nan=2), VT_EINVAL, 'mask voxel 2 is not finite'),
    ('extract_dot_multi', 'lin', BOTH, dict(tmpl_nan=[(1, 5)], mask_nan=3), VT_EINVAL, 'template 1 voxel 5 is not finite'),      # the stack first
    ('extract_dot_multi', 'filt', BOTH, dict(tmpl_nan=[(0, 0)], nan_at=[(0, 9)]), VT_EINVAL, 'matrix 0 entry 9 is not finite'),
]

# ---- back-projection -------------------------------------------------------------------------------------------------------------------
for _fn, _per in (('backproject', ''), ('backproject_boxes', ' per box')):
    ROWS += [
        (_fn, 'filt', BOTH, {}, VT_EUNSUPPORTED, AXIS0),
        (_fn, 'scipy', BOTH, {}, VT_EUNSUPPORTED, NOSCIPY),
        (_fn, 'filt', BOTH, dict(nan_at=[(0, 0)], planes=[0, 99]), VT_EUNSUPPORTED, AXIS0),
        (_fn, 'filt', BOTH, dict(n=0), VT_EINVAL, 'batch size 0'),
        (_fn, 'filt', BOTH, dict(box=(0, 5, 6)), VT_EINVAL, 'non-positive %s dims (0,5,6)' % FUNCS[_fn][0]),
        (_fn, 'scipy', BOTH, dict(box=(65536, 65536, 4)), VT_EUNSUPPORTED, FUNCS[_fn][1]),
        (_fn, 'stk', BOTH, dict(planes=[0, 20]), VT_EINVAL, 'plane index 20 of entry 1 outside [0, 20)'),
        (_fn, 'lin', BOTH, dict(planes=[-1, 20]), VT_EINVAL, 'plane index -1 of entry 0 outside [0, 20)'),
        (_fn, 'lin', BOTH, dict(planes=None), VT_EINVAL, f'2 matrices{_per} for a stack of 20 images and no plane indices'),
        (_fn, 'lin', BOTH, dict(planes=[0, 20], w=np.full((2, 2), np.nan)), VT_EINVAL, 'weight 0 is not finite'),
        (_fn, 'lin', BOTH, dict(planes=[0, 20], nan_at=[(1, 6)]), VT_EINVAL, 'matrix 1 entry 6 is not finite'),
        (_fn, 'slab', BOTH, dict(planes=[0, 20]), VT_EINVAL, slab('back-projection')),
    ]
ROWS += [
    ('backproject_boxes', 'lin', BOTH, dict(nb=0), VT_EINVAL, 'number of boxes 0'),
    ('backproject_boxes', 'lin', BOTH, dict(nb=-1, n=0), VT_EINVAL, 'number of boxes -1'),
    ('backproject_boxes', 'filt', BOTH, dict(nb=0), VT_EINVAL, 'number of boxes 0'),
    ('backproject_boxes', 'lin', BOTH, dict(nb=0, out=None), VT_EINVAL, NULLARG),
    ('backproject_boxes', 'lin', BOTH, dict(nb=65536, n=65536), VT_EUNSUPPORTED,
     '65536 boxes x 65536 entries: more than 2^31 - 1 (box, entry) pairs'),
    ('backproject_boxes', 'scipy', BOTH, dict(nb=65536, n=65536), VT_EUNSUPPORTED, NOSCIPY),
    ('backproject_boxes', 'lin', BOTH, dict(nb=1 << 20, n=1, box=(32768, 65535, 32768)), VT_EUNSUPPORTED, 'output too large (1048576 boxes)'),
    # 2^30 boxes of 2 x 3 x 2 linear tiles (8, 8, 16); the bounds come before anything of the arrays is read
    ('backproject_boxes', 'lin', BOTH, dict(nb=1 << 30, n=1, box=(10, 18, 18)), VT_EUNSUPPORTED, 'grid too large (1073741824 boxes x 12 tiles)'),
    ('backproject_boxes', 'lin', BOTH, dict(nb=1 << 30, n=1, box=(10, 18, 18), nan_at=[(0, 0)], planes=[99]), VT_EUNSUPPORTED,
     'grid too large (1073741824 boxes x 12 tiles)'),
]


def test_every_refusal_has_its_code_and_text():
    lib = _native.load()
    vol = np.random.RandomState(3).random_sample(SHAPE).astype(np.float32)
    svs = {'lin': vt.StaticVolume(vol, interpolation='linear', device='gpu:0'),
           'filt': vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0'),
           'stk': vt.StaticVolume(vol, interpolation='filt_bspline', device='gpu:0', stack=True),
           'scipy': vt.StaticVolume(vol, interpolation='linear', device='gpu:0', edge='scipy')}
    handles = {k: sv._handle for k, sv in svs.items()}
    raw = {}
    for key, args in (('slab', (vol.ctypes.data, 0, 4, 40, 4, 20)), ('def', (None, _native.SRC_DEFERRED, 0, 20, 0, 20))):
        h = ctypes.c_void_p()
        _native.check(lib.vt_volume_create_slab(0, *SHAPE, 0, *args, ctypes.byref(h)), 'vt_volume_create_slab ' + key)
        raw[key] = handles[key] = h
    try:
        wrong = []
        for fn, hd, precisions, o, code, text in ROWS:
            for f64 in precisions:
                got = call(lib, fn, handles[hd], f64, o)
                if got != (code, text):
                    wrong.append((fn + ('_f64' if f64 else ''), hd, {k: v for k, v in o.items() if k != 'w'}, got, (code, text)))
        assert not wrong, '\n'.join(map(str, wrong))
        assert len(ROWS) > 9 * 24
        for key, h in handles.items():                       # nothing was launched
            info = _native.VolumeInfo()
            _native.check(lib.vt_volume_info(h, ctypes.byref(info)), 'vt_volume_info')
            assert info.last_kernel == 0 and info.last_grid == 0, key
    finally:
        for h in raw.values():
            lib.vt_volume_destroy(h)
        for sv in svs.values():
            sv.close()
