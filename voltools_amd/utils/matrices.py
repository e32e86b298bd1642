"""4x4 pull-matrix builders (host side, numpy only).

Behavioural mirror of the reference's ``voltools/utils/matrices.py``:

* every matrix is a *pull* map in array-axis order (row 0 <-> axis 0), see
  ``/root/reference/voltools/transforms.py:147-152`` (scipy call) and ``:265-274`` (kernel);
* ``translation_matrix`` negates its argument (``matrices.py:22-27``);
* ``rotation_matrix`` negates the angles ("CCW notation", ``matrices.py:45``) and understands the
  24 Euler conventions ``s|r`` + three axis letters (``matrices.py:6-19``);
* ``transform_matrix`` composes ``T . C- . R . Sh . Sc . C+`` with float32 products, left to right
  (``matrices.py:111-154``) and normalises by ``m[3, 3]``.

The rotation is assembled here from elementary axis rotations instead of the closed-form Euler
table the reference uses; the two agree to float64 rounding before the final cast to ``dtype``
(pinned by ``tests/golden/matrices.npz``).
"""
from functools import reduce
from itertools import permutations
from typing import Sequence, Tuple, Union

import numpy as np

_AXIS_INDEX = {'x': 0, 'y': 1, 'z': 2}


def _euler_orders():
    """All 24 conventions: proper (aba) and Tait-Bryan (abc) sequences in both frames."""
    seqs = []
    for a, b, c in permutations('xyz', 3):
        seqs.append(a + b + c)
    for a, b in permutations('xyz', 2):
        seqs.append(a + b + a)
    return [f + s for f in 'sr' for s in sorted(seqs)]


AVAILABLE_ROTATIONS = _euler_orders()
AVAILABLE_UNITS = ['rad', 'deg']

Vec3 = Union[Tuple[float, float, float], Sequence[float], np.ndarray]


def _axis_rotation(axis: int, angle: float) -> np.ndarray:
    """Right-handed rotation by ``angle`` (radians) about coordinate axis ``axis`` (float64 3x3)."""
    c, s = np.cos(angle), np.sin(angle)
    a, b = (axis + 1) % 3, (axis + 2) % 3
    r = np.identity(3, dtype=np.float64)
    r[a, a] = c
    r[a, b] = -s
    r[b, a] = s
    r[b, b] = c
    return r


def translation_matrix(translation: Vec3, dtype=np.float32) -> np.ndarray:
    """Pull matrix of a shift by ``translation``: the offset column holds ``-translation``."""
    m = np.identity(4, dtype=dtype)
    m[:3, 3] = np.negative(np.asarray(translation[:3], dtype=dtype))
    return m


def rotation_matrix(rotation: Vec3, rotation_units: str = 'deg', rotation_order: str = 'rzxz',
                    dtype=np.float32) -> np.ndarray:
    """Pull matrix of an Euler rotation ``rotation=(a0, a1, a2)`` in convention ``rotation_order``.

    ``s...``: rotations about the fixed axes in the order written; ``r...``: about the rotating
    axes in the order written (equivalently fixed axes in reverse order).  Angles are negated
    first, exactly like the reference (``matrices.py:45``).
    """
    if rotation_units not in AVAILABLE_UNITS:
        raise ValueError(f'Rotation units must be one of {AVAILABLE_UNITS}')
    if rotation_order not in AVAILABLE_ROTATIONS:
        raise ValueError(f'Rotation order must be one of {AVAILABLE_ROTATIONS}')

    angles = np.asarray(rotation, dtype=np.float64)[:3]
    if rotation_units == 'deg':
        angles = np.deg2rad(angles)
    angles = -angles

    frame, axes = rotation_order[0], [_AXIS_INDEX[ch] for ch in rotation_order[1:]]
    steps = [_axis_rotation(ax, an) for ax, an in zip(axes, angles)]
    if frame == 's':
        steps.reverse()          # fixed axes: the first rotation is applied first -> rightmost
    r3 = reduce(np.matmul, steps)

    m = np.identity(4, dtype=dtype)
    m[:3, :3] = r3
    return m


def shear_matrix(coefficients: Vec3, dtype=np.float32) -> np.ndarray:
    """Upper-triangular shear: ``c[0]`` couples axis 0<-1, ``c[1]`` 0<-2, ``c[2]`` 1<-2."""
    m = np.identity(4, dtype=dtype)
    m[0, 1], m[0, 2], m[1, 2] = coefficients[0], coefficients[1], coefficients[2]
    return m


def scale_matrix(coefficients: Vec3, dtype=np.float32) -> np.ndarray:
    m = np.identity(4, dtype=dtype)
    m[0, 0], m[1, 1], m[2, 2] = coefficients[0], coefficients[1], coefficients[2]
    return m


def transform_matrix(scale: Vec3 = None, shear: Vec3 = None, rotation: Vec3 = None,
                     rotation_units: str = 'deg', rotation_order: str = 'rzxz',
                     translation: Vec3 = None, center: Vec3 = None, dtype=np.float32) -> np.ndarray:
    """Compose translation . (centre shift) . rotation . shear . scale . (centre shift back).

    Products are taken left to right in ``dtype`` so the float32 rounding is the reference's
    (``matrices.py:122-150``); the result is divided by ``m[3, 3]``.
    """
    factors = []
    if translation is not None:
        factors.append(translation_matrix(translation, dtype))
    if center is not None:
        factors.append(translation_matrix(tuple(-1 * c for c in center), dtype))
    if rotation is not None:
        factors.append(rotation_matrix(rotation, rotation_units, rotation_order, dtype))
    if shear is not None:
        factors.append(shear_matrix(shear, dtype))
    if scale is not None:
        factors.append(scale_matrix(scale, dtype))
    if center is not None:
        factors.append(translation_matrix(center, dtype))

    m = reduce(np.dot, factors, np.identity(4, dtype=dtype))
    m /= m[3, 3]
    return m


def box_matrices(positions, rotations=None, box_shape=None, rotation_units: str = 'deg',
                 rotation_order: str = 'rzxz') -> np.ndarray:
    """Pull matrices (n, 4, 4), float64, of ``n`` boxes of shape ``box_shape`` cut out of a volume (``StaticVolume.extract``).

    With ``c = (box_shape - 1) / 2`` and ``R_i = rotation_matrix(rotations[i], ...)[:3, :3]`` (identity when ``rotations`` is
    None): ``M_i[:3, :3] = R_i`` and ``M_i[:3, 3] = positions[i] - R_i . c``, so the centre of box ``i`` samples the source at
    ``positions[i]``; with no rotation and an integer ``positions[i] - c`` the box is the plain crop starting there.
    """
    box = _box_shape(box_shape)
    pos = np.asarray(positions, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
        raise ValueError('positions must have shape (n, 3)')
    n = pos.shape[0]
    if rotations is not None:
        rot = np.asarray(rotations, dtype=np.float64)
        if rot.ndim != 2 or rot.shape[1] != 3 or rot.shape[0] != n:
            raise ValueError('rotations must have shape (n, 3), one per position')
    c = (np.asarray(box, dtype=np.float64) - 1.0) / 2.0
    ms = np.zeros((n, 4, 4), dtype=np.float64)
    for i in range(n):
        r3 = np.identity(3, dtype=np.float64) if rotations is None else \
            rotation_matrix(rot[i], rotation_units, rotation_order, dtype=np.float64)[:3, :3]
        ms[i, :3, :3] = r3
        ms[i, :3, 3] = pos[i] - r3 @ c
        ms[i, 3, 3] = 1.0
    return ms


def place_matrices(positions, rotations=None, box_shape=None, rotation_units: str = 'deg',
                   rotation_order: str = 'rzxz') -> np.ndarray:
    """Pull matrices (n, 4, 4), float64, that put ``n`` copies of a map of shape ``box_shape`` into a larger one
    (``StaticVolume.place``): the exact inverses of ``box_matrices(positions, rotations, box_shape, ...)``.

    With ``c = (box_shape - 1) / 2`` and ``R_i`` as in ``box_matrices``: ``P_i[:3, :3] = R_i^T`` and ``P_i[:3, 3] = c - R_i^T .
    positions[i]``, so output voxel ``positions[i]`` samples the centre of the map: copy ``i`` has its centre at ``positions[i]``, in
    the orientation that ``extract_at(positions, rotations)`` would undo.
    """
    box = _box_shape(box_shape)
    pos = np.asarray(positions, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
        raise ValueError('positions must have shape (n, 3)')
    n = pos.shape[0]
    if rotations is not None:
        rot = np.asarray(rotations, dtype=np.float64)
        if rot.ndim != 2 or rot.shape[1] != 3 or rot.shape[0] != n:
            raise ValueError('rotations must have shape (n, 3), one per position')
    c = (np.asarray(box, dtype=np.float64) - 1.0) / 2.0
    ms = np.zeros((n, 4, 4), dtype=np.float64)
    for i in range(n):
        r3 = np.identity(3, dtype=np.float64) if rotations is None else \
            rotation_matrix(rot[i], rotation_units, rotation_order, dtype=np.float64)[:3, :3]
        ms[i, :3, :3] = r3.T
        ms[i, :3, 3] = c - r3.T @ pos[i]
        ms[i, 3, 3] = 1.0
    return ms


def tilt_matrices(angles, tilt_axis: int = 1, shape=None, rotation_units: str = 'deg', center: Vec3 = None) -> np.ndarray:
    """Pull matrices (n, 4, 4) of a tilt series of a volume of shape ``shape`` (``StaticVolume.tilt_series``): matrix ``i`` is
    ``transform_matrix(rotation=r, rotation_order='sxyz', center=center)`` with ``r`` zero except ``r[tilt_axis] = angles[i]``,
    i.e. a turn about array axis ``tilt_axis`` (1 or 2: perpendicular to the projection axis, 0: in the image plane).
    ``center`` defaults to ``(shape - 1) / 2`` in float32, as in ``StaticVolume.project``.
    """
    if isinstance(tilt_axis, bool) or not isinstance(tilt_axis, (int, np.integer)) or not 0 <= tilt_axis <= 2:
        raise ValueError('tilt_axis must be 0, 1 or 2')
    a = np.asarray(angles, dtype=np.float64)
    if a.ndim != 1 or a.shape[0] == 0:
        raise ValueError('angles must be a non-empty sequence')
    if center is None:
        center = np.divide(np.subtract(_box_shape(shape), 1), 2, dtype=np.float32)
    ms = []
    for angle in a:
        r = [0.0, 0.0, 0.0]
        r[int(tilt_axis)] = float(angle)
        ms.append(transform_matrix(rotation=tuple(r), rotation_units=rotation_units, rotation_order='sxyz', center=center))
    return np.stack(ms)


def backproject_matrices(angles, tilt_axis: int = 1, output_shape=None, image_shape=None, rotation_units: str = 'deg',
                         center: Vec3 = None) -> np.ndarray:
    """Pull matrices (n, 4, 4), float64, that back-project a tilt series into a volume of shape ``output_shape``
    (``StaticVolume.backproject``): the inverses of ``tilt_matrices(angles, tilt_axis, output_shape, rotation_units, center)``, so rows
    1 and 2 of matrix ``i`` send a voxel index of the volume to the pixel of image ``i`` that ``tilt_series`` of that volume sums it into.

    ``image_shape`` (``(H, W)``, or ``(T, H, W)`` whose last two count): the images' own shape where it differs from
    ``output_shape[1:]``; ``(image_shape - 1) / 2 - (output_shape[1:] - 1) / 2`` is added to the translations of rows 1 and 2, which
    puts the centre of the volume's projection at the centre of the image.
    """
    out = _box_shape(output_shape)
    fwd = np.asarray(tilt_matrices(angles, tilt_axis, out, rotation_units, center), dtype=np.float64)
    ms = np.linalg.inv(fwd)
    ms[:, 3, :] = (0.0, 0.0, 0.0, 1.0)
    if image_shape is not None:
        try:
            img = tuple(image_shape)
        except TypeError:
            raise ValueError('image_shape must be (H, W) or (T, H, W), positive ints')
        if len(img) not in (2, 3) or not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) and b > 0 for b in img):
            raise ValueError('image_shape must be (H, W) or (T, H, W), positive ints')
        shift = (np.asarray(img[-2:], dtype=np.float64) - 1.0) / 2.0 - (np.asarray(out[1:], dtype=np.float64) - 1.0) / 2.0
        ms[:, 1, 3] += shift[0]
        ms[:, 2, 3] += shift[1]
    return ms


def backproject_box_matrices(positions, angles, tilt_axis: int = 1, volume_shape=None, box_shape=None, image_shape=None,
                             rotation_units: str = 'deg', center: Vec3 = None) -> np.ndarray:
    """Pull matrices (nb, n, 4, 4), float64, that back-project a tilt series into ``nb`` boxes of shape ``box_shape``
    (``StaticVolume.backproject_boxes``), box ``b`` being the region of the volume of shape ``volume_shape`` centred at
    ``positions[b]`` (voxel coordinates of that volume, fractional allowed).

    With ``M_i = backproject_matrices(angles, tilt_axis, volume_shape, image_shape, rotation_units, center)[i]`` and ``c = (box_shape -
    1) / 2``, entry ``(b, i)`` has ``M_i``'s linear part and the translation ``M_i[:3, 3] + M_i[:3, :3] . (positions[b] - c)``: voxel
    ``v`` of box ``b`` is voxel ``v + positions[b] - c`` of the full back-projection.
    """
    if volume_shape is None or box_shape is None:
        raise ValueError('volume_shape and box_shape are required')
    box = _box_shape(box_shape)
    pos = np.asarray(positions, dtype=np.float64)
    if pos.ndim != 2 or pos.shape[1] != 3 or pos.shape[0] == 0:
        raise ValueError('positions must have shape (nb, 3)')
    m = backproject_matrices(angles, tilt_axis, volume_shape, image_shape, rotation_units, center)
    c = (np.asarray(box, dtype=np.float64) - 1.0) / 2.0
    ms = np.empty((pos.shape[0],) + m.shape, dtype=np.float64)
    ms[:] = m
    # (nb, n, 3): M_i[:3, :3] . (positions[b] - c)
    ms[:, :, :3, 3] += np.einsum('irc,bc->bir', m[:, :3, :3], pos - c)
    return ms


def _image_shape(shape, name: str) -> Tuple[int, int]:
    """``(H, W)``, or ``(T, H, W)`` whose last two count: two positive ints, or ValueError."""
    try:
        s = tuple(shape)
    except TypeError:
        raise ValueError(f'{name} must be (H, W) or (T, H, W), positive ints')
    if len(s) not in (2, 3) or not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) and b > 0 for b in s):
        raise ValueError(f'{name} must be (H, W) or (T, H, W), positive ints')
    return int(s[-2]), int(s[-1])


def stack_matrices(shifts=None, rotations=None, scales=None, image_shape=None, output_shape=None,
                   rotation_units: str = 'deg') -> np.ndarray:
    """Pull matrices (n, 3, 3), float64, on ``(h, w, 1)`` for ``StaticVolume.affine_stack``: image ``i`` appears in the output turned by
    ``rotations[i]``, magnified by ``scales[i]`` about the centres and moved by ``shifts[i]``.

    With ``ci = (image_shape - 1) / 2``, ``co = (output_shape - 1) / 2`` and ``R = [[cos t, -sin t], [sin t, cos t]]`` on ``(y, x)``, output
    pixel ``p`` reads the image at ``q = ci + R^T . (p - co - shift_i) / s_i``.  ``shifts``: ``(n, 2)`` in pixels ``(y, x)``; ``rotations``:
    ``(n,)``; ``scales``: ``(n,)``, non-zero; None = no shift, no turn, scale 1.  At least one of them must be given (it fixes ``n``).
    ``image_shape`` (required) and ``output_shape`` (None = ``image_shape``): ``(H, W)``, or ``(T, H, W)`` whose last two count.
    """
    if rotation_units not in AVAILABLE_UNITS:
        raise ValueError(f'rotation_units must be one of {AVAILABLE_UNITS}')
    if image_shape is None:
        raise ValueError('image_shape is required')
    img = _image_shape(image_shape, 'image_shape')
    out = img if output_shape is None else _image_shape(output_shape, 'output_shape')
    given = [np.asarray(a, dtype=np.float64) for a in (shifts, rotations, scales) if a is not None]
    if not given:
        raise ValueError('one of shifts, rotations, scales must be given')
    n = given[0].shape[0] if given[0].ndim else 0
    sh = np.zeros((n, 2)) if shifts is None else np.asarray(shifts, dtype=np.float64)
    th = np.zeros(n) if rotations is None else np.asarray(rotations, dtype=np.float64)
    sc = np.ones(n) if scales is None else np.asarray(scales, dtype=np.float64)
    if n == 0 or sh.shape != (n, 2) or th.shape != (n,) or sc.shape != (n,):
        raise ValueError('shifts must have shape (n, 2), rotations and scales shape (n,), n > 0')
    if not (np.isfinite(sh).all() and np.isfinite(th).all() and np.isfinite(sc).all()) or (sc == 0).any():
        raise ValueError('shifts, rotations and scales must be finite, scales non-zero')
    if rotation_units == 'deg':
        th = np.deg2rad(th)
    ci = (np.asarray(img, dtype=np.float64) - 1.0) / 2.0
    co = (np.asarray(out, dtype=np.float64) - 1.0) / 2.0
    c, s = np.cos(th), np.sin(th)
    ms = np.zeros((n, 3, 3), dtype=np.float64)
    # R^T / s
    ms[:, 0, 0] = c / sc
    ms[:, 0, 1] = s / sc
    ms[:, 1, 0] = -s / sc
    ms[:, 1, 1] = c / sc
    ms[:, :2, 2] = ci - np.einsum('irc,ic->ir', ms[:, :2, :2], co + sh)
    ms[:, 2, 2] = 1.0
    return ms


def _box_shape(box_shape) -> Tuple[int, int, int]:
    """Three positive ints, or ValueError."""
    try:
        box = tuple(box_shape)
    except TypeError:
        raise ValueError('box_shape must be three positive ints')
    if len(box) != 3 or not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) and b > 0 for b in box):
        raise ValueError('box_shape must be three positive ints')
    return tuple(int(b) for b in box)


def grid_nodes(grid_shape, output_shape) -> np.ndarray:
    """Output coordinates of the nodes of a displacement grid (``StaticVolume.warp``): a float64 array ``(gD, gH, gW, 3)`` whose entry
    ``[i, j, k]`` is ``(i (oD - 1) / (gD - 1), j (oH - 1) / (gH - 1), k (oW - 1) / (gW - 1))`` -- the nodes span the output corner to
    corner.  An axis with one node (the field is constant along it) reports the middle of the output, ``(o - 1) / 2``.  Per axis either
    ``g == 1`` or ``2 <= g <= o``.  A caller writes ``displacements = f(grid_nodes(grid_shape, output_shape))``.
    """
    try:
        g = _box_shape(grid_shape)
        o = _box_shape(output_shape)
    except ValueError:
        raise ValueError('grid_shape and output_shape must be three positive ints each')
    axes = []
    for gk, ok in zip(g, o):
        if gk == 1:
            axes.append(np.array([(ok - 1) / 2.0]))
        elif 2 <= gk <= ok:
            axes.append(np.arange(gk, dtype=np.float64) * (ok - 1) / (gk - 1))
        else:
            raise ValueError(f'grid_shape {g}: per axis 1 node, or 2 up to the output size {o}')
    nodes = np.empty(g + (3,), dtype=np.float64)
    nodes[..., 0] = axes[0][:, None, None]
    nodes[..., 1] = axes[1][None, :, None]
    nodes[..., 2] = axes[2][None, None, :]
    return nodes


def stack_grid_nodes(grid_shape, output_shape) -> np.ndarray:
    """Output coordinates of the nodes of a 2-D displacement grid (``StaticVolume.warp_stack``): a float64 array ``(gH, gW, 2)`` whose
    entry ``[j, k]`` is ``(j (Ho - 1) / (gH - 1), k (Wo - 1) / (gW - 1))`` -- the nodes span the output image corner to corner.  The 2-D
    ``grid_nodes``, with its convention for an axis of one node: the middle of the output, ``(o - 1) / 2``.  Per axis either ``g == 1`` or
    ``2 <= g <= o``.
    """
    try:
        g, o = tuple(grid_shape), tuple(output_shape)
    except TypeError:
        raise ValueError('grid_shape and output_shape must be two positive ints each')
    if len(g) != 2 or len(o) != 2:
        raise ValueError('grid_shape and output_shape must be two positive ints each')
    return grid_nodes((1,) + g, (1,) + o)[0, :, :, 1:]
