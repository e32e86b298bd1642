"""``StaticVolume``: upload (and prefilter) once, transform many times.

API mirror of ``/root/reference/voltools/volume.py:13-165``.  On a GPU device the constructor hands the
data to ``vt_volume_create`` (upload + one-time three-pass prefilter for ``filt_*``), and every
``affine`` is one 64-byte matrix hand-over plus one kernel launch (``volume.py:61-91``).  ``reshape`` is not
available here, as in the reference (``volume.py:14-16``).
"""
import ctypes
import time
from typing import Tuple, Union

import numpy as np
from scipy.ndimage import affine_transform, convolve1d, map_coordinates, spline_filter

from . import _native
from .transforms import affine as _affine, AVAILABLE_INTERPOLATIONS, _INTERPOLATIONS, _triple, _scipy_arguments
from .utils import (scale_matrix, shear_matrix, rotation_matrix, translation_matrix, transform_matrix, box_matrices, place_matrices, tilt_matrices,
                    backproject_matrices, backproject_box_matrices, stack_matrices, ramp_taps, patch_bounds, peak_shifts, patch_moments, normalized_scores,
                    get_available_devices, switch_to_device)
from .utils.matrices import _box_shape

Vec3 = Union[Tuple[float, float, float], np.ndarray]


def _warp_coordinates(disp: np.ndarray, m: np.ndarray, shape) -> np.ndarray:
    """Source coordinates ``(3, oD, oH, oW)``, float64, of ``StaticVolume.warp``: ``M . v`` plus the trilinear interpolation of the float32
    grid ``disp`` -- per axis ``q = v (g - 1) / (o - 1)``, cell ``c = min(floor(q), g - 2)``, ``f = q - c``, lerps ``a + f (b - a)`` along
    axis 2, then 1, then 0 (the order of the GPU kernel; numpy rounds the product and the sum separately, a difference of an ulp)."""
    u = disp.astype(np.float64)
    for axis in (2, 1, 0):
        g, o = u.shape[axis], shape[axis]
        if g == 1:
            u = np.repeat(u, o, axis=axis) if o > 1 else u
            continue
        q = np.arange(o, dtype=np.float64) * ((g - 1) / (o - 1))
        c = np.minimum(np.floor(q).astype(np.int64), g - 2)
        f = (q - c).reshape([-1 if k == axis else 1 for k in range(4)])
        a, b = np.take(u, c, axis=axis), np.take(u, c + 1, axis=axis)
        u = a + f * (b - a)
    d, h, w = (np.arange(n, dtype=np.float64) for n in shape)
    coords = np.empty((3,) + tuple(shape), dtype=np.float64)
    for r in range(3):
        coords[r] = (m[r, 0] * d[:, None, None] + (m[r, 1] * h[None, :, None] + (m[r, 2] * w[None, None, :] + m[r, 3]))) + u[..., r]
    return coords


def _warp_stack_coordinates(disp: np.ndarray, m: np.ndarray, shape):
    """Source coordinates ``(y, x)``, float64 ``(Ho, Wo)`` each, of one entry of ``StaticVolume.warp_stack``: rows 1 and 2 of ``M`` on
    ``(h, w, 1)`` plus the bilinear interpolation of the float32 grid ``disp`` ``(gH, gW, 2)`` -- ``_warp_coordinates`` in two dimensions,
    lerps along axis 1 of the grid (x), then axis 0 (y)."""
    u = disp.astype(np.float64)
    for axis in (1, 0):
        g, o = u.shape[axis], shape[axis]
        if g == 1:
            u = np.repeat(u, o, axis=axis) if o > 1 else u
            continue
        q = np.arange(o, dtype=np.float64) * ((g - 1) / (o - 1))
        c = np.minimum(np.floor(q).astype(np.int64), g - 2)
        f = (q - c).reshape([-1 if k == axis else 1 for k in range(3)])
        a, b = np.take(u, c, axis=axis), np.take(u, c + 1, axis=axis)
        u = a + f * (b - a)
    h, w = (np.arange(n, dtype=np.float64) for n in shape)
    yy = (m[1, 1] * h[:, None] + (m[1, 2] * w[None, :] + m[1, 3])) + u[..., 0]
    xx = (m[2, 1] * h[:, None] + (m[2, 2] * w[None, :] + m[2, 3])) + u[..., 1]
    return yy, xx


def _window_and_grid(max_shift, patch_grid, H: int, W: int):
    """``((Rh, Rw), (gH, gW))`` of the stack calls that take a shift window and a patch grid, checked against images ``(H, W)``."""
    def pair(val, name):
        try:
            a, b = val
        except (TypeError, ValueError):
            raise ValueError(f'{name} must be a pair of ints') from None
        for x in (a, b):
            if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
                raise ValueError(f'{name} must be a pair of ints')
        return int(a), int(b)
    rh, rw = pair(max_shift, 'max_shift')
    gh, gw = pair(patch_grid, 'patch_grid')
    if not (0 <= rh <= H - 1 and 0 <= rw <= W - 1):
        raise ValueError(f'max_shift must lie inside [0, {H - 1}] x [0, {W - 1}]')
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError(f'patch_grid must lie inside [1, {H}] x [1, {W}]')
    return (rh, rw), (gh, gw)


def _plane_indices(val, name: str, T: int) -> np.ndarray:
    """A non-empty vector of image indices inside ``[0, T)`` as contiguous int32."""
    a = np.asarray(val)
    if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f'{name} must be a vector of integers')
    if a.min() < 0 or a.max() >= T:
        raise ValueError(f'{name} must lie inside [0, {T})')
    return np.ascontiguousarray(a, dtype=np.int32)


class StaticVolume:
    """For StaticVolume transforms the boolean reshape cannot be given as an argument."""

    def __init__(self, data, interpolation: str = 'linear', device: str = 'gpu', *, edge: str = 'texture', max_resident_bytes: int = 0,
                 stack: bool = False):
        """``edge`` (extension, GPU devices): ``'texture'`` = the reference GPU path's boundary contract, ``'scipy'`` = the
        contract of its CPU path (see ``transforms.py`` of this package).  ``max_resident_bytes`` (extension, GPU devices): how much HBM
        this volume may keep resident, its plain copy included -- the copies built lazily per orientation used (``info().resident_bytes``)
        are released least recently used first to stay inside it, and a copy that cannot fit is not built (the call then runs on the
        kernels that sample the plain layout; results are the same).  0 = no limit (or the ``VT_MAX_RESIDENT_GB`` environment default).
        The reference keeps one CUDA array per StaticVolume (``volume.py:37-45``).  ``stack`` (extension): the planes are independent
        images, a tilt series for ``backproject``; ``filt_*`` interpolations then prefilter inside each plane only (``spline_filter`` per
        plane on ``device='cpu'``), and such a volume serves the back-projections, ``affine_stack`` / ``align_stack`` and ``warp_stack`` alone.  With the other interpolations
        the flag changes nothing.  Not together with ``edge='scipy'``."""
        if data.ndim != 3:
            raise ValueError('Expected a 3D array')
        if edge not in ('texture', 'scipy'):
            raise ValueError("edge must be 'texture' or 'scipy'")
        if not isinstance(stack, (bool, np.bool_)):
            raise ValueError('stack must be a bool')
        if stack and edge == 'scipy':
            raise ValueError("stack=True cannot be combined with edge='scipy'")
        self.edge = edge
        self.stack = bool(stack)
        if device not in get_available_devices():
            raise ValueError(f'Unknown device ({device}), must be one of {get_available_devices()}')

        self.device = device
        self.interpolation = interpolation
        self.shape = tuple(int(s) for s in data.shape)
        self._handle = None

        if device.startswith('gpu'):
            if interpolation not in _INTERPOLATIONS:
                raise ValueError(f'Interpolation must be one of {AVAILABLE_INTERPOLATIONS}')
            self._dev = switch_to_device(device)
            self._lib = _native.load()
            iface = getattr(data, '__cuda_array_interface__', None)
            if iface is not None and not isinstance(data, np.ndarray):
                ptr, is_dev, _ = _native.resolve_output(data, self.shape, self._dev)
                flags = _native.SRC_DEVICE
            else:
                host = np.ascontiguousarray(data, dtype=np.float32)
                ptr, flags = host.ctypes.data, 0
            if edge == 'scipy':
                flags |= _native.EDGE_SCIPY
            if self.stack:
                flags |= _native.STACK
            h = ctypes.c_void_p()
            _native.check(self._lib.vt_volume_create(self._dev, *self.shape, _INTERPOLATIONS[interpolation],
                                                     ptr, flags, ctypes.byref(h)), 'vt_volume_create')
            self._handle = h
            self.d_type = np.dtype(np.float32)
            if max_resident_bytes:
                self.set_max_resident(int(max_resident_bytes))
        elif device == 'cpu':
            self.data = data

    # -- lifetime ---------------------------------------------------------------------------------
    def close(self) -> None:
        if getattr(self, '_handle', None):
            self._lib.vt_volume_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- introspection (no reference counterpart; used by bench.py and the tests) ------------------
    def info(self) -> _native.VolumeInfo:
        info = _native.VolumeInfo()
        _native.check(self._lib.vt_volume_info(self._handle, ctypes.byref(info)), 'vt_volume_info')
        return info

    def release_copies(self) -> int:
        """Free the resident copies this volume built lazily besides its plain one (exchanged orientations, plane-quad forms); they are
        rebuilt on demand.  Returns the bytes freed.  (No reference counterpart: the reference holds one CUDA array, volume.py:37-45.)"""
        if self.device == 'cpu':
            return 0
        freed = ctypes.c_uint64()
        _native.check(self._lib.vt_volume_release_copies(self._handle, ctypes.byref(freed)), 'vt_volume_release_copies')
        return int(freed.value)

    def set_max_resident(self, nbytes: int) -> None:
        """Change the resident-memory budget (bytes, the plain copy included; 0 = none).  See ``__init__``."""
        if self.device != 'cpu':
            _native.check(self._lib.vt_volume_set_max_resident(self._handle, ctypes.c_uint64(int(nbytes))), 'vt_volume_set_max_resident')

    def synchronize(self) -> None:
        _native.check(self._lib.vt_volume_sync(self._handle), 'vt_volume_sync')

    def timer_start(self) -> None:
        _native.check(self._lib.vt_timer_start(self._handle), 'vt_timer_start')

    def timer_stop(self) -> float:
        ms = ctypes.c_float()
        _native.check(self._lib.vt_timer_stop(self._handle, ctypes.byref(ms)), 'vt_timer_stop')
        return ms.value

    # -- the hot call -------------------------------------------------------------------------------
    def affine(self, transform_m: np.ndarray, profile: bool = False, output=None,
               keep_outside: bool = False, _flags: int = 0) -> Union[np.ndarray, None]:
        if self.device == 'cpu':
            return _affine(self.data, transform_m, interpolation=self.interpolation, profile=profile,
                           output=output, device=self.device)

        m = np.asarray(transform_m)
        flags = _flags | (_native.KEEP_OUTSIDE if keep_outside else 0)
        if output is None:
            result = _native.host_result(self.shape, self._dev)
            ptr, is_dev, fill = result.ctypes.data, False, None
            flags &= ~_native.KEEP_OUTSIDE        # a fresh buffer is zero outside (volume.py:73)
        else:
            ptr, is_dev, fill = _native.resolve_output(output, self.shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE

        if profile:
            self.timer_start()
        if m.dtype == np.float64:
            m64 = np.ascontiguousarray(m.reshape(4, 4))
            rc = self._lib.vt_volume_affine_f64(self._handle, m64.ctypes.data, ptr, flags)
        else:
            m32 = np.ascontiguousarray(m, dtype=np.float32).reshape(4, 4)
            rc = self._lib.vt_volume_affine(self._handle, m32.ctypes.data, ptr, flags)
        _native.check(rc, 'vt_volume_affine')
        if profile:
            print(f'transform finished in {self.timer_stop():.3f}ms')
        return result        # None when output= was given (volume.py:91)

    def transform(self, scale: Union[float, Vec3] = None, shear: Union[float, Vec3] = None,
                  rotation: Vec3 = None, rotation_units: str = 'deg', rotation_order: str = 'rzxz',
                  translation: Vec3 = None, center: Vec3 = None, profile: bool = False,
                  output=None) -> Union[np.ndarray, None]:
        if center is None:
            center = np.divide(np.subtract(self.shape, 1), 2, dtype=np.float32)
        m = transform_matrix(_triple(scale), _triple(shear), rotation, rotation_units, rotation_order,
                             translation, center)
        return self.affine(m, profile, output)


    def affine_batch(self, matrices: np.ndarray, profile: bool = False, output=None,
                     _flags: int = 0) -> Union[np.ndarray, None]:
        """``affine`` for a stack of matrices (n, 4, 4) in one call.  Returns a float32 array
        (n, D, H, W), or fills ``output`` of that shape (numpy or device array) and returns None.  Small volumes
        (<= 96^3: template rotations) are served by a single kernel launch."""
        ms = np.ascontiguousarray(np.asarray(matrices, dtype=np.float32))
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        n = ms.shape[0]
        shape = (n,) + tuple(self.shape)
        if self.device == 'cpu':
            res = np.stack([_affine(self.data, m, interpolation=self.interpolation, device='cpu') for m in ms])
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        _native.check(self._lib.vt_volume_affine_batch(self._handle, n, ms.ctypes.data, ptr, flags), 'vt_volume_affine_batch')
        if profile:
            print(f'{n} transforms finished in {self.timer_stop():.3f}ms')
        return result

    # -- sub-volume extraction (extension: scipy's output_shape, transforms.py:136-150, per matrix and in one launch) ----
    def extract(self, matrices: np.ndarray, box_shape, profile: bool = False, output=None, *,
                _flags: int = 0) -> Union[np.ndarray, None]:
        """``n`` boxes of shape ``box_shape = (bd, bh, bw)`` cut out of the volume, each through its own pull matrix:
        box ``i`` is what ``affine(matrices[i])`` would return if the output shape were ``box_shape`` --
        ``src = M_i[:3, :3] . (d, h, w) + M_i[:3, 3]`` with ``(d, h, w)`` the voxel index inside the box.  Voxels that map outside
        the volume are 0.  Returns a float32 array ``(n, bd, bh, bw)``, or fills ``output`` of that shape (numpy, ``vt.empty`` device
        array, torch-ROCm tensor) and returns None on a GPU device, like ``affine_batch``.  Box ``i`` depends on ``matrices[i]`` only,
        bit for bit.  float64 matrices keep their precision; anything else is taken as float32."""
        box = _box_shape(box_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        shape = (n,) + box
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            data = self.data
            if prefilter:       # what affine_transform(prefilter=True) does first (mode='constant'), once instead of per box
                data = spline_filter(data, order, output=np.float64, mode='constant')
            res = np.empty(shape, dtype=self.data.dtype if np.issubdtype(self.data.dtype, np.floating) else np.float64)
            t_start = time.time()
            for i in range(n):
                affine_transform(data, ms[i], output_shape=box, output=res[i], order=order, prefilter=False)
            if profile:
                print(f'{n} boxes extracted in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_extract_f64(self._handle, n, ms.ctypes.data, *box, ptr, flags)
        else:
            rc = self._lib.vt_volume_extract(self._handle, n, ms.ctypes.data, *box, ptr, flags)
        _native.check(rc, 'vt_volume_extract')
        if profile:
            print(f'{n} boxes extracted in {self.timer_stop():.3f}ms')
        return result

    # -- resampling through a displacement grid (extension: what scipy.ndimage.map_coordinates is to affine_transform) ----
    def warp(self, displacements, matrix=None, output_shape=None, profile: bool = False, output=None, *,
             _flags: int = 0) -> Union[np.ndarray, None]:
        """The volume resampled through a map that need not be affine: ``out[v] = sample(src, M . v + u(v))`` for every voxel ``v = (d, h,
        w)`` of an output of shape ``output_shape`` (default: the volume's).  ``displacements`` is a control grid ``(gD, gH, gW, 3)`` of
        displacement vectors in source voxels along array axes 0, 1, 2, taken as float32; its nodes span the output corner to corner
        (``utils.grid_nodes``), ``u(v)`` is their trilinear interpolation in float64.  Per axis either one node (constant along that axis) or
        2 up to the output size; a grid of the output's shape is a dense field.  ``matrix`` is a 4 x 4 pull matrix, None for the identity;
        float64 keeps its precision, anything else is taken as float32.  Voxels that map outside the volume are 0.  Returns a float32
        array of ``output_shape``, or fills ``output`` of that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None
        on a GPU device.  ``device='cpu'`` evaluates the same float64 coordinates in numpy and hands them to
        ``scipy.ndimage.map_coordinates``."""
        shape = _box_shape(self.shape if output_shape is None else output_shape)
        disp = np.asarray(displacements)
        if disp.ndim != 4 or disp.shape[3] != 3:
            raise ValueError('displacements must have shape (gD, gH, gW, 3)')
        if not all(g == 1 or 2 <= g <= o for g, o in zip(disp.shape[:3], shape)):
            raise ValueError(f'displacements of grid shape {disp.shape[:3]}: per axis 1 node, or 2 up to the output size {shape}')
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        if matrix is not None:
            m = np.asarray(matrix)
            if m.shape != (4, 4):
                raise ValueError('matrix must have shape (4, 4)')
            m = np.ascontiguousarray(m, dtype=np.float64 if m.dtype == np.float64 else np.float32)
        else:
            m = None
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            data = self.data
            if prefilter:
                data = spline_filter(data, order, output=np.float64, mode='constant')
            t_start = time.time()
            coords = _warp_coordinates(disp, np.eye(4) if m is None else m.astype(np.float64), shape)
            res = map_coordinates(data, coords, order=order, mode='constant', cval=0, prefilter=False)
            res = res.astype(self.data.dtype if np.issubdtype(self.data.dtype, np.floating) else np.float64, copy=False)
            if profile:
                print(f'warp finished in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        mptr = None if m is None else m.ctypes.data
        if m is not None and m.dtype == np.float64:
            rc = self._lib.vt_volume_warp_f64(self._handle, mptr, disp.ctypes.data, *disp.shape[:3], *shape, ptr, flags)
        else:
            rc = self._lib.vt_volume_warp(self._handle, mptr, disp.ctypes.data, *disp.shape[:3], *shape, ptr, flags)
        _native.check(rc, 'vt_volume_warp')
        if profile:
            print(f'warp finished in {self.timer_stop():.3f}ms')
        return result

    def extract_at(self, positions, rotations=None, box_shape=None, rotation_units: str = 'deg',
                   rotation_order: str = 'rzxz', profile: bool = False, output=None) -> Union[np.ndarray, None]:
        """``extract`` of boxes centred at ``positions`` (n, 3), each turned by ``rotations[i]`` (n, 3; none: axis-aligned crops):
        the matrices of ``utils.box_matrices``, in float64."""
        return self.extract(box_matrices(positions, rotations, box_shape, rotation_units, rotation_order), box_shape,
                            profile, output)

    # -- weighted sum of extracted boxes (extension: sub-tomogram averaging, symmetrisation; no reference counterpart) ----
    def extract_sum(self, matrices: np.ndarray, box_shape, weights=None, profile: bool = False, output=None, *,
                    _flags: int = 0) -> Union[np.ndarray, None]:
        """``float32(sum_i weights[i] * extract(matrices, box_shape)[i])`` without writing the boxes: one box of shape ``box_shape``.
        Every sample is widened to float64, multiplied by its float64 weight and added in float64, in the order of ``matrices``; the sum is
        rounded to float32 once.  ``weights``: shape ``(n,)``, converted to float64; None = ones.  Returns a float32 array ``(bd, bh, bw)``,
        or fills ``output`` of that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like
        ``extract``.  Repeated calls give identical bits.  float64 matrices keep their precision; anything else is taken as float32."""
        box = _box_shape(box_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f'weights must have shape ({n},)')
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        if output is not None and tuple(getattr(output, 'shape', ())) != box:
            raise ValueError(f'output must have shape {box}')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            data = self.data
            if prefilter:       # what affine_transform(prefilter=True) does first (mode='constant'), once instead of per box
                data = spline_filter(data, order, output=np.float64, mode='constant')
            one = np.empty(box, dtype=self.data.dtype if np.issubdtype(self.data.dtype, np.floating) else np.float64)
            acc = np.zeros(box, dtype=np.float64)
            t_start = time.time()
            for i in range(n):
                affine_transform(data, ms[i], output_shape=box, output=one, order=order, prefilter=False)
                acc += w[i] * one.astype(np.float64)
            res = acc.astype(np.float32)
            if profile:
                print(f'{n} boxes summed in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(box, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, box, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_extract_sum_f64(self._handle, n, ms.ctypes.data, w.ctypes.data, *box, ptr, flags)
        else:
            rc = self._lib.vt_volume_extract_sum(self._handle, n, ms.ctypes.data, w.ctypes.data, *box, ptr, flags)
        _native.check(rc, 'vt_volume_extract_sum')
        if profile:
            print(f'{n} boxes summed in {self.timer_stop():.3f}ms')
        return result

    def average_at(self, positions, rotations=None, box_shape=None, weights=None, rotation_units: str = 'deg',
                   rotation_order: str = 'rzxz', profile: bool = False, output=None) -> Union[np.ndarray, None]:
        """Weighted average of the boxes ``extract_at`` would cut: ``extract_sum`` of ``utils.box_matrices(...)`` with ``weights``
        (None: ones) divided by their sum on the host in float64."""
        ms = box_matrices(positions, rotations, box_shape, rotation_units, rotation_order)
        w = np.ones(ms.shape[0], dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
        if w.shape != (ms.shape[0],):
            raise ValueError(f'weights must have shape ({ms.shape[0]},)')
        total = w.sum()
        if not np.isfinite(w).all() or total == 0:
            raise ValueError('weights must be finite and must not sum to 0')
        return self.extract_sum(ms, box_shape, w / total, profile, output)

    # -- posed, weighted copies of this map summed into one larger map (extension: place-back, synthetic tomograms, particle subtraction) ----
    def place(self, matrices: np.ndarray, output_shape, weights=None, profile: bool = False, output=None, *,
              accumulate: bool = False, _flags: int = 0) -> Union[np.ndarray, None]:
        """``n`` copies of this volume put into one map of shape ``output_shape = (oD, oH, oW)``, copy ``i`` through its pull matrix
        (output voxel index -> coordinate in this volume, ``src = P_i[:3, :3] . (d, h, w) + P_i[:3, 3]``; ``utils.place_matrices`` builds
        them from positions and rotations): ``out = float32(b + sum_i weights[i] * A_i)`` with ``A_i`` what ``affine(matrices[i])`` would
        return at that output shape (0 outside the copy) and ``b`` zero, or with ``accumulate=True`` the contents of ``output``, which is
        then required (negative weights subtract copies from a map).  Every term is widened to float64, multiplied by its float64 weight
        and added in float64, in the order of ``matrices``; the sum is rounded to float32 once: ``extract_sum(matrices, output_shape,
        weights)`` evaluates the same expression.  On a GPU device only the output tiles a copy can reach are computed, so the cost
        follows the volume covered, not ``n`` x the output volume; with ``accumulate`` every voxel outside those tiles keeps its bits.
        ``weights``: shape ``(n,)``, converted to float64; None = ones.  Returns a float32 array ``(oD, oH, oW)``, or fills ``output`` of
        that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like ``extract_sum``.  Repeated
        calls give identical bits.  float64 matrices keep their precision; anything else is taken as float32."""
        shape = _box_shape(output_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f'weights must have shape ({n},)')
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        if accumulate and output is None:
            raise ValueError('accumulate=True adds into output, which must be given')
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            data = self.data
            if prefilter:       # what affine_transform(prefilter=True) does first (mode='constant'), once instead of per copy
                data = spline_filter(data, order, output=np.float64, mode='constant')
            one = np.empty(shape, dtype=self.data.dtype if np.issubdtype(self.data.dtype, np.floating) else np.float64)
            acc = np.asarray(output).astype(np.float64) if accumulate else np.zeros(shape, dtype=np.float64)
            t_start = time.time()
            for i in range(n):
                affine_transform(data, ms[i], output_shape=shape, output=one, order=order, prefilter=False)
                acc += w[i] * one.astype(np.float64)
            res = acc.astype(np.float32)
            if profile:
                print(f'{n} copies placed in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags | (_native.ACCUMULATE if accumulate else 0)
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_place_f64(self._handle, n, ms.ctypes.data, w.ctypes.data, *shape, ptr, flags)
        else:
            rc = self._lib.vt_volume_place(self._handle, n, ms.ctypes.data, w.ctypes.data, *shape, ptr, flags)
        _native.check(rc, 'vt_volume_place')
        if profile:
            print(f'{n} copies placed in {self.timer_stop():.3f}ms')
        return result

    def place_at(self, positions, rotations=None, output_shape=None, weights=None, rotation_units: str = 'deg',
                 rotation_order: str = 'rzxz', profile: bool = False, output=None, *, accumulate: bool = False) -> Union[np.ndarray, None]:
        """``place`` of copies centred at ``positions`` (n, 3) of the output, copy ``i`` in the orientation ``extract_at(positions,
        rotations)`` would undo (none: axis-aligned): the matrices of ``utils.place_matrices`` for this volume's shape, in float64."""
        return self.place(place_matrices(positions, rotations, self.shape, rotation_units, rotation_order), output_shape, weights,
                          profile, output, accumulate=accumulate)

    # -- G weighted sums of the same boxes (extension: class averages, half-set maps, bootstrap replicas; no reference counterpart) ----
    def extract_sum_multi(self, matrices: np.ndarray, box_shape, weights, profile: bool = False, output=None, *,
                          _flags: int = 0) -> Union[np.ndarray, None]:
        """``G`` weighted sums of the same ``n`` boxes, each box sampled once: ``out[j] = float32(sum_i weights[i, j] *
        extract(matrices, box_shape)[i])`` without writing the boxes.  ``weights``: shape ``(n, G)`` with G >= 1, converted to float64,
        finite.  Box ``j`` holds the bits ``extract_sum(matrices, box_shape, weights[:, j])`` gives (all samples finite): it does not
        depend on G, on the other columns or on the column's place.  Returns a float32 array ``(G, bd, bh, bw)``, or fills ``output`` of
        that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like ``extract_sum``.
        float64 matrices keep their precision; anything else is taken as float32."""
        box = _box_shape(box_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        w = np.ascontiguousarray(weights, dtype=np.float64)
        if w.ndim != 2 or w.shape[0] != n or w.shape[1] < 1:
            raise ValueError(f'weights must have shape ({n}, G) with G >= 1')
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        g = w.shape[1]
        shape = (g,) + box
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            data = self.data
            if prefilter:       # what affine_transform(prefilter=True) does first (mode='constant'), once instead of per box
                data = spline_filter(data, order, output=np.float64, mode='constant')
            one = np.empty(box, dtype=self.data.dtype if np.issubdtype(self.data.dtype, np.floating) else np.float64)
            acc = np.zeros(shape, dtype=np.float64)
            t_start = time.time()
            for i in range(n):
                affine_transform(data, ms[i], output_shape=box, output=one, order=order, prefilter=False)
                one64 = one.astype(np.float64)
                for j in range(g):
                    acc[j] += w[i, j] * one64
            res = acc.astype(np.float32)
            if profile:
                print(f'{n} boxes summed into {g} in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_extract_sum_multi_f64(self._handle, n, ms.ctypes.data, g, w.ctypes.data, *box, ptr, flags)
        else:
            rc = self._lib.vt_volume_extract_sum_multi(self._handle, n, ms.ctypes.data, g, w.ctypes.data, *box, ptr, flags)
        _native.check(rc, 'vt_volume_extract_sum_multi')
        if profile:
            print(f'{n} boxes summed into {g} in {self.timer_stop():.3f}ms')
        return result

    def class_averages_at(self, positions, rotations=None, box_shape=None, labels=None, weights=None, n_classes=None,
                          rotation_units: str = 'deg', rotation_order: str = 'rzxz', profile: bool = False,
                          output=None) -> Union[np.ndarray, None]:
        """``G`` weighted averages of the boxes ``extract_at`` would cut, in one ``extract_sum_multi`` call: the step of a classification
        round that follows ``correlate_templates_at``.  Exactly one of ``labels`` (integers ``(n,)`` in ``[0, n_classes)``; ``n_classes``
        defaults to ``max + 1``) or ``weights`` (``(n, G)`` float64) must be given.  Each column is divided by its sum on the host in
        float64, as ``average_at`` does; a column whose sum is 0 stays all zero, so an empty class gives a zero box."""
        ms = box_matrices(positions, rotations, box_shape, rotation_units, rotation_order)
        n = ms.shape[0]
        if (labels is None) == (weights is None):
            raise ValueError('exactly one of labels and weights must be given')
        if labels is not None:
            lab = np.asarray(labels)
            if lab.shape != (n,) or not np.issubdtype(lab.dtype, np.integer):
                raise ValueError(f'labels must be integers of shape ({n},)')
            g = int(lab.max()) + 1 if n_classes is None else int(n_classes)
            if g < 1 or lab.min() < 0 or lab.max() >= g:
                raise ValueError(f'labels must lie in [0, {g})')
            w = np.zeros((n, g), dtype=np.float64)
            w[np.arange(n), lab] = 1.0
        else:
            w = np.array(weights, dtype=np.float64)
            if w.ndim != 2 or w.shape[0] != n or w.shape[1] < 1:
                raise ValueError(f'weights must have shape ({n}, G) with G >= 1')
            if n_classes is not None and int(n_classes) != w.shape[1]:
                raise ValueError(f'n_classes = {n_classes} does not match weights of shape {w.shape}')
            if not np.isfinite(w).all():
                raise ValueError('weights must be finite')
        total = w.sum(axis=0)
        if not np.isfinite(total).all():
            raise ValueError('weights must be finite')
        nz = total != 0
        w[:, nz] = w[:, nz] / total[nz]
        w[:, ~nz] = 0.0
        return self.extract_sum_multi(ms, box_shape, w, profile, output)

    # -- per-box template scores (extension: alignment search, template-matching refinement, classification; no reference counterpart) ----
    def extract_dot(self, matrices: np.ndarray, template, mask=None, profile: bool = False, output=None, *,
                    _flags: int = 0) -> Union[np.ndarray, None]:
        """Three float64 sums over each box ``B_i = extract(matrices, template.shape)[i]`` without writing the boxes:
        ``out[i] = (sum(mask * B_i), sum(mask * B_i**2), sum(template * B_i))``.  ``template`` (3-D; its shape is the box shape) and
        ``mask`` (same shape; None = ones) are converted to contiguous float32 and must be finite.  Every sample is widened to float64
        and added in a fixed order: ``out[i]`` depends on ``matrices[i]``, the template and the mask only, bit for bit, and repeated
        calls give identical bits.  Returns a float64 array ``(n, 3)``, or fills ``output`` of that shape (C-contiguous numpy float64,
        or a torch-ROCm float64 tensor on the volume's device) and returns None on a GPU device (``device='cpu'`` returns ``output``, like ``extract``).  float64 matrices keep their
        precision; anything else is taken as float32."""
        tmpl = np.ascontiguousarray(template, dtype=np.float32)
        if tmpl.ndim != 3:
            raise ValueError('template must be a 3-D array (its shape is the box shape)')
        box = _box_shape(tmpl.shape)
        msk = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
        if msk is not None and msk.shape != box:
            raise ValueError(f'mask must have the template\'s shape {box}')
        if not np.isfinite(tmpl).all() or (msk is not None and not np.isfinite(msk).all()):
            raise ValueError('template and mask must be finite')
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        shape = (n, 3)
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            if output is not None and not (isinstance(output, np.ndarray) and output.dtype == np.float64):
                raise ValueError(f'output must be a float64 array of shape {shape}')
            t_start = time.time()
            boxes = self.extract(ms, box).astype(np.float64)
            t64 = tmpl.astype(np.float64)
            m64 = np.ones(box, dtype=np.float64) if msk is None else msk.astype(np.float64)
            res = np.stack([(m64 * boxes).sum(axis=(1, 2, 3)), (m64 * boxes * boxes).sum(axis=(1, 2, 3)),
                            (t64 * boxes).sum(axis=(1, 2, 3))], axis=1)
            if profile:
                print(f'{n} boxes scored in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = np.empty(shape, dtype=np.float64)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev, dtype=np.float64)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        mptr = None if msk is None else msk.ctypes.data
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_extract_dot_f64(self._handle, n, ms.ctypes.data, tmpl.ctypes.data, mptr, *box, ptr, flags)
        else:
            rc = self._lib.vt_volume_extract_dot(self._handle, n, ms.ctypes.data, tmpl.ctypes.data, mptr, *box, ptr, flags)
        _native.check(rc, 'vt_volume_extract_dot')
        if profile:
            print(f'{n} boxes scored in {self.timer_stop():.3f}ms')
        return result

    def correlate_at(self, positions, rotations=None, template=None, mask=None, rotation_units: str = 'deg',
                     rotation_order: str = 'rzxz', profile: bool = False) -> np.ndarray:
        """Locally normalised cross-correlation coefficient of ``template`` (under ``mask``; None = ones) with each of the boxes
        ``extract_at(positions, rotations, template.shape)`` would cut, as float64 ``(n,)``.  On the host, in float64: ``N = sum(mask)``,
        ``t = template - sum(mask * template) / N``, ``sigma_t = sqrt(sum(mask * t**2) / N)``; ``extract_dot`` with the template
        ``float32(mask * t / (N * sigma_t))`` gives ``S0, S1, S2``, and ``cc = S2 / sqrt(S1 / N - (S0 / N)**2)`` (0 where the box has
        no variance under the mask).  Because ``sum(mask * t) = 0`` the box mean needs no subtraction."""
        if template is None:
            raise ValueError('correlate_at needs a template')
        t64 = np.asarray(template, dtype=np.float64)
        if t64.ndim != 3:
            raise ValueError('template must be a 3-D array (its shape is the box shape)')
        m64 = np.ones(t64.shape, dtype=np.float64) if mask is None else np.asarray(mask, dtype=np.float32).astype(np.float64)   # the mask the kernel reads
        if m64.shape != t64.shape:
            raise ValueError(f'mask must have the template\'s shape {t64.shape}')
        if not np.isfinite(t64).all() or not np.isfinite(m64).all():
            raise ValueError('template and mask must be finite')
        N = m64.sum()
        if N == 0:
            raise ValueError('the mask sums to 0')
        that = t64 - (m64 * t64).sum() / N
        sigma_t = np.sqrt((m64 * that * that).sum() / N)
        if not sigma_t > 0:
            raise ValueError('the template has no variance under the mask')
        tmpl = (m64 * that / (N * sigma_t)).astype(np.float32)
        ms = box_matrices(positions, rotations, t64.shape, rotation_units, rotation_order)
        s = self.extract_dot(ms, tmpl, None if mask is None else m64.astype(np.float32), profile)
        var = s[:, 1] / N - (s[:, 0] / N) ** 2
        cc = np.zeros(s.shape[0], dtype=np.float64)
        ok = var > 0
        cc[ok] = s[ok, 2] / np.sqrt(var[ok])
        return cc

    # -- per-box scores against a stack of templates (extension: multi-reference classification and template matching) ----
    def extract_dot_multi(self, matrices: np.ndarray, templates, mask=None, profile: bool = False, output=None, *,
                          _flags: int = 0) -> Union[np.ndarray, None]:
        """``extract_dot`` against K templates under one mask, each box staged and sampled once: ``out[i] = (sum(mask * B_i),
        sum(mask * B_i**2), sum(templates[0] * B_i), .., sum(templates[K-1] * B_i))`` with ``B_i = extract(matrices, box)[i]``.
        ``templates`` is 4-D ``(K, d, h, w)`` (``templates.shape[1:]`` is the box shape), ``mask`` has the box shape (None = ones); both
        are converted to contiguous float32 and must be finite.  Columns 0, 1 and ``2 + j`` hold exactly the bits
        ``extract_dot(matrices, templates[j], mask)`` gives in its columns 0, 1, 2: a column depends on ``matrices[i]``, its template and
        the mask only.  Returns a float64 array ``(n, 2 + K)``, or fills ``output`` of that shape (C-contiguous numpy float64, or a
        torch-ROCm float64 tensor on the volume's device) and returns None on a GPU device (``device='cpu'`` returns ``output``), like
        ``extract_dot``.  float64 matrices keep their precision; anything else is taken as float32."""
        tmpls = np.ascontiguousarray(templates, dtype=np.float32)
        if tmpls.ndim != 4 or tmpls.shape[0] == 0:
            raise ValueError('templates must be a non-empty 4-D stack (K, d, h, w); its trailing shape is the box shape')
        K = tmpls.shape[0]
        box = _box_shape(tmpls.shape[1:])
        msk = None if mask is None else np.ascontiguousarray(mask, dtype=np.float32)
        if msk is not None and msk.shape != box:
            raise ValueError(f'mask must have the templates\' shape {box}')
        if not np.isfinite(tmpls).all() or (msk is not None and not np.isfinite(msk).all()):
            raise ValueError('templates and mask must be finite')
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        shape = (n, 2 + K)
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            if output is not None and not (isinstance(output, np.ndarray) and output.dtype == np.float64):
                raise ValueError(f'output must be a float64 array of shape {shape}')
            t_start = time.time()
            boxes = self.extract(ms, box).astype(np.float64)
            m64 = np.ones(box, dtype=np.float64) if msk is None else msk.astype(np.float64)
            cols = [(m64 * boxes).sum(axis=(1, 2, 3)), (m64 * boxes * boxes).sum(axis=(1, 2, 3))]
            cols += [(tmpls[j].astype(np.float64) * boxes).sum(axis=(1, 2, 3)) for j in range(K)]      # extract_dot's expressions
            res = np.stack(cols, axis=1)
            if profile:
                print(f'{n} boxes scored against {K} templates in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = np.empty(shape, dtype=np.float64)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev, dtype=np.float64)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        mptr = None if msk is None else msk.ctypes.data
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_extract_dot_multi_f64(self._handle, n, ms.ctypes.data, K, tmpls.ctypes.data, mptr, *box, ptr, flags)
        else:
            rc = self._lib.vt_volume_extract_dot_multi(self._handle, n, ms.ctypes.data, K, tmpls.ctypes.data, mptr, *box, ptr, flags)
        _native.check(rc, 'vt_volume_extract_dot_multi')
        if profile:
            print(f'{n} boxes scored against {K} templates in {self.timer_stop():.3f}ms')
        return result

    def correlate_templates_at(self, positions, rotations=None, templates=None, mask=None, rotation_units: str = 'deg',
                               rotation_order: str = 'rzxz', profile: bool = False) -> np.ndarray:
        """``correlate_at`` against K templates under one mask with one ``extract_dot_multi`` call: float64 ``(n, K)``, column ``j``
        equal to ``correlate_at(positions, rotations, templates[j], mask)`` bit for bit.  Every template is normalised on the host as
        ``correlate_at`` normalises its one (``N = sum(mask)``, ``t = template - sum(mask * template) / N``, ``sigma_t = sqrt(sum(mask *
        t**2) / N)``, ``float32(mask * t / (N * sigma_t))``); then ``cc[i, j] = T_j / sqrt(S1 / N - (S0 / N)**2)``, 0 where the box has
        no variance under the mask."""
        if templates is None:
            raise ValueError('correlate_templates_at needs templates')
        t64 = np.asarray(templates, dtype=np.float64)
        if t64.ndim != 4 or t64.shape[0] == 0:
            raise ValueError('templates must be a non-empty 4-D stack (K, d, h, w); its trailing shape is the box shape')
        box = t64.shape[1:]
        m64 = np.ones(box, dtype=np.float64) if mask is None else np.asarray(mask, dtype=np.float32).astype(np.float64)   # the mask the kernel reads
        if m64.shape != box:
            raise ValueError(f'mask must have the templates\' shape {box}')
        if not np.isfinite(t64).all() or not np.isfinite(m64).all():
            raise ValueError('templates and mask must be finite')
        N = m64.sum()
        if N == 0:
            raise ValueError('the mask sums to 0')
        tmpls = np.empty(t64.shape, dtype=np.float32)
        for j in range(t64.shape[0]):
            that = t64[j] - (m64 * t64[j]).sum() / N
            sigma_t = np.sqrt((m64 * that * that).sum() / N)
            if not sigma_t > 0:
                raise ValueError(f'template {j} has no variance under the mask')
            tmpls[j] = (m64 * that / (N * sigma_t)).astype(np.float32)
        ms = box_matrices(positions, rotations, box, rotation_units, rotation_order)
        s = self.extract_dot_multi(ms, tmpls, None if mask is None else m64.astype(np.float32), profile)
        var = s[:, 1] / N - (s[:, 0] / N) ** 2
        cc = np.zeros((s.shape[0], t64.shape[0]), dtype=np.float64)
        ok = var > 0
        cc[ok] = s[ok, 2:] / np.sqrt(var[ok])[:, None]
        return cc

    # -- projection (examples/projections.py:20-26 does transform(...).sum(axis=0)) -------
    def projection(self, transform_m: np.ndarray, profile: bool = False, output=None,
                   _flags: int = 0) -> Union[np.ndarray, None]:
        """``affine(transform_m).sum(axis=0)`` without materialising the transformed volume.

        Returns a float32 (H, W) numpy array, or fills ``output`` (numpy / device array of that shape) and returns
        None, like ``affine``.  Rotations about axis 0 (the example's ``rotation=(i, 0, 0)``, ``'sxyz'``) cost one
        streaming pass over the resident volume plus a 2-D interpolation."""
        shape2 = tuple(self.shape[1:])
        if self.device == 'cpu':
            vol = _affine(self.data, transform_m, interpolation=self.interpolation, profile=profile, device='cpu')
            proj = vol.sum(axis=0, dtype=np.float64).astype(np.float32)
            if output is None:
                return proj
            output[...] = proj
            return output

        m = np.asarray(transform_m)
        flags = _flags
        if output is None:
            result = np.empty(shape2, dtype=np.float32)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape2, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        if m.dtype == np.float64:
            m64 = np.ascontiguousarray(m.reshape(4, 4))
            rc = self._lib.vt_volume_project_f64(self._handle, m64.ctypes.data, ptr, flags)
        else:
            m32 = np.ascontiguousarray(m, dtype=np.float32).reshape(4, 4)
            rc = self._lib.vt_volume_project(self._handle, m32.ctypes.data, ptr, flags)
        _native.check(rc, 'vt_volume_project')
        if profile:
            print(f'projection finished in {self.timer_stop():.3f}ms')
        return result

    def project(self, scale: Union[float, Vec3] = None, shear: Union[float, Vec3] = None,
                rotation: Vec3 = None, rotation_units: str = 'deg', rotation_order: str = 'rzxz',
                translation: Vec3 = None, center: Vec3 = None, profile: bool = False,
                output=None) -> Union[np.ndarray, None]:
        """``transform(...)`` followed by ``sum(axis=0)`` (same arguments as ``transform``)."""
        if center is None:
            center = np.divide(np.subtract(self.shape, 1), 2, dtype=np.float32)
        m = transform_matrix(_triple(scale), _triple(shear), rotation, rotation_units, rotation_order,
                             translation, center)
        return self.projection(m, profile, output)

    # -- a stack of projections per call (extension: the loop of examples/projections.py:20-26 for any rotation axis) ----
    def projection_batch(self, matrices: np.ndarray, output_shape=None, profile: bool = False, output=None, *,
                         _flags: int = 0) -> Union[np.ndarray, None]:
        """``n`` projections in one call: image ``i`` is ``affine(matrices[i])`` at output shape ``output_shape = (depth, H, W)``
        (default: the volume's shape) summed over axis 0, without materialising any transformed volume.  Returns a float32 array
        ``(n, H, W)``, or fills ``output`` of that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU
        device, like ``extract``.  Image ``i`` depends on ``matrices[i]`` only, bit for bit.  float64 matrices keep their precision;
        anything else is taken as float32."""
        oshape = tuple(self.shape) if output_shape is None else _box_shape(output_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        shape = (n,) + oshape[1:]
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            data = self.data
            if prefilter:       # what affine_transform(prefilter=True) does first (mode='constant'), once instead of per matrix
                data = spline_filter(data, order, output=np.float64, mode='constant')
            res = np.empty(shape, dtype=np.float32)
            vol = np.empty(oshape, dtype=self.data.dtype if np.issubdtype(self.data.dtype, np.floating) else np.float64)
            t_start = time.time()
            for i in range(n):
                affine_transform(data, ms[i], output_shape=oshape, output=vol, order=order, prefilter=False)
                res[i] = vol.sum(axis=0, dtype=np.float64)
            if profile:
                print(f'{n} projections finished in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_project_batch_f64(self._handle, n, ms.ctypes.data, *oshape, ptr, flags)
        else:
            rc = self._lib.vt_volume_project_batch(self._handle, n, ms.ctypes.data, *oshape, ptr, flags)
        _native.check(rc, 'vt_volume_project_batch')
        if profile:
            print(f'{n} projections finished in {self.timer_stop():.3f}ms')
        return result

    def tilt_series(self, angles, tilt_axis: int = 1, rotation_units: str = 'deg', center: Vec3 = None, output_shape=None,
                    profile: bool = False, output=None) -> Union[np.ndarray, None]:
        """``projection_batch`` of the volume turned about array axis ``tilt_axis`` by each of ``angles``: the matrices of
        ``utils.tilt_matrices``.  ``tilt_series([a], k)[0]`` is the image of ``project(rotation=r, rotation_order='sxyz')`` with
        ``r[k] = a``."""
        return self.projection_batch(tilt_matrices(angles, tilt_axis, self.shape, rotation_units, center), output_shape, profile, output)

    # -- back-projection: a stack of images summed into one volume (extension: the transpose of projection_batch; WBP, SIRT) ----
    def backproject(self, matrices: np.ndarray, output_shape, weights=None, profile: bool = False, output=None, *,
                    planes=None, accumulate: bool = False, _flags: int = 0) -> Union[np.ndarray, None]:
        """This volume taken as a stack of ``T`` images ``(T, H, W)`` and back-projected into one volume of shape ``output_shape =
        (oD, oH, oW)``: ``out = float32(b + sum_i weights[i] * B_i)`` with ``B_i[d, h, w]`` image ``planes[i]`` interpolated in two
        dimensions at ``y = M_i[1, :3] . (d, h, w) + M_i[1, 3]``, ``x = M_i[2, :3] . (d, h, w) + M_i[2, 3]`` (rows 0 and 3 of a matrix are
        ignored; ``utils.backproject_matrices`` builds the matrices of a tilt series), 0 outside the image, and ``b`` zero, or with
        ``accumulate=True`` the contents of ``output``, which is then required.  The interpolation is the volume's, in the plane: bilinear,
        or the 4 x 4 cubic B-spline; ``filt_*`` needs a volume built with ``stack=True``.  Every term is widened to float64, multiplied by
        its float64 weight and added in float64, in the order of ``matrices``; the sum is rounded to float32 once.
        ``planes``: ``n`` image indices inside ``[0, T)``; None = ``0 .. n-1``, and then ``n`` must equal ``T``.  ``weights``: shape
        ``(n,)``, converted to float64; None = ones.  Returns a float32 array ``(oD, oH, oW)``, or fills ``output`` of that shape (numpy,
        ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like ``place``.  Repeated calls give identical
        bits.  float64 matrices keep their precision; anything else is taken as float32."""
        shape = _box_shape(output_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] != (4, 4) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        n = ms.shape[0]
        w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f'weights must have shape ({n},)')
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        if planes is None:
            if n != self.shape[0]:
                raise ValueError(f'{n} matrices for a stack of {self.shape[0]} images: planes must be given')
            pl = None
        else:
            pl = np.asarray(planes)
            if pl.shape != (n,) or not np.issubdtype(pl.dtype, np.integer):
                raise ValueError(f'planes must be {n} integers')
            if pl.min() < 0 or pl.max() >= self.shape[0]:
                raise ValueError(f'planes must lie inside [0, {self.shape[0]})')
            pl = np.ascontiguousarray(pl, dtype=np.int32)
        if accumulate and output is None:
            raise ValueError('accumulate=True adds into output, which must be given')
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_') and not self.stack:
            raise ValueError('back-projection with a filt_* interpolation needs in-plane coefficients: build the volume with stack=True')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            acc = np.asarray(output).astype(np.float64) if accumulate else np.zeros(shape, dtype=np.float64)
            d, h, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape), indexing='ij')
            coeffs = {}
            t_start = time.time()
            for i in range(n):
                k = i if pl is None else int(pl[i])
                if k not in coeffs:     # spline_filter per plane: the planes are independent images
                    img = np.asarray(self.data[k], dtype=np.float64)
                    coeffs[k] = spline_filter(img, order, output=np.float64, mode='constant') if prefilter else img
                m = ms[i].astype(np.float64)
                yy = m[1, 0] * d + m[1, 1] * h + m[1, 2] * x + m[1, 3]
                xx = m[2, 0] * d + m[2, 1] * h + m[2, 2] * x + m[2, 3]
                one = map_coordinates(coeffs[k], [yy, xx], order=order, mode='constant', cval=0.0, prefilter=False, output=np.float64)
                acc += w[i] * one.astype(np.float32).astype(np.float64)
            res = acc.astype(np.float32)
            if profile:
                print(f'{n} images back-projected in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags | (_native.ACCUMULATE if accumulate else 0)
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        pl_ptr = None if pl is None else pl.ctypes.data
        if ms.dtype == np.float64:
            rc = self._lib.vt_volume_backproject_f64(self._handle, n, ms.ctypes.data, pl_ptr, w.ctypes.data, *shape, ptr, flags)
        else:
            rc = self._lib.vt_volume_backproject(self._handle, n, ms.ctypes.data, pl_ptr, w.ctypes.data, *shape, ptr, flags)
        _native.check(rc, 'vt_volume_backproject')
        if profile:
            print(f'{n} images back-projected in {self.timer_stop():.3f}ms')
        return result

    def backproject_tilts(self, angles, tilt_axis: int = 1, rotation_units: str = 'deg', center: Vec3 = None, output_shape=None,
                          weights=None, profile: bool = False, output=None, *, accumulate: bool = False) -> Union[np.ndarray, None]:
        """``backproject`` of this stack as the tilt series ``tilt_series(angles, tilt_axis, ...)`` of a volume of shape ``output_shape``
        (required) would give: image ``i`` belongs to ``angles[i]``; the matrices of ``utils.backproject_matrices`` for this stack's image
        shape, in float64."""
        if output_shape is None:
            raise ValueError('output_shape is required')
        ms = backproject_matrices(angles, tilt_axis, output_shape, self.shape[1:], rotation_units, center)
        return self.backproject(ms, output_shape, weights, profile, output, accumulate=accumulate)

    # -- nb boxes of one shape back-projected from the stack in one launch (extension: per-particle reconstruction from a tilt series) ----
    def backproject_boxes(self, matrices: np.ndarray, box_shape, weights=None, profile: bool = False, output=None, *,
                          planes=None, accumulate: bool = False, _flags: int = 0,
                          _max_table_bytes: int = 256 << 20) -> Union[np.ndarray, None]:
        """``nb`` sub-volumes of shape ``box_shape = (bD, bH, bW)`` from this stack of ``T`` images, ``n`` entries each: ``matrices`` has
        shape ``(nb, n, 4, 4)`` and entry ``(b, i)`` sends a voxel index inside box ``b`` to a pixel of image ``planes[i]`` (rows 1 and 2
        count; ``utils.backproject_box_matrices`` builds them from positions and tilt angles).  Box ``b`` holds exactly what
        ``backproject(matrices[b], box_shape, weights[b], planes=planes, accumulate=...)`` gives, bit for bit on a GPU device, whatever
        ``nb``, the other boxes and its place in the batch are -- in one kernel launch instead of ``nb``.
        ``planes``: ``n`` image indices shared by all boxes; None = ``0 .. n-1``, and then ``n`` must equal ``T``.  ``weights``: shape
        ``(n,)``, used for every box, or ``(nb, n)``; converted to float64; None = ones.  Returns a float32 array ``(nb, bD, bH, bW)``, or
        fills ``output`` of that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like
        ``backproject``; ``accumulate=True`` adds into ``output``, which is then required.  float64 matrices keep their precision;
        anything else is taken as float32.  The library receives 200 bytes of tables per (box, entry); beyond ``_max_table_bytes`` the
        call is cut along the box axis into several library calls on consecutive slices of the output, which cannot show in the
        result."""
        box = _box_shape(box_shape)
        ms = np.asarray(matrices)
        if ms.ndim != 4 or ms.shape[2:] != (4, 4) or ms.shape[0] == 0 or ms.shape[1] == 0:
            raise ValueError('matrices must have shape (nb, n, 4, 4)')
        ms = np.ascontiguousarray(ms, dtype=np.float64 if ms.dtype == np.float64 else np.float32)
        nb, n = ms.shape[:2]
        if weights is None:
            w = np.ones((nb, n), dtype=np.float64)
        else:
            w = np.asarray(weights, dtype=np.float64)
            if w.shape == (n,):
                w = np.broadcast_to(w, (nb, n))
            elif w.shape != (nb, n):
                raise ValueError(f'weights must have shape ({n},) or ({nb}, {n})')
            w = np.ascontiguousarray(w)
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        if planes is None:
            if n != self.shape[0]:
                raise ValueError(f'{n} matrices per box for a stack of {self.shape[0]} images: planes must be given')
            pl = None
        else:
            pl = np.asarray(planes)
            if pl.shape != (n,) or not np.issubdtype(pl.dtype, np.integer):
                raise ValueError(f'planes must be {n} integers')
            if pl.min() < 0 or pl.max() >= self.shape[0]:
                raise ValueError(f'planes must lie inside [0, {self.shape[0]})')
            pl = np.ascontiguousarray(pl, dtype=np.int32)
        shape = (nb,) + box
        if accumulate and output is None:
            raise ValueError('accumulate=True adds into output, which must be given')
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_') and not self.stack:
            raise ValueError('back-projection with a filt_* interpolation needs in-plane coefficients: build the volume with stack=True')
        if not isinstance(_max_table_bytes, (int, np.integer)) or isinstance(_max_table_bytes, bool) or _max_table_bytes <= 0:
            raise ValueError('_max_table_bytes must be a positive int')
        if self.device == 'cpu':
            res = np.empty(shape, dtype=np.float32)
            t_start = time.time()
            for b in range(nb):      # the CPU backproject of that box's matrices, as it stands
                if accumulate:
                    res[b] = np.asarray(output[b])
                    self.backproject(ms[b], box, w[b], output=res[b], planes=pl, accumulate=True)
                else:
                    res[b] = self.backproject(ms[b], box, w[b], planes=pl)
            if profile:
                print(f'{nb} boxes back-projected from {n} images in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags | (_native.ACCUMULATE if accumulate else 0)
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        pl_ptr = None if pl is None else pl.ctypes.data
        f64 = ms.dtype == np.float64
        call = self._lib.vt_volume_backproject_boxes_f64 if f64 else self._lib.vt_volume_backproject_boxes
        per_call = max(1, int(_max_table_bytes) // (200 * n))      # boxes per library call: 192-byte entry + 8-byte weight per pair
        box_bytes = 4 * box[0] * box[1] * box[2]
        for b0 in range(0, nb, per_call):
            k = min(per_call, nb - b0)
            rc = call(self._handle, k, n, ms.ctypes.data + b0 * n * 16 * ms.itemsize, pl_ptr, w.ctypes.data + b0 * n * 8, *box,
                      ptr + b0 * box_bytes, flags)
            _native.check(rc, 'vt_volume_backproject_boxes')
        if profile:
            print(f'{nb} boxes back-projected from {n} images in {self.timer_stop():.3f}ms')
        return result

    def backproject_boxes_at(self, positions, angles, tilt_axis: int = 1, volume_shape=None, box_shape=None,
                             rotation_units: str = 'deg', center: Vec3 = None, weights=None, profile: bool = False, output=None, *,
                             accumulate: bool = False) -> Union[np.ndarray, None]:
        """``backproject_boxes`` of this stack as the tilt series of a volume of shape ``volume_shape`` (required): box ``b``, of shape
        ``box_shape`` (required), is the region of ``backproject_tilts(angles, tilt_axis, ..., output_shape=volume_shape)`` centred at
        ``positions[b]`` (voxel coordinates of that volume, fractional allowed), without the volume ever being formed.  Image ``i`` belongs
        to ``angles[i]``; the matrices are ``utils.backproject_box_matrices`` for this stack's image shape, in float64."""
        if volume_shape is None or box_shape is None:
            raise ValueError('volume_shape and box_shape are required')
        ms = backproject_box_matrices(positions, angles, tilt_axis, volume_shape, box_shape, self.shape[1:], rotation_units, center)
        return self.backproject_boxes(ms, box_shape, weights, profile, output, accumulate=accumulate)

    # -- per-image 2-D transforms of the stack: a stack in, a stack out (extension: tilt alignment, movie frames, regridding) ----
    def affine_stack(self, matrices: np.ndarray, output_shape=None, weights=None, profile: bool = False, output=None, *,
                     planes=None, _flags: int = 0) -> Union[np.ndarray, None]:
        """This volume taken as a stack of ``T`` images ``(T, H, W)``, each resampled under its own 2-D affine map: ``out[i, h, w] =
        float32(weights[i] * B_i[h, w])`` with ``B_i[h, w]`` image ``planes[i]`` interpolated in two dimensions at ``(y, x, 1) = M_i . (h,
        w, 1)``, 0 outside the image -- ``backproject``'s definition for one entry and an output of depth 1, one image per entry instead of
        their sum.  ``matrices``: ``(n, 3, 3)`` homogeneous pull matrices on ``(h, w, 1)`` (``utils.stack_matrices`` builds them from
        shifts, rotations and scales), embedded into rows and columns 1, 2, 3 of a 4 x 4 matrix; or ``(n, 4, 4)`` as ``backproject`` takes
        them, of which rows 1 and 2 and columns 1, 2, 3 count.  ``output_shape``: ``(Ho, Wo)``, None = ``(H, W)``.  The interpolation is the
        volume's, in the plane: bilinear, or the 4 x 4 cubic B-spline; ``filt_*`` needs a volume built with ``stack=True``.
        ``planes``: ``n`` image indices inside ``[0, T)``; None = ``0 .. n-1``, and then ``n`` must equal ``T``.  ``weights``: shape
        ``(n,)``, converted to float64; None = ones.  Returns a float32 array ``(n, Ho, Wo)``, or fills ``output`` of that shape (numpy,
        ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like ``backproject``.  An image does not depend on
        the rest of the batch, and repeated calls give identical bits.  float64 matrices keep their precision; anything else is taken as
        float32."""
        ms = np.asarray(matrices)
        if ms.ndim != 3 or ms.shape[1:] not in ((3, 3), (4, 4)) or ms.shape[0] == 0:
            raise ValueError('matrices must have shape (n, 3, 3) or (n, 4, 4)')
        dtype = np.float64 if ms.dtype == np.float64 else np.float32
        if ms.shape[1:] == (3, 3):
            m4 = np.zeros((ms.shape[0], 4, 4), dtype=dtype)
            m4[:, 0, 0] = 1
            m4[:, 1:, 1:] = ms
            ms = m4
        ms = np.ascontiguousarray(ms, dtype=dtype)
        n = ms.shape[0]
        try:
            hw = tuple(self.shape[1:]) if output_shape is None else tuple(output_shape)
        except TypeError:
            raise ValueError('output_shape must be two positive ints')
        if len(hw) != 2 or not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) and b > 0 for b in hw):
            raise ValueError('output_shape must be two positive ints')
        shape = (n, int(hw[0]), int(hw[1]))
        w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f'weights must have shape ({n},)')
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        if planes is None:
            if n != self.shape[0]:
                raise ValueError(f'{n} matrices for a stack of {self.shape[0]} images: planes must be given')
            pl = None
        else:
            pl = np.asarray(planes)
            if pl.shape != (n,) or not np.issubdtype(pl.dtype, np.integer):
                raise ValueError(f'planes must be {n} integers')
            if pl.min() < 0 or pl.max() >= self.shape[0]:
                raise ValueError(f'planes must lie inside [0, {self.shape[0]})')
            pl = np.ascontiguousarray(pl, dtype=np.int32)
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_') and not self.stack:
            raise ValueError('affine_stack with a filt_* interpolation needs in-plane coefficients: build the volume with stack=True')
        if self.device == 'cpu':
            order, prefilter = _scipy_arguments(self.interpolation)
            res = np.empty(shape, dtype=np.float32)
            h, x = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in shape[1:]), indexing='ij')
            coeffs = {}
            t_start = time.time()
            for i in range(n):
                k = i if pl is None else int(pl[i])
                if k not in coeffs:     # spline_filter per plane: the planes are independent images
                    img = np.asarray(self.data[k], dtype=np.float64)
                    coeffs[k] = spline_filter(img, order, output=np.float64, mode='constant') if prefilter else img
                m = ms[i].astype(np.float64)
                yy = m[1, 1] * h + m[1, 2] * x + m[1, 3]
                xx = m[2, 1] * h + m[2, 2] * x + m[2, 3]
                one = map_coordinates(coeffs[k], [yy, xx], order=order, mode='constant', cval=0.0, prefilter=False, output=np.float64)
                res[i] = (0.0 + w[i] * one.astype(np.float32).astype(np.float64)).astype(np.float32)
            if profile:
                print(f'{n} images resampled in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        pl_ptr = None if pl is None else pl.ctypes.data
        fn = self._lib.vt_volume_affine_stack_f64 if ms.dtype == np.float64 else self._lib.vt_volume_affine_stack
        _native.check(fn(self._handle, n, ms.ctypes.data, pl_ptr, w.ctypes.data, shape[1], shape[2], ptr, flags), 'vt_volume_affine_stack')
        if profile:
            print(f'{n} images resampled in {self.timer_stop():.3f}ms')
        return result

    def align_stack(self, shifts=None, rotations=None, scales=None, output_shape=None, rotation_units: str = 'deg', weights=None,
                    profile: bool = False, output=None, *, planes=None) -> Union[np.ndarray, None]:
        """``affine_stack`` with the matrices of ``utils.stack_matrices`` for this stack's image shape: image ``planes[i]`` (None: ``i``)
        appears in output image ``i`` turned by ``rotations[i]``, magnified by ``scales[i]`` about the centres and moved by
        ``shifts[i]`` pixels ``(y, x)``; float64 matrices."""
        ms = stack_matrices(shifts, rotations, scales, self.shape[1:], output_shape, rotation_units)
        return self.affine_stack(ms, output_shape, weights, profile, output, planes=planes)

    def _warp_stack_arguments(self, displacements, matrices, output_shape, planes, take_weights):
        """What ``warp_stack`` and ``warp_stack_sum`` share: the checked arguments ``(disp, shared, ms, n, shape, gshape, w, pl)``.
        ``take_weights(n)`` checks and returns the call's weights; it runs where ``warp_stack`` has always checked them."""
        disp = np.asarray(displacements)
        if disp.ndim not in (3, 4) or disp.shape[-1] != 2 or 0 in disp.shape:
            raise ValueError('displacements must have shape (n, gH, gW, 2) or (gH, gW, 2)')
        shared = disp.ndim == 3
        disp = np.ascontiguousarray(disp, dtype=np.float32)
        if matrices is not None:
            ms = np.asarray(matrices)
            if ms.ndim != 3 or ms.shape[1:] not in ((3, 3), (4, 4)) or ms.shape[0] == 0:
                raise ValueError('matrices must have shape (n, 3, 3) or (n, 4, 4)')
            dtype = np.float64 if ms.dtype == np.float64 else np.float32
            if ms.shape[1:] == (3, 3):
                m4 = np.zeros((ms.shape[0], 4, 4), dtype=dtype)
                m4[:, 0, 0] = 1
                m4[:, 1:, 1:] = ms
                ms = m4
            ms = np.ascontiguousarray(ms, dtype=dtype)
            n = ms.shape[0]
        else:
            ms = None
            n = self.shape[0] if shared else disp.shape[0]
        if not shared and disp.shape[0] != n:
            raise ValueError(f'{disp.shape[0]} grids for {n} entries: one grid per entry, or one shared grid (gH, gW, 2)')
        try:
            hw = tuple(self.shape[1:]) if output_shape is None else tuple(output_shape)
        except TypeError:
            raise ValueError('output_shape must be two positive ints')
        if len(hw) != 2 or not all(isinstance(b, (int, np.integer)) and not isinstance(b, bool) and b > 0 for b in hw):
            raise ValueError('output_shape must be two positive ints')
        shape = (n, int(hw[0]), int(hw[1]))
        gshape = disp.shape[-3:-1]
        if not all(g == 1 or 2 <= g <= o for g, o in zip(gshape, shape[1:])):
            raise ValueError(f'displacements of grid shape {gshape}: per axis 1 node, or 2 up to the output size {shape[1:]}')
        if not np.isfinite(disp).all():
            raise ValueError('displacements must be finite')
        w = take_weights(n)
        if planes is None:
            if n != self.shape[0]:
                raise ValueError(f'{n} entries for a stack of {self.shape[0]} images: planes must be given')
            pl = None
        else:
            pl = np.asarray(planes)
            if pl.shape != (n,) or not np.issubdtype(pl.dtype, np.integer):
                raise ValueError(f'planes must be {n} integers')
            if pl.min() < 0 or pl.max() >= self.shape[0]:
                raise ValueError(f'planes must lie inside [0, {self.shape[0]})')
            pl = np.ascontiguousarray(pl, dtype=np.int32)
        return disp, shared, ms, n, shape, gshape, w, pl

    def _warp_stack_cpu_samples(self, disp, shared, ms, n, shape, pl):
        """The ``device='cpu'`` samples of ``warp_stack`` and ``warp_stack_sum``: entry by entry the float32 image ``B_i``, unweighted."""
        order, prefilter = _scipy_arguments(self.interpolation)
        coeffs = {}
        for i in range(n):
            k = i if pl is None else int(pl[i])
            if k not in coeffs:     # spline_filter per plane: the planes are independent images
                img = np.asarray(self.data[k], dtype=np.float64)
                coeffs[k] = spline_filter(img, order, output=np.float64, mode='constant') if prefilter else img
            yy, xx = _warp_stack_coordinates(disp if shared else disp[i], np.eye(4) if ms is None else ms[i].astype(np.float64), shape[1:])
            one = map_coordinates(coeffs[k], [yy, xx], order=order, mode='constant', cval=0.0, prefilter=False, output=np.float64)
            yield one.astype(np.float32)

    def warp_stack(self, displacements, matrices=None, output_shape=None, weights=None, profile: bool = False, output=None, *,
                   planes=None, _flags: int = 0) -> Union[np.ndarray, None]:
        """``affine_stack`` with a 2-D displacement field per image: ``out[i, h, w] = float32(weights[i] * B_i[h, w])`` with ``B_i[h, w]``
        image ``planes[i]`` interpolated in two dimensions at ``(y, x) = M_i . (h, w, 1) + u_i(h, w)``, 0 outside the image.
        ``displacements``: control grids ``(n, gH, gW, 2)``, or ``(gH, gW, 2)`` for one grid shared by every entry, taken as float32;
        component 0 moves ``y``, component 1 moves ``x``, in source pixels.  The nodes span the output image corner to corner
        (``utils.stack_grid_nodes``), ``u_i`` is their bilinear interpolation in float64 -- ``warp``'s grid rule on axes 1 and 2.  Per axis
        either one node or 2 up to the output size; a grid of the output's shape is a dense field.  ``matrices``: None for the identity,
        or ``(n, 3, 3)`` / ``(n, 4, 4)`` as ``affine_stack`` takes them; float64 keeps its precision.  ``n`` is the number of matrices if
        given, else the number of grids, else ``T``.  ``output_shape``, ``planes``, ``weights`` and ``output`` are ``affine_stack``'s.
        Returns a float32 array ``(n, Ho, Wo)``, or fills ``output`` and returns None on a GPU device.  An image does not depend on the
        rest of the batch.  ``device='cpu'`` evaluates the same float64 coordinates in numpy and hands them to
        ``scipy.ndimage.map_coordinates`` per entry."""
        def take_weights(n):
            w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
            if w.shape != (n,):
                raise ValueError(f'weights must have shape ({n},)')
            if not np.isfinite(w).all():
                raise ValueError('weights must be finite')
            return w
        disp, shared, ms, n, shape, gshape, w, pl = self._warp_stack_arguments(displacements, matrices, output_shape, planes, take_weights)
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_') and not self.stack:
            raise ValueError('warp_stack with a filt_* interpolation needs in-plane coefficients: build the volume with stack=True')
        if self.device == 'cpu':
            res = np.empty(shape, dtype=np.float32)
            t_start = time.time()
            for i, one in enumerate(self._warp_stack_cpu_samples(disp, shared, ms, n, shape, pl)):
                res[i] = (0.0 + w[i] * one.astype(np.float64)).astype(np.float32)
            if profile:
                print(f'{n} images warped in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        pl_ptr = None if pl is None else pl.ctypes.data
        m_ptr = None if ms is None else ms.ctypes.data
        fn = self._lib.vt_volume_warp_stack_f64 if ms is not None and ms.dtype == np.float64 else self._lib.vt_volume_warp_stack
        _native.check(fn(self._handle, n, m_ptr, disp.ctypes.data, 1 if shared else n, gshape[0], gshape[1], pl_ptr, w.ctypes.data,
                         shape[1], shape[2], ptr, flags), 'vt_volume_warp_stack')
        if profile:
            print(f'{n} images warped in {self.timer_stop():.3f}ms')
        return result

    def warp_stack_sum(self, displacements, matrices=None, output_shape=None, weights=None, profile: bool = False, output=None, *,
                       planes=None, accumulate: bool = False, _flags: int = 0) -> Union[np.ndarray, None]:
        """The images ``warp_stack`` would write, summed without being written: ``out[c] = float32(b + sum_i W[i, c] * B_i)`` with ``B_i``
        ``warp_stack``'s unweighted float32 image ``i``, summed in float64 in ascending ``i`` (each product rounded, then each sum) and
        rounded once -- the motion-corrected sum of a movie.  ``displacements``, ``matrices``, ``output_shape`` and ``planes`` are
        ``warp_stack``'s.  ``weights``: None (ones) or ``(n,)`` for one sum, returned as ``(Ho, Wo)``; or ``(n, G)`` for ``G`` sums from
        one sampling of every image (all frames, even and odd frames, exposure windows), returned as ``(G, Ho, Wo)``; float64.
        ``accumulate=True`` starts the sums from ``output`` as found (``b``), which must then be given; else ``b = 0``.  A sum does
        not depend on ``G``, on the other columns or on its place among them.  Returns a float32 array, or fills ``output`` of that
        shape and returns None on a GPU device.  ``device='cpu'`` sums the samples of its own ``warp_stack(weights=None)`` by the same
        expression."""
        holder = {}

        def take_weights(n):
            w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
            if w.ndim not in (1, 2) or w.shape[0] != n or 0 in w.shape:
                raise ValueError(f'weights must have shape ({n},) or ({n}, G)')
            if not np.isfinite(w).all():
                raise ValueError('weights must be finite')
            holder['single'] = w.ndim == 1
            return w.reshape(n, -1)
        disp, shared, ms, n, shape, gshape, w, pl = self._warp_stack_arguments(displacements, matrices, output_shape, planes, take_weights)
        g = w.shape[1]
        full = (g, shape[1], shape[2])
        oshape = full[1:] if holder['single'] else full
        if accumulate and output is None:
            raise ValueError('accumulate=True adds into output, which must be given')
        if output is not None and tuple(getattr(output, 'shape', ())) != oshape:
            raise ValueError(f'output must have shape {oshape}')
        if self.interpolation.startswith('filt_') and not self.stack:
            raise ValueError('warp_stack_sum with a filt_* interpolation needs in-plane coefficients: build the volume with stack=True')
        if self.device == 'cpu':
            t_start = time.time()
            acc = np.asarray(output, dtype=np.float32).astype(np.float64).reshape(full) if accumulate else np.zeros(full, dtype=np.float64)
            for i, one in enumerate(self._warp_stack_cpu_samples(disp, shared, ms, n, shape, pl)):
                s64 = one.astype(np.float64)
                for c in range(g):
                    acc[c] = acc[c] + w[i, c] * s64
            res = acc.astype(np.float32).reshape(oshape)
            if profile:
                print(f'{n} images warped and summed in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags | (_native.ACCUMULATE if accumulate else 0)
        if output is None:
            result = _native.host_result(oshape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, oshape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        pl_ptr = None if pl is None else pl.ctypes.data
        m_ptr = None if ms is None else ms.ctypes.data
        fn = self._lib.vt_volume_warp_stack_sum_f64 if ms is not None and ms.dtype == np.float64 else self._lib.vt_volume_warp_stack_sum
        _native.check(fn(self._handle, n, m_ptr, disp.ctypes.data, 1 if shared else n, gshape[0], gshape[1], pl_ptr, g, w.ctypes.data,
                         shape[1], shape[2], ptr, flags), 'vt_volume_warp_stack_sum')
        if profile:
            print(f'{n} images warped and summed in {self.timer_stop():.3f}ms')
        return result

    def motion_corrected_sum(self, displacements=None, shifts=None, halves: bool = False, **kw) -> Union[np.ndarray, None]:
        """The sum of this stack's frames after motion correction, one ``warp_stack_sum`` call.  ``displacements``: the per-patch
        displacement grids as ``find_shifts(..., patch_grid=...)`` returns them, ``(n, gH, gW, 2)`` or one shared ``(gH, gW, 2)``;
        None = no local motion (one zero node).  ``shifts``: ``(n, 2)`` whole-frame shifts ``(y, x)``, turned into translation matrices
        by ``utils.stack_matrices`` as ``align_stack`` does; None = none.  ``halves=True`` returns ``(3, Ho, Wo)``: the sum of all
        frames, of the even ones and of the odd ones, from one sampling.  Further keywords go to ``warp_stack_sum`` (``output_shape``,
        ``planes``, ``output``, ``accumulate``, ``profile``)."""
        if 'weights' in kw or 'matrices' in kw:
            raise ValueError('motion_corrected_sum chooses weights and matrices itself: use warp_stack_sum')
        if displacements is None:
            displacements = np.zeros((1, 1, 2), dtype=np.float32)
        ms = None
        if shifts is not None:
            ms = stack_matrices(shifts, None, None, self.shape[1:], kw.get('output_shape'))
        disp = np.asarray(displacements)
        n = ms.shape[0] if ms is not None else (disp.shape[0] if disp.ndim == 4 else self.shape[0])
        weights = None
        if halves:
            weights = np.ones((n, 3), dtype=np.float64)
            weights[1::2, 1] = 0.0
            weights[0::2, 2] = 0.0
        return self.warp_stack_sum(displacements, ms, weights=weights, **kw)

    # -- a 1-D filter per image of the stack (extension: the ramp filter of weighted back-projection, low-pass, derivative taps) ----
    def filter_stack(self, taps, axis: int = 2, weights=None, pad: str = 'zero', profile: bool = False, output=None, *,
                     planes=None, _flags: int = 0) -> Union[np.ndarray, None]:
        """This volume taken as a stack of ``T`` images ``(T, H, W)``, each convolved with a 1-D filter along ``axis`` (1 or 2):
        ``out[i] = float32(weights[i] * convolve(image planes[i], taps_i))`` with ``numpy.convolve(line, taps_i, 'same')`` on every line
        along ``axis``, which is ``scipy.ndimage.convolve1d(image, taps_i, axis, mode='constant' | 'nearest', origin=0)``.  ``taps``:
        ``(K,)`` for one row shared by every entry or ``(n, K)`` for a row per entry, converted to float64; ``K`` odd and at most ``2 L
        - 1`` for an axis of extent ``L``.  ``pad``: ``'zero'`` reads 0 outside the image, ``'edge'`` the nearest sample.  ``planes``:
        ``n`` image indices inside ``[0, T)``; None = ``0 .. n-1``, and then ``n`` must equal ``T`` (``n`` is the number of tap rows if
        there are several, else of planes, else ``T``).  ``weights``: shape ``(n,)``, float64; None = ones.  The volume must hold samples:
        a ``filt_*`` interpolation holds prefilter coefficients and is refused -- filter on a ``'linear'`` volume and build the
        ``filt_*`` one from the result.  ``stack=True`` is not needed.  Returns a float32 array ``(n, H, W)``, or fills ``output`` of
        that shape (numpy, ``vt.empty`` device array, torch-ROCm tensor) and returns None on a GPU device, like ``affine_stack``.
        On a GPU device the sum runs in float64 over the non-zero taps only, in ascending order, and is rounded once; an image does not
        depend on the rest of the batch and repeated calls give identical bits.  ``device='cpu'`` is ``convolve1d`` on the float64 image,
        times the weight, cast to float32: the two devices agree to rounding on finite data only, since a zero tap times a non-finite
        sample is skipped on the GPU and NaN in scipy."""
        t = np.asarray(taps, dtype=np.float64)
        if t.ndim not in (1, 2) or 0 in t.shape:
            raise ValueError('taps must have shape (K,) or (n, K)')
        shared = t.ndim == 1
        t = np.ascontiguousarray(t)
        if axis not in (1, 2) or isinstance(axis, bool):
            raise ValueError('axis must be 1 or 2')
        if pad not in ('zero', 'edge'):
            raise ValueError("pad must be 'zero' or 'edge'")
        extent = self.shape[axis]
        k = t.shape[-1]
        if k % 2 == 0 or k > 2 * extent - 1:
            raise ValueError(f'{k} taps: an odd count of at most {2 * extent - 1} for an axis of extent {extent}')
        if not np.isfinite(t).all():
            raise ValueError('taps must be finite')
        if planes is None:
            pl = None
            n = self.shape[0] if shared else t.shape[0]
            if n != self.shape[0]:
                raise ValueError(f'{n} tap rows for a stack of {self.shape[0]} images: planes must be given')
        else:
            pl = np.asarray(planes)
            if pl.ndim != 1 or pl.size == 0 or not np.issubdtype(pl.dtype, np.integer):
                raise ValueError('planes must be a vector of integers')
            n = pl.shape[0]
            if pl.min() < 0 or pl.max() >= self.shape[0]:
                raise ValueError(f'planes must lie inside [0, {self.shape[0]})')
            pl = np.ascontiguousarray(pl, dtype=np.int32)
        if not shared and t.shape[0] != n:
            raise ValueError(f'{t.shape[0]} tap rows for {n} entries: one row per entry, or one shared row (K,)')
        w = np.ones(n, dtype=np.float64) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if w.shape != (n,):
            raise ValueError(f'weights must have shape ({n},)')
        if not np.isfinite(w).all():
            raise ValueError('weights must be finite')
        shape = (n, int(self.shape[1]), int(self.shape[2]))
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_'):
            raise ValueError('filter_stack needs samples, and a filt_* volume holds prefilter coefficients: filter on a linear volume '
                             'and build the filt_* volume from the result')
        if self.device == 'cpu':
            res = np.empty(shape, dtype=np.float32)
            t_start = time.time()
            for i in range(n):
                img = np.asarray(self.data[i if pl is None else int(pl[i])], dtype=np.float64)
                one = convolve1d(img, t if shared else t[i], axis=axis - 1, mode='constant' if pad == 'zero' else 'nearest', cval=0.0, origin=0)
                res[i] = (w[i] * one).astype(np.float32)
            if profile:
                print(f'{n} images filtered in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = _native.host_result(shape, self._dev)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        pl_ptr = None if pl is None else pl.ctypes.data
        _native.check(self._lib.vt_volume_filter_stack(self._handle, n, pl_ptr, t.ctypes.data, 1 if shared else n, k, axis,
                                                       0 if pad == 'zero' else 1, w.ctypes.data, ptr, flags), 'vt_volume_filter_stack')
        if profile:
            print(f'{n} images filtered in {self.timer_stop():.3f}ms')
        return result

    def ramp_filter(self, tilt_axis: int = 1, window: str = 'ramp', half_width=None, weights=None, pad: str = 'edge',
                    output=None) -> Union[np.ndarray, None]:
        """The filter of weighted back-projection on a tilt series whose tilt axis lies along array axis ``tilt_axis`` of the volume it
        came from (the convention of ``tilt_series`` and ``backproject_tilts``): ``filter_stack`` with ``utils.ramp_taps(L, window,
        half_width)`` along the in-plane axis that is not the tilt axis, ``tilt_axis=1`` -> ``axis=2`` and ``tilt_axis=2`` -> ``axis=1``,
        ``L`` that axis's extent."""
        if tilt_axis not in (1, 2) or isinstance(tilt_axis, bool):
            raise ValueError('tilt_axis must be 1 or 2')
        axis = 3 - tilt_axis
        return self.filter_stack(ramp_taps(self.shape[axis], window, half_width), axis, weights, pad, False, output)

    # -- shift scores of the stack against references (extension: where align_stack's shifts and warp_stack's grids come from) ----
    def correlate_stack(self, references=None, max_shift=(8, 8), patch_grid=(1, 1), profile: bool = False, output=None, *,
                        planes=None, reference_planes=None, _flags: int = 0) -> Union[np.ndarray, None]:
        """This volume taken as a stack of ``T`` images ``(T, H, W)``, each cross-correlated with a reference over the window of integer
        shifts ``max_shift = (Rh, Rw)``, per patch of ``patch_grid = (gH, gW)``:
        ``out[i, a, b, u, v] = sum over (y, x) in patch (a, b) of reference_i[y, x] * image_i[y + u - Rh, x + v - Rw]``, the image read
        as 0 outside, summed in float64.  Patch ``(a, b)`` covers rows ``[a H // gH, (a + 1) H // gH)`` and columns ``[b W // gW, (b + 1)
        W // gW)`` (``utils.patch_bounds``); ``1 <= gH <= H``, ``1 <= gW <= W``, ``0 <= Rh <= H - 1``, ``0 <= Rw <= W - 1``.  Exactly one
        of ``references`` and ``reference_planes`` must be given: ``references`` is ``(H, W)`` (shared by every entry) or ``(n, H, W)``,
        taken as float32 and finite; ``reference_planes`` are ``n`` indices of images of this stack (a tilt against its neighbour:
        nothing is uploaded).  ``planes``: ``n`` image indices inside ``[0, T)``; None = ``0 .. n-1``, and then ``n`` must equal ``T``
        (``n`` is the number of references if there are several, else of reference planes, else of planes, else ``T``).  The volume must
        hold samples: a ``filt_*`` interpolation is refused; ``stack=True`` is not needed.  Returns a float64 array ``(n, gH, gW, 2 Rh +
        1, 2 Rw + 1)``, or fills ``output`` of that shape (C-contiguous numpy float64, or a torch-ROCm float64 tensor on the volume's device) and returns None
        on a GPU device.  On a GPU device every product is exact, the additions follow a fixed order that depends on the patch's rows
        and columns alone, a score does not depend on the rest of the batch, the other patches or the window, and repeated calls give
        identical bits; a zero outside the image is multiplied, not skipped, so a non-finite reference pixel makes every score of its
        patch non-finite.  ``device='cpu'`` evaluates the same definition in float64 numpy, one sliced product-sum per shift (a shift's
        samples outside the image are left out there, which differs for non-finite references only)."""
        T, H, W = (int(s) for s in self.shape)
        if (references is None) == (reference_planes is None):
            raise ValueError('exactly one of references and reference_planes must be given')

        (rh, rw), (gh, gw) = _window_and_grid(max_shift, patch_grid, H, W)
        refs = shared = None
        if references is not None:
            refs = np.asarray(references, dtype=np.float32)
            if refs.ndim not in (2, 3) or refs.shape[-2:] != (H, W) or refs.shape[0] == 0:
                raise ValueError(f'references must have shape ({H}, {W}) or (n, {H}, {W})')
            shared = refs.ndim == 2
            refs = np.ascontiguousarray(refs)
            if not np.isfinite(refs).all():
                raise ValueError('references must be finite')
        pl = None if planes is None else _plane_indices(planes, 'planes', T)
        rp = None if reference_planes is None else _plane_indices(reference_planes, 'reference_planes', T)
        if refs is not None and not shared:
            n = refs.shape[0]
        elif rp is not None:
            n = rp.shape[0]
        elif pl is not None:
            n = pl.shape[0]
        else:
            n = T
        if pl is None and n != T:
            raise ValueError(f'{n} entries for a stack of {T} images: planes must be given')
        if pl is not None and pl.shape[0] != n:
            raise ValueError(f'{pl.shape[0]} planes for {n} entries')
        shape = (n, gh, gw, 2 * rh + 1, 2 * rw + 1)
        if int(np.prod(shape, dtype=np.float64)) >= 2 ** 31:
            raise ValueError(f'an output of shape {shape} has 2^31 elements or more')
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_'):
            raise ValueError('correlate_stack needs samples, and a filt_* volume holds prefilter coefficients: correlate on a linear volume')
        if self.device == 'cpu':
            if output is not None and not (isinstance(output, np.ndarray) and output.dtype == np.float64):
                raise ValueError(f'output must be a float64 array of shape {shape}')
            t_start = time.time()
            res = np.zeros(shape, dtype=np.float64)
            ye, xe = patch_bounds(H, gh), patch_bounds(W, gw)
            for i in range(n):
                img = np.asarray(self.data[i if pl is None else int(pl[i])], dtype=np.float32).astype(np.float64)
                if rp is not None:
                    ref = np.asarray(self.data[int(rp[i])], dtype=np.float32).astype(np.float64)
                else:
                    ref = (refs if shared else refs[i]).astype(np.float64)
                for a in range(gh):
                    for b in range(gw):
                        y0, y1, x0, x1 = int(ye[a]), int(ye[a + 1]), int(xe[b]), int(xe[b + 1])
                        for u in range(2 * rh + 1):
                            ya, yb = max(y0, rh - u), min(y1, H + rh - u)          # reference rows whose sample lies inside the image
                            if ya >= yb:
                                continue
                            for v in range(2 * rw + 1):
                                xa, xb = max(x0, rw - v), min(x1, W + rw - v)
                                if xa < xb:
                                    res[i, a, b, u, v] = (ref[ya:yb, xa:xb] * img[ya + u - rh:yb + u - rh, xa + v - rw:xb + v - rw]).sum()
            if profile:
                print(f'{n} images correlated in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = np.empty(shape, dtype=np.float64)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev, dtype=np.float64)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        _native.check(self._lib.vt_volume_correlate_stack(self._handle, n, None if pl is None else pl.ctypes.data,
                                                          None if refs is None else refs.ctypes.data,
                                                          0 if refs is None else (1 if shared else n),
                                                          None if rp is None else rp.ctypes.data, gh, gw, rh, rw, ptr, flags),
                      'vt_volume_correlate_stack')
        if profile:
            print(f'{n} images correlated in {self.timer_stop():.3f}ms')
        return result

    # -- window sums of the stack (extension: what turns correlate_stack's scores into correlation coefficients) ----
    def moments_stack(self, max_shift=(8, 8), patch_grid=(1, 1), profile: bool = False, output=None, *, planes=None,
                      _flags: int = 0) -> Union[np.ndarray, None]:
        """This volume taken as a stack of ``T`` images ``(T, H, W)``: the sum and the sum of squares of the samples that lie under
        every patch of ``patch_grid = (gH, gW)`` at every shift of the window ``max_shift = (Rh, Rw)``,
        ``out[i, a, b, u, v, 0] = sum over (y, x) in patch (a, b) of image_i[y + u - Rh, x + v - Rw]`` and ``out[i, a, b, u, v, 1]`` the
        same sum of the squares, the image read as 0 outside, summed in float64: the two sums of the image that stand beside
        ``correlate_stack``'s score in a correlation coefficient (``utils.normalized_scores``).  The patches, the window, their ranges
        and ``planes`` are ``correlate_stack``'s: ``planes`` are ``n`` image indices inside ``[0, T)``; None = every image in order.
        The volume must hold samples: a ``filt_*`` interpolation is refused; ``stack=True`` is not needed.  Returns a float64 array
        ``(n, gH, gW, 2 Rh + 1, 2 Rw + 1, 2)``, or fills ``output`` of that shape (C-contiguous numpy float64, or a torch-ROCm float64
        tensor on the volume's device) and returns None on a GPU device.  On a GPU device every square is exact, the additions follow
        a fixed order (row sums over the patch's columns, then over its rows) that depends on the patch's rows and columns and the shift
        alone, every value is a plain sum of its own samples (no running sums), so a value does not depend on the rest of the batch, the
        other patches or the window, a non-finite pixel reaches exactly the (patch, shift) pairs whose window covers it, and repeated
        calls give identical bits.  The work is pixels x (2 Rw + 1) additions, not pixels x shifts.  ``device='cpu'`` evaluates the same
        definition in float64 numpy."""
        T, H, W = (int(s) for s in self.shape)
        (rh, rw), (gh, gw) = _window_and_grid(max_shift, patch_grid, H, W)
        pl = None if planes is None else _plane_indices(planes, 'planes', T)
        n = T if pl is None else pl.shape[0]
        shape = (n, gh, gw, 2 * rh + 1, 2 * rw + 1, 2)
        if int(np.prod(shape, dtype=np.float64)) >= 2 ** 31:
            raise ValueError(f'an output of shape {shape} has 2^31 elements or more')
        if output is not None and tuple(getattr(output, 'shape', ())) != shape:
            raise ValueError(f'output must have shape {shape}')
        if self.interpolation.startswith('filt_'):
            raise ValueError('moments_stack needs samples, and a filt_* volume holds prefilter coefficients: take moments on a linear volume')
        if self.device == 'cpu':
            if output is not None and not (isinstance(output, np.ndarray) and output.dtype == np.float64):
                raise ValueError(f'output must be a float64 array of shape {shape}')
            t_start = time.time()
            res = np.empty(shape, dtype=np.float64)
            ye, xe = patch_bounds(H, gh)[:-1], patch_bounds(W, gw)[:-1]
            done = {}
            for i in range(n):
                p = i if pl is None else int(pl[i])
                if p in done:
                    res[i] = res[done[p]]
                    continue
                done[p] = i
                padded = np.zeros((H + 2 * rh, W + 2 * rw), dtype=np.float64)
                padded[rh:rh + H, rw:rw + W] = np.asarray(self.data[p], dtype=np.float32)
                with np.errstate(invalid='ignore', over='ignore'):
                    for k, field in enumerate((padded, padded * padded)):
                        # column sums per patch column and column shift first, as the device does, then the rows per row shift
                        rows = np.stack([np.add.reduceat(field[:, v:v + W], xe, axis=1) for v in range(2 * rw + 1)], axis=-1)
                        for u in range(2 * rh + 1):
                            res[i, :, :, u, :, k] = np.add.reduceat(rows[u:u + H], ye, axis=0)
            if profile:
                print(f'moments of {n} images in {(time.time() - t_start) * 1000:.3f}ms')
            if output is None:
                return res
            output[...] = res
            return output
        flags = _flags
        if output is None:
            result = np.empty(shape, dtype=np.float64)
            ptr, is_dev = result.ctypes.data, False
        else:
            ptr, is_dev, _ = _native.resolve_output(output, shape, self._dev, dtype=np.float64)
            result = None
        if is_dev:
            flags |= _native.OUT_DEVICE
        if profile:
            self.timer_start()
        _native.check(self._lib.vt_volume_moments_stack(self._handle, n, None if pl is None else pl.ctypes.data, gh, gw, rh, rw, ptr, flags),
                      'vt_volume_moments_stack')
        if profile:
            print(f'moments of {n} images in {self.timer_stop():.3f}ms')
        return result

    def correlate_stack_normalized(self, references=None, max_shift=(8, 8), patch_grid=(1, 1), profile: bool = False, output=None, *,
                                   planes=None, reference_planes=None) -> Union[np.ndarray, None]:
        """``correlate_stack``'s scores as correlation coefficients: ``utils.normalized_scores(correlate_stack(...), moments_stack(...),
        reference moments)``, float64 ``(n, gH, gW, 2 Rh + 1, 2 Rw + 1)`` inside [-1, 1] up to rounding, and exactly 0 where a patch or
        the samples under it are constant or a sum is not finite.  The arguments are ``correlate_stack``'s.  Samples outside the image
        count as zeros among the patch's pixels, which is ``correlate_stack``'s own convention: a patch on the image border is pulled
        towards the shifts that stay inside.  The reference's two sums per patch come from ``utils.patch_moments`` for host
        ``references`` and, for ``reference_planes`` on a GPU device, from ``moments_stack(max_shift=(0, 0), planes=reference_planes)``, so
        that nothing is downloaded; the two routes add in different orders and may differ in the last bits.  The scores and the window
        sums are computed on the device and combined on the host (numpy); ``output`` must be a numpy float64 array of the result's
        shape, which is filled and returned."""
        scores = self.correlate_stack(references, max_shift, patch_grid, profile, planes=planes, reference_planes=reference_planes)
        moments = self.moments_stack(max_shift, patch_grid, profile, planes=planes)
        if reference_planes is not None:
            if self.device == 'cpu':
                ref_moments = patch_moments(np.asarray(self.data, dtype=np.float32)[np.asarray(reference_planes)], patch_grid)
            else:
                ref_moments = self.moments_stack((0, 0), patch_grid, planes=reference_planes)[:, :, :, 0, 0, :]
        else:
            refs = np.asarray(references, dtype=np.float32)
            ref_moments = patch_moments(refs[None] if refs.ndim == 2 else refs, patch_grid)
        ncc = normalized_scores(scores, moments, ref_moments, image_shape=self.shape[1:])
        if output is None:
            return ncc
        if not (isinstance(output, np.ndarray) and output.dtype == np.float64 and output.shape == ncc.shape):
            raise ValueError(f'output must be a float64 array of shape {ncc.shape}')
        output[...] = ncc
        return output

    def find_shifts(self, references=None, max_shift=(8, 8), patch_grid=(1, 1), subpixel: bool = True, *, planes=None,
                    reference_planes=None, normalized: bool = False) -> np.ndarray:
        """Where every image, or every patch of it, matches its reference best: ``utils.peak_shifts(correlate_stack(...), subpixel)``,
        float64 ``(n, gH, gW, 2)``.  Entry ``[i, a, b]`` is the displacement ``d = (dy, dx)`` with ``image_i[y + d] ~ reference_i[y]`` on
        patch ``(a, b)``, searched inside ``max_shift`` and refined by a three-point parabola per axis.  ``align_stack(shifts=-d[:, 0,
        0])`` moves the images back onto their references, and ``d`` itself is ``warp_stack``'s displacement for that patch: an output
        pixel ``y`` of the patch samples the image at ``y + d``.  The values belong to the patch centres, which are not ``warp_stack``'s
        nodes -- those span the image corner to corner (``utils.stack_grid_nodes``) -- so a grid for ``warp_stack`` is interpolated or
        extrapolated from them.  ``normalized=True`` takes the peak of ``correlate_stack_normalized`` instead: the correlation
        coefficient follows the structure under the patch where the raw score, on images with a positive mean, follows whatever bright
        thing slides under it."""
        if normalized:
            scores = self.correlate_stack_normalized(references, max_shift, patch_grid, planes=planes, reference_planes=reference_planes)
        else:
            scores = self.correlate_stack(references, max_shift, patch_grid, planes=planes, reference_planes=reference_planes)
        return peak_shifts(scores, subpixel)

    def translate(self, translation: Vec3, profile: bool = False, output=None):
        return self.affine(translation_matrix(translation), profile, output)

    def shear(self, coefficients: Union[float, Vec3], profile: bool = False, output=None):
        return self.affine(shear_matrix(_triple(coefficients)), profile, output)

    def scale(self, coefficients: Union[float, Vec3], profile: bool = False, output=None):
        return self.affine(scale_matrix(_triple(coefficients)), profile, output)

    def rotate(self, rotation: Vec3, rotation_units: str = 'deg', rotation_order: str = 'rzxz',
               profile: bool = False, output=None):
        m = rotation_matrix(rotation=rotation, rotation_units=rotation_units, rotation_order=rotation_order)
        return self.affine(m, profile, output)
