#!/usr/bin/env python3
"""Every image of a resident stack under its own 2-D affine map: one vt_volume_affine_stack call (kernel 21: one workgroup per (entry,
2-D tile), one patch, one sample per pixel) against the only route before it, a loop of n depth-1 vt_volume_backproject calls (kernel 18:
one launch, one stream synchronise and one table upload per image, a 3-D tile of which one plane exists).

  arm A   for i in range(n): vt_volume_backproject(matrix i, planes = [i], output (1, H, W)) into image i of a device array
  arm B   vt_volume_affine_stack(matrices, planes = 0 .. n-1, output (H, W)) into a second device array

Per case: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's stream
around REPS repetitions; the figure is the median over the rounds, the spread max - min.  Both arms' times include their per-call uploads.
Every pixel of B is compared with A at TOL (the tolerance of tests/test_gpu_extract.py on unit-range data, weights 1), and bit for bit
(int32 views) with VT_FORCE_DIRECT on both arms; the tool fails on a difference.  "B TB/s" is B's algorithmic traffic -- the stack read
once, the output written once -- over B's time, beside the 6.29 TB/s a device copy reaches.
usage: tools/stack_affine_time.py [--reps 3] [--rounds 3] [--cases 1 2] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

TOL = {'linear': 1e-6, 'bspline': 1e-6, 'bspline_simple': 1e-6, 'filt_bspline': 3e-6, 'filt_bspline_simple': 3e-6}
COPY_TBS = 6.29
CASES = {1: (61, 512, 512), 2: (41, 1024, 1024)}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('stack_affine_time.py needs a GPU')
import torch

lib = _native.load()
print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call of n images onto the images\' own shape')
print(f'{"interp":13s} {"stack":>14s} {"motion":>9s} {"tile":>11s} {"grid":>7s} {"lds KiB":>7s} | {"A med":>8s} {"A spread":>8s} | {"B med":>8s} '
      f'{"B spread":>8s} | {"A/B":>6s} | {"B TB/s":>6s} {"of copy":>7s} | {"max|B-A|":>9s} direct')

failed = False
for case in args.cases:
    shape = CASES[case]
    n, H, W = shape
    rs = np.random.RandomState(400 + case)
    series = rs.random_sample(shape).astype(np.float32)
    motions = {
        'shifts': vt.utils.stack_matrices(shifts=rs.randint(-20, 21, (n, 2)), image_shape=shape),
        'rot 3 deg': vt.utils.stack_matrices(shifts=rs.uniform(-2.0, 2.0, (n, 2)), rotations=np.full(n, 3.0), image_shape=shape),
    }
    out_a = torch.zeros(shape, dtype=torch.float32, device='cuda:0')
    out_b = torch.ones(shape, dtype=torch.float32, device='cuda:0')
    planes = np.arange(n, dtype=np.int32)
    for interp in args.interp:
        sv = vt.StaticVolume(series, interpolation=interp, device='gpu:0', stack=True)
        h = sv._handle
        for name, m3 in motions.items():
            ms = np.zeros((n, 4, 4), np.float32)
            ms[:, 0, 0] = 1
            ms[:, 1:, 1:] = m3

            def arm_a(flags=0):
                for i in range(n):
                    _native.check(lib.vt_volume_backproject(h, 1, ms.ctypes.data + i * 64, planes.ctypes.data + 4 * i, None, 1, H, W,
                                                            ctypes.c_void_p(out_a.data_ptr() + 4 * H * W * i), _native.OUT_DEVICE | flags), 'backproject')

            def arm_b(flags=0):
                _native.check(lib.vt_volume_affine_stack(h, n, ms.ctypes.data, None, None, H, W, ctypes.c_void_p(out_b.data_ptr()),
                                                         _native.OUT_DEVICE | flags), 'affine_stack')

            def timed(fn):
                sv.timer_start()
                for _ in range(args.reps):
                    fn()
                return sv.timer_stop() / args.reps

            arm_a(_native.FORCE_DIRECT); arm_b(_native.FORCE_DIRECT); sv.synchronize()
            same = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
            arm_a(); sv.synchronize()
            failed = failed or sv.info().last_kernel != 18
            arm_b(); sv.synchronize()
            info = sv.info()
            failed = failed or info.last_kernel != 21
            err = float((out_a - out_b).abs().max())
            failed = failed or not same or not err <= TOL[interp]
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(arm_a))
                tb.append(timed(arm_b))
            sv.synchronize()
            aa, bb = float(np.median(ta)), float(np.median(tb))
            tbs = 2 * 4.0 * n * H * W / (bb * 1e-3) / 1e12
            print(f'{interp:13s} {"x".join(str(s) for s in shape):>14s} {name:>9s} {str(tuple(info.last_tile)):>11s} {info.last_grid:7d} '
                  f'{info.last_lds_bytes / 1024:7.1f} | {aa:8.3f} {max(ta) - min(ta):8.3f} | {bb:8.3f} {max(tb) - min(tb):8.3f} | {aa / bb:6.2f} | '
                  f'{tbs:6.2f} {100 * tbs / COPY_TBS:6.1f}% | {err:9.2e} {"same" if same else "DIFF"}', flush=True)
        sv.close()
    del out_a, out_b
print('A = a loop of n depth-1 backproject calls (kernel 18), B = one affine_stack call (kernel 21), device output, float32 matrices, per-call '
      'uploads included, hip events on the handle\'s stream.  B TB/s = (stack + output bytes) / B\'s time, of copy = against 6.29 TB/s.  '
      'max|B-A| on the default routes (bound: TOL); direct: every pixel of B against A with VT_FORCE_DIRECT, int32 views.')
if failed:
    sys.exit('stack_affine_time.py: the arms disagree')
