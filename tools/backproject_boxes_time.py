#!/usr/bin/env python3
"""nb sub-tomograms of one shape straight from a resident tilt series: one vt_volume_backproject_boxes call (kernel 19: kernel 18 with a
box index, nb x tiles workgroups in one launch) against the only route before it, a loop of nb vt_volume_backproject calls (kernel 18:
one launch, one stream synchronise and one table upload per box).

  arm A   for b in range(nb): vt_volume_backproject(matrices[b], planes = 0 .. n-1, box shape, w[b]) into box b of a device array
  arm B   vt_volume_backproject_boxes(matrices, planes = 0 .. n-1, w, box shape) into a second device array

Per case: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's stream
around REPS repetitions; the figure is the median over the rounds, the spread max - min.  Both arms' times include their per-call uploads.
"B host" is the wall time of one B call on an idle stream up to its return (device output: the call returns after the launch), i.e. the
host pass that fills nb x n entries plus the table upload, median of ROUNDS x REPS calls timed on their own, each after a synchronise
(inside the timed repetitions a call first waits for the previous one's kernel, so its wall time says nothing about the host pass).
Every voxel of B is compared with A bit for bit (int32 views, the sign of a zero included) and the tool fails on a difference.  The
nb = 1 row shows what the box index costs against kernel 18 itself.
usage: tools/backproject_boxes_time.py [--reps 3] [--rounds 3] [--cases 1 2 3] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

TILTS, IMAGE, TOMO = 41, (1024, 1024), (256, 1024, 1024)
# (boxes, box shape)
CASES = {1: (1000, (64, 64, 64)), 2: (200, (32, 32, 32)), 3: (1, (64, 64, 64))}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2, 3])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('backproject_boxes_time.py needs a GPU')
import torch

lib = _native.load()
n = TILTS
rs = np.random.RandomState(300)
series = rs.random_sample((n,) + IMAGE).astype(np.float32)
angles = np.linspace(-60.0, 60.0, n)
print(f'{n} tilts of {IMAGE[1]}x{IMAGE[0]}, tomogram {"x".join(str(s) for s in TOMO[::-1])}; reps {args.reps}, rounds {args.rounds}; times in ms per '
      f'call of nb boxes')
print(f'{"interp":13s} {"nb":>5s} {"box":>9s} {"tile":>12s} {"grid":>7s} {"lds KiB":>7s} | {"A med":>9s} {"A spread":>8s} | {"B med":>9s} '
      f'{"B spread":>8s} {"B host":>8s} | {"A/B":>6s} | bits')

failed = False
handles = {interp: vt.StaticVolume(series, interpolation=interp, device='gpu:0', stack=True) for interp in args.interp}
for case in args.cases:
    nb, box = CASES[case]
    rs = np.random.RandomState(300 + case)
    half = np.asarray(box, np.float64) / 2
    pos = rs.uniform(half, np.asarray(TOMO, np.float64) - half, (nb, 3))              # every box inside the tomogram, fractional centres
    ms = np.ascontiguousarray(vt.utils.backproject_box_matrices(pos, angles, 1, TOMO, box, IMAGE), dtype=np.float32)
    w = np.ascontiguousarray(rs.uniform(0.5, 1.5, (nb, n)))
    box_vox = int(np.prod(box))
    out_a = torch.zeros((nb,) + box, dtype=torch.float32, device='cuda:0')
    out_b = torch.ones((nb,) + box, dtype=torch.float32, device='cuda:0')
    for interp in args.interp:
        sv = handles[interp]
        h = sv._handle
        host_b = []

        def arm_a():
            for b in range(nb):
                _native.check(lib.vt_volume_backproject(h, n, ms.ctypes.data + b * n * 64, None, w.ctypes.data + b * n * 8, *box,
                                                        ctypes.c_void_p(out_a.data_ptr() + 4 * box_vox * b), _native.OUT_DEVICE), 'backproject')

        def arm_b():
            _native.check(lib.vt_volume_backproject_boxes(h, nb, n, ms.ctypes.data, None, w.ctypes.data, *box,
                                                          ctypes.c_void_p(out_b.data_ptr()), _native.OUT_DEVICE), 'backproject_boxes')

        def timed(fn):
            sv.timer_start()
            for _ in range(args.reps):
                fn()
            return sv.timer_stop() / args.reps

        arm_a(); sv.synchronize()
        failed = failed or sv.info().last_kernel != 18
        arm_b(); sv.synchronize()
        info = sv.info()
        failed = failed or info.last_kernel != 19
        same = bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32)))
        failed = failed or not same
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        for _ in range(args.rounds * args.reps):      # the host part of B on its own: the stream is idle when the call starts
            sv.synchronize()
            t0 = time.perf_counter()
            arm_b()
            host_b.append((time.perf_counter() - t0) * 1e3)
        sv.synchronize()
        aa, bb = float(np.median(ta)), float(np.median(tb))
        print(f'{interp:13s} {nb:5d} {"x".join(str(s) for s in box[::-1]):>9s} {str(tuple(info.last_tile)):>12s} {info.last_grid:7d} '
              f'{info.last_lds_bytes / 1024:7.1f} | {aa:9.3f} {max(ta) - min(ta):8.3f} | {bb:9.3f} {max(tb) - min(tb):8.3f} '
              f'{float(np.median(host_b)):8.3f} | {aa / bb:6.2f} | {"same" if same else "DIFF"}', flush=True)
    del out_a, out_b
for sv in handles.values():
    sv.close()
print('A = a loop of nb backproject calls (kernel 18), B = one backproject_boxes call (kernel 19), device output, float32 matrices, per-call '
      'uploads included, hip events on the handle\'s stream.  B host = wall time of a B call on an idle stream up to its return (the host pass over '
      'nb x n entries and the table upload; part of B).  bits: every voxel of B against A, the sign of a zero included.')
if failed:
    sys.exit('backproject_boxes_time.py: the arms disagree')
