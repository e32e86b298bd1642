#!/usr/bin/env python3
"""A tilt series back-projected into one volume: vt_volume_backproject (kernel 18: one image patch per tilt in one of two LDS buffers,
bilinear or 4 x 4 cubic taps, one barrier per tilt) against the only route before it, vt_volume_place on the same handle with matrices
whose row 0 is (0, 0, 0, plane) (kernel 17: two planes staged per tilt, eight taps, two barriers; linear only -- the cubic kinds have no
other route, their handles are stack=True and only arm B runs).

  arm A   vt_volume_place(plane-row matrices, output shape, w), device output (includes its memset of the output)
  arm B   vt_volume_backproject(matrices, planes = 0 .. n-1, output shape, w), device output

Per case: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's stream
around REPS repetitions; the figure is the median over the rounds, the spread max - min.  Both arms' times include their per-call uploads.
Where both arms run, the outputs are compared bit for bit on every voxel (up to the sign of a zero) and the tool fails on a difference.
usage: tools/backproject_time.py [--reps 3] [--rounds 3] [--cases 1 2] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

# (tilts, image (H, W), output (D, H, W), tomogram the output is a box of or None, first voxel of the box)
CASES = {1: (61, (512, 512), (256, 512, 512), None, None),
         2: (41, (1024, 1024), (64, 64, 64), (256, 1024, 1024), (150, 700, 120))}      # one sub-tomogram, off centre

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('backproject_time.py needs a GPU')
import torch

lib = _native.load()
print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call')
print(f'{"interp":13s} {"tilts":>5s} {"image":>10s} {"output":>13s} {"tile":>12s} {"tiles":>7s} {"lds KiB":>7s} | {"A med":>8s} {"A spread":>8s} | '
      f'{"B med":>8s} {"B spread":>8s} | {"A/B":>6s} | bits')

failed = False
for case in args.cases:
    n, image, out_shape, tomo, first = CASES[case]
    rs = np.random.RandomState(200 + case)
    series = rs.random_sample((n,) + image).astype(np.float32)
    angles = np.linspace(-60.0, 60.0, n)
    w = rs.uniform(0.5, 1.5, n)
    ms = vt.utils.backproject_matrices(angles, 1, out_shape if tomo is None else tomo, image)
    if tomo is not None:                      # the box's voxel index + first = the tomogram's voxel index
        shift = np.eye(4)
        shift[:3, 3] = first
        ms = ms @ shift
    ms = np.ascontiguousarray(ms, dtype=np.float32)
    pm = ms.copy()                            # arm A: the trilinear sample at an exactly integer plane
    pm[:, 0, :3] = 0
    pm[:, 0, 3] = np.arange(n)
    out_a = torch.zeros(out_shape, dtype=torch.float32, device='cuda:0')
    out_b = torch.ones(out_shape, dtype=torch.float32, device='cuda:0')
    for interp in args.interp:
        both = interp == 'linear'
        sv = vt.StaticVolume(series, interpolation=interp, device='gpu:0', stack=True)
        h = sv._handle

        def arm_a():
            _native.check(lib.vt_volume_place(h, n, pm.ctypes.data, w.ctypes.data, *out_shape, ctypes.c_void_p(out_a.data_ptr()),
                                              _native.OUT_DEVICE), 'place')

        def arm_b():
            _native.check(lib.vt_volume_backproject(h, n, ms.ctypes.data, None, w.ctypes.data, *out_shape, ctypes.c_void_p(out_b.data_ptr()),
                                                    _native.OUT_DEVICE), 'backproject')

        def timed(fn):
            sv.timer_start()
            for _ in range(args.reps):
                fn()
            return sv.timer_stop() / args.reps

        same = None
        if both:
            arm_a(); sv.synchronize()
            failed = failed or sv.info().last_kernel != 17
        arm_b(); sv.synchronize()
        info = sv.info()
        failed = failed or info.last_kernel != 18
        if both:
            same = bool(torch.equal((out_a + 0.0).view(torch.int32), (out_b + 0.0).view(torch.int32)))
            failed = failed or not same
        ta, tb = [], []
        for _ in range(args.rounds):
            if both:
                ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        tile = tuple(info.last_tile)
        bb = float(np.median(tb))
        a_txt = f'{float(np.median(ta)):8.3f} {max(ta) - min(ta):8.3f}' if both else f'{"-":>8s} {"-":>8s}'
        r_txt = f'{float(np.median(ta)) / bb:6.2f}' if both else f'{"-":>6s}'
        print(f'{interp:13s} {n:5d} {"x".join(str(s) for s in image[::-1]):>10s} {"x".join(str(s) for s in out_shape[::-1]):>13s} '
              f'{str(tile):>12s} {info.last_grid:7d} {info.last_lds_bytes / 1024:7.1f} | {a_txt} | {bb:8.3f} {max(tb) - min(tb):8.3f} | {r_txt} | '
              f'{"-" if same is None else ("same" if same else "DIFF")}', flush=True)
        sv.close()
    del out_a, out_b
print('A = place with plane-row matrices (kernel 17, memset included; linear only), B = backproject (kernel 18), device output, per-call '
      'uploads included, hip events on the handle\'s stream.  bits: B against A on every voxel, up to the sign of a zero.')
if failed:
    sys.exit('backproject_time.py: the arms disagree')
