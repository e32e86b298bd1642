#!/usr/bin/env python3
"""Batched box extraction out of a resident 1024 x 1024 x 512 tomogram: the new entry point against what the library
offered before it for the same job.

  arm A   vt_volume_set_output_shape(box) + vt_volume_affine_batch, device output (one launch of the batched direct
          kernel up to 96^3, a loop of single transforms for 128^3)
  arm B   vt_volume_extract, device output, default routing

Per row: every shape warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the
handle's stream around REPS repetitions; the spread of an arm is max - min over its rounds.
usage: tools/extract_time.py [--reps 20] [--rounds 3] [--rows 64] [--interp filt_bspline]   (--rows / --interp: one row only,
e.g. under a kernel trace)"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=20)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rows', type=int, nargs='*', default=[32, 64, 96, 128])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
ap.add_argument('--shape', type=int, nargs=3, default=[512, 1024, 1024])
args = ap.parse_args()

SHAPE = tuple(args.shape)                      # (D, H, W): 1024 x 1024 x 512 with the short axis slowest
N_FOR = {32: 1000, 64: 1000, 96: 1000, 128: 256}
lib = _native.load()

rs = np.random.RandomState(0)
vol = np.empty(SHAPE, np.float32)
for d in range(SHAPE[0]):
    vol[d] = rs.random_sample(SHAPE[1:])
out = vt.empty((max(N_FOR[b] * b ** 3 for b in args.rows),), device='gpu:0')
print(f'source {SHAPE[2]} x {SHAPE[1]} x {SHAPE[0]} float32, RandomState(0); reps {args.reps}, rounds {args.rounds}; times in us per box')
print(f'{"interp":13s} {"box":>5s} {"n":>5s} {"kernel":>6s} {"tile":>10s} {"lds KiB":>7s} {"wg/CU":>5s} | {"A med":>8s} {"A spread":>8s} | {"B med":>8s} {"B spread":>8s} '
      f'| {"A/B":>5s} | {"B Gvox/s":>8s} {"store-side share":>16s}')

for interp in args.interp:
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    h = sv._handle
    for b in args.rows:
        n, box = N_FOR[b], (b, b, b)
        r = np.random.RandomState(1000 + b)
        rot = r.uniform(0.0, 360.0, (n, 3))                 # random 'sxyz' angles, seeded
        pos = r.uniform(0.0, 1.0, (n, 3)) * (np.asarray(SHAPE) - 1)     # uniform over the volume: some boxes straddle the faces
        ms = np.ascontiguousarray(vt.utils.box_matrices(pos, rot, box, rotation_order='sxyz'), dtype=np.float32)

        def arm_a():
            _native.check(lib.vt_volume_set_output_shape(h, *box), 'set_output_shape')
            _native.check(lib.vt_volume_affine_batch(h, n, ms.ctypes.data, ctypes.c_void_p(out.ptr), _native.OUT_DEVICE), 'affine_batch')

        def arm_b():
            _native.check(lib.vt_volume_extract(h, n, ms.ctypes.data, *box, ctypes.c_void_p(out.ptr), _native.OUT_DEVICE), 'extract')

        def timed(fn):
            sv.timer_start()
            for _ in range(args.reps):
                fn()
            return sv.timer_stop() * 1e3 / args.reps / n    # us per box

        arm_a(); arm_b(); sv.synchronize()                    # warm both
        info = sv.info()
        kernel, tile, lds = info.last_kernel, tuple(info.last_tile), info.last_lds_bytes
        wg = min(8, (160 * 1024) // max(lds, 1)) if kernel == 11 else 0
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        a, bb = float(np.median(ta)), float(np.median(tb))
        gvox = b ** 3 / bb / 1e3
        print(f'{interp:13s} {b:4d}^3 {n:5d} {kernel:6d} {str(tile):>10s} {lds / 1024:7.1f} {wg:5d} | {a:8.2f} {max(ta) - min(ta):8.2f} | {bb:8.2f} {max(tb) - min(tb):8.2f} '
              f'| {a / bb:5.2f} | {gvox:8.2f} {gvox * 4e9 / 8e12 * 100:15.1f}%')
    _native.check(lib.vt_volume_set_output_shape(h, *SHAPE), 'set_output_shape')
    sv.close()
print('wg/CU: workgroups per CU the planner expects from the LDS allocation of the launch (the batch-wide maximum box); the cubic '
      'instantiations hold at most 3 by registers.  store-side share: 4 B per output voxel against 8 TB/s; source reads not counted.')
