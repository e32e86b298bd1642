#!/usr/bin/env python3
"""n posed, weighted copies of a small resident map summed into one large map: vt_volume_place (kernel 17, per-tile lists, one workgroup
per non-empty output tile) against the only route before it, vt_volume_extract_sum on the same handle with the output as "the box"
(kernel 13: every output tile walks all n table entries).

  arm A   vt_volume_extract_sum(ms, output shape, w), device output
  arm B   vt_volume_place(ms, output shape, w), device output (includes its memset of the output)

Per case: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's stream
around REPS repetitions; the figure is the median over the rounds, the spread max - min.  Both arms' times include their per-call uploads.
The outputs are compared bit for bit (up to the sign of a zero; the output has 1024 tiles or more, so A runs one segment) and the tool
fails on a difference.  Host time: wall clock of one asynchronous call on an idle stream -- A fills the table entries and enqueues their
upload, B does the same and bins the entries into the per-tile lists, so B - A is the binning and the upload of the lists.
usage: tools/place_time.py [--reps 3] [--rounds 3] [--cases 1 2] [--interp filt_bspline linear]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

CASES = {1: ((64, 64, 64), 1000, (512, 1024, 1024)),      # (map, n, output (D, H, W)): 1024 x 1024 x 512 with the short axis slowest
         2: ((32, 32, 32), 200, (512, 512, 512))}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
ap.add_argument('--interp', nargs='*', default=['filt_bspline', 'linear'])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('place_time.py needs a GPU')
import torch

lib = _native.load()
print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call')
print(f'{"interp":13s} {"map":>5s} {"n":>5s} {"output":>16s} {"tile":>12s} {"tiles":>7s} {"non-empty":>9s} {"lds KiB":>7s} | {"A med":>8s} '
      f'{"A spread":>8s} | {"B med":>8s} {"B spread":>8s} | {"A/B":>6s} | {"host A":>7s} {"host B":>7s} {"B - A":>7s} | bits')

failed = False
for case in args.cases:
    tshape, n, out_shape = CASES[case]
    rs = np.random.RandomState(100 + case)
    tvol = rs.random_sample(tshape).astype(np.float32)
    pos = rs.uniform(0.0, 1.0, (n, 3)) * (np.asarray(out_shape) - 1)      # uniform over the output: some copies straddle the faces
    rot = rs.uniform(0.0, 360.0, (n, 3))                                  # random 'sxyz' angles, seeded
    w = rs.uniform(-1, 2, n)
    ms = np.ascontiguousarray(vt.utils.place_matrices(pos, rot, tshape, rotation_order='sxyz'), dtype=np.float32)
    out_a = torch.zeros(out_shape, dtype=torch.float32, device='cuda:0')
    out_b = torch.ones(out_shape, dtype=torch.float32, device='cuda:0')
    for interp in args.interp:
        sv = vt.StaticVolume(tvol, interpolation=interp, device='gpu:0')
        h = sv._handle

        def arm_a():
            _native.check(lib.vt_volume_extract_sum(h, n, ms.ctypes.data, w.ctypes.data, *out_shape, ctypes.c_void_p(out_a.data_ptr()),
                                                    _native.OUT_DEVICE), 'extract_sum')

        def arm_b():
            _native.check(lib.vt_volume_place(h, n, ms.ctypes.data, w.ctypes.data, *out_shape, ctypes.c_void_p(out_b.data_ptr()),
                                              _native.OUT_DEVICE), 'place')

        def timed(fn):
            sv.timer_start()
            for _ in range(args.reps):
                fn()
            return sv.timer_stop() / args.reps

        def host(fn):
            best = []
            for _ in range(3):
                sv.synchronize()
                t0 = time.perf_counter()
                fn()
                best.append((time.perf_counter() - t0) * 1e3)
                sv.synchronize()
            return min(best)

        arm_a(); sv.synchronize()
        info = sv.info()
        tile = tuple(info.last_tile)
        tiles = int(np.prod([-(-s // t) for s, t in zip(out_shape, tile)]))
        one_segment = info.last_kernel == 13 and info.last_grid == tiles
        arm_b(); sv.synchronize()
        info = sv.info()
        same = bool(torch.equal((out_a + 0.0).view(torch.int32), (out_b + 0.0).view(torch.int32)))
        failed = failed or not same or not one_segment or info.last_kernel != 17
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        ha, hb = host(arm_a), host(arm_b)
        aa, bb = float(np.median(ta)), float(np.median(tb))
        print(f'{interp:13s} {tshape[0]:4d}^3 {n:5d} {"x".join(str(s) for s in out_shape[::-1]):>16s} {str(tile):>12s} {tiles:7d} '
              f'{info.last_grid:9d} {info.last_lds_bytes / 1024:7.1f} | {aa:8.3f} {max(ta) - min(ta):8.3f} | {bb:8.3f} {max(tb) - min(tb):8.3f} | '
              f'{aa / bb:6.2f} | {ha:7.3f} {hb:7.3f} {hb - ha:7.3f} | {"same" if same else "DIFF"} (kernels {13 if one_segment else "13, segmented"}, '
              f'{info.last_kernel})', flush=True)
        sv.close()
    del out_a, out_b
print('A = extract_sum with the output as the box (kernel 13, one segment), B = place (kernel 17, memset included), device output, per-call '
      'uploads included, hip events on the handle\'s stream.  host: wall clock of one asynchronous call on an idle stream (minimum of 3); '
      'B - A = binning into per-tile lists + their upload.  bits: B against A on every voxel, up to the sign of a zero.')
if failed:
    sys.exit('place_time.py: the arms disagree')
