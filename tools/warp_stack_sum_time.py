#!/usr/bin/env python3
"""The sum of the warped images of a resident stack: one vt_volume_warp_stack_sum call (kernel 26) against the route before it, the n
images written by vt_volume_warp_stack (kernel 22) and reduced by torch in float32.

  arm A   vt_volume_warp_stack(grids) into a device array of n images, then  G = 1: torch.sum(images, 0)
                                                                                G = 3: torch.einsum('nhw,ng->ghw', images, weights)
  arm B   vt_volume_warp_stack_sum(grids, weights) into a device array of G images

Grids are +-2 pixels on 8 x 8 nodes, one per image or one shared by every image; G = 3 is (all, even, odd).  Per case: the arms warmed,
then ROUNDS rounds of A, B alternated inside this process, each timed by the wall clock around REPS repetitions.  The library and
torch use different streams, so no one pair of events spans arm A: each arm ends synchronised instead (A synchronises the handle's
stream, queues the reduction and synchronises the device; B synchronises the handle's stream), which both arms pay alike.  The figure
is the median over the rounds, the spread max - min.  Every arm's time
includes its per-call uploads.  err = max |B - float64 sum of A's frames|; mem = device memory beyond the source that the arm's results
need (A: the n images and the sums; B: the sums).
usage: tools/warp_stack_sum_time.py [--reps 3] [--rounds 3] [--cases 1 2 3] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

CASES = {1: (61, 512, 512), 2: (41, 1024, 1024), 3: (40, 4096, 4096)}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2, 3])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('warp_stack_sum_time.py needs a GPU')
import torch

lib = _native.load()
print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call (wall clock around synchronised arms), n images onto their own shape')
print(f'{"interp":13s} {"stack":>14s} {"grid":>10s} {"G":>2s} {"tile":>11s} {"lds KiB":>7s} | {"A med":>9s} {"spread":>7s} | {"B med":>9s} '
      f'{"spread":>7s} | {"A/B":>6s} | {"err":>9s} | {"mem A MiB":>9s} {"mem B MiB":>9s}')

for case in args.cases:
    shape = CASES[case]
    n, H, W = shape
    rs = np.random.RandomState(700 + case)
    series = rs.random_sample(shape).astype(np.float32)
    grids = {'own': rs.uniform(-2.0, 2.0, (n, 8, 8, 2)).astype(np.float32), 'shared': rs.uniform(-2.0, 2.0, (1, 8, 8, 2)).astype(np.float32)}
    halves = np.ones((n, 3))
    halves[1::2, 1] = 0.0
    halves[0::2, 2] = 0.0
    images = torch.zeros(shape, dtype=torch.float32, device='cuda:0')
    for interp in args.interp:
        sv = vt.StaticVolume(series, interpolation=interp, device='gpu:0', stack=True)
        h = sv._handle
        for gname, g in grids.items():
            n_grids = g.shape[0]
            for G, wts in ((1, None), (3, halves)):
                w_dev = None if wts is None else torch.tensor(wts, dtype=torch.float32, device='cuda:0')
                out_b = torch.ones((G, H, W), dtype=torch.float32, device='cuda:0')
                keep = {}

                def arm_a():
                    _native.check(lib.vt_volume_warp_stack(h, n, None, g.ctypes.data, n_grids, 8, 8, None, None, H, W,
                                                           ctypes.c_void_p(images.data_ptr()), _native.OUT_DEVICE), 'warp_stack')
                    sv.synchronize()
                    keep['a'] = images.sum(0, keepdim=True) if w_dev is None else torch.einsum('nhw,ng->ghw', images, w_dev)
                    torch.cuda.synchronize()

                def arm_b():
                    _native.check(lib.vt_volume_warp_stack_sum(h, n, None, g.ctypes.data, n_grids, 8, 8, None, G,
                                                               None if wts is None else wts.ctypes.data, H, W,
                                                               ctypes.c_void_p(out_b.data_ptr()), _native.OUT_DEVICE), 'warp_stack_sum')
                    sv.synchronize()

                def timed(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        fn()
                    return (time.perf_counter() - t0) * 1e3 / args.reps

                arm_a(); arm_b()
                info = sv.info()
                assert info.last_kernel == 26
                ref = torch.zeros((G, H, W), dtype=torch.float64, device='cuda:0')
                for i in range(n):                                  # the float64 ascending sum of A's frames
                    for c in range(G):
                        ref[c] += (1.0 if wts is None else float(wts[i, c])) * images[i].double()
                err = float((out_b.double() - ref).abs().max())
                del ref
                ta, tb = [], []
                for _ in range(args.rounds):
                    ta.append(timed(arm_a))
                    tb.append(timed(arm_b))
                a, b = float(np.median(ta)), float(np.median(tb))
                mem_a, mem_b = 4.0 * (n + G) * H * W / 2 ** 20, 4.0 * G * H * W / 2 ** 20
                print(f'{interp:13s} {"x".join(str(s) for s in shape):>14s} {gname:>10s} {G:2d} {str(tuple(info.last_tile)):>11s} '
                      f'{info.last_lds_bytes / 1024:7.1f} | {a:9.3f} {max(ta) - min(ta):7.3f} | {b:9.3f} {max(tb) - min(tb):7.3f} | {a / b:6.2f} | '
                      f'{err:9.2e} | {mem_a:9.1f} {mem_b:9.1f}', flush=True)
                del out_b, keep
        sv.close()
    del images
print('A = one warp_stack call (kernel 22) into n device images + torch\'s float32 reduction, B = one warp_stack_sum call (kernel 26); '
      'device output, per-call uploads included; err = max |B - float64 ascending sum of A\'s frames|.')
