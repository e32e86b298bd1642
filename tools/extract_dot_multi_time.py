#!/usr/bin/env python3
"""Scores of n boxes out of a resident 1024 x 1024 x 512 tomogram against K templates under one mask: one call of the multi-template
entry point against K calls of the single-template one, the only way before it.

  arm A   K calls of vt_volume_extract_dot (kernel 14), device output n x 3 each: every call stages and samples every box again
  arm B   one call of vt_volume_extract_dot_multi (kernel 15), device output n x (2 + K)

Per row: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's
stream around REPS repetitions; the spread of an arm is max - min over its rounds.  Both arms' times include their per-call uploads
(table of matrices, templates, mask).  The columns of B are compared with A's bit for bit.
usage: tools/extract_dot_multi_time.py [--reps 3] [--rounds 3] [--rows 32 64] [--k 1 4 16] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rows', type=int, nargs='*', default=[32, 64])
ap.add_argument('--k', type=int, nargs='*', default=[1, 4, 16])
ap.add_argument('--n', type=int, default=1000)
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
ap.add_argument('--shape', type=int, nargs=3, default=[512, 1024, 1024])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('extract_dot_multi_time.py needs a GPU')
import torch

SHAPE = tuple(args.shape)                      # (D, H, W): 1024 x 1024 x 512 with the short axis slowest
lib = _native.load()

rs = np.random.RandomState(0)
vol = np.empty(SHAPE, np.float32)
for d in range(SHAPE[0]):
    vol[d] = rs.random_sample(SHAPE[1:])
print(f'source {SHAPE[2]} x {SHAPE[1]} x {SHAPE[0]} float32, RandomState(0); reps {args.reps}, rounds {args.rounds}; times in us per box')
print(f'{"interp":13s} {"box":>5s} {"n":>6s} {"K":>3s} {"tile":>12s} {"launches":>8s} {"lds KiB":>7s} {"partials MiB":>12s} {"templates MiB":>13s} | '
      f'{"A med":>8s} {"A spread":>8s} | {"B med":>8s} {"B spread":>8s} | {"A/B":>5s} | {"bits":>5s}')


def matrices(b, n):
    r = np.random.RandomState(1000 + b + n)
    rot = r.uniform(0.0, 360.0, (n, 3))                 # random 'sxyz' angles, seeded
    pos = r.uniform(0.0, 1.0, (n, 3)) * (np.asarray(SHAPE) - 1)     # uniform over the volume: some boxes straddle the faces
    return np.ascontiguousarray(vt.utils.box_matrices(pos, rot, (b, b, b), rotation_order='sxyz'), dtype=np.float32)


for interp in args.interp:
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    h = sv._handle
    for b in args.rows:
        n = args.n
        box = (b, b, b)
        ms = matrices(b, n)
        g = np.meshgrid(*[np.linspace(-1, 1, b)] * 3, indexing='ij')
        mask = np.clip((1.0 - np.sqrt(sum(x * x for x in g))) / 0.3, 0, 1).astype(np.float32)      # soft sphere
        for K in args.k:
            tmpls = np.random.RandomState(7).uniform(-1, 1, (K,) + box).astype(np.float32)
            out_a = torch.empty((K, n, 3), dtype=torch.float64, device='cuda:0')
            out_b = torch.empty((n, 2 + K), dtype=torch.float64, device='cuda:0')

            def arm_a():
                for j in range(K):
                    _native.check(lib.vt_volume_extract_dot(h, n, ms.ctypes.data, tmpls[j].ctypes.data, mask.ctypes.data, *box,
                                                            ctypes.c_void_p(out_a[j].data_ptr()), _native.OUT_DEVICE), 'extract_dot')

            def arm_b():
                _native.check(lib.vt_volume_extract_dot_multi(h, n, ms.ctypes.data, K, tmpls.ctypes.data, mask.ctypes.data, *box,
                                                              ctypes.c_void_p(out_b.data_ptr()), _native.OUT_DEVICE), 'extract_dot_multi')

            def timed(fn):
                sv.timer_start()
                for _ in range(args.reps):
                    fn()
                return sv.timer_stop() * 1e3 / args.reps / n    # us per box

            arm_a(); sv.synchronize()
            arm_b(); sv.synchronize()
            info = sv.info()
            assert info.last_kernel == 15
            tile = tuple(info.last_tile)
            tiles = int(np.prod([-(-b // t) for t in tile]))
            part_one = tiles * (2 + K) * 8
            per_launch = max(1, min(n, (64 << 20) // part_one))
            launches = -(-n // per_launch)
            a, bb_ = out_a.cpu().numpy(), out_b.cpu().numpy()
            same = all(np.array_equal(a[j][:, :2].view(np.uint64), bb_[:, :2].view(np.uint64)) and
                       np.array_equal(np.ascontiguousarray(a[j][:, 2]).view(np.uint64), np.ascontiguousarray(bb_[:, 2 + j]).view(np.uint64))
                       for j in range(K))
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(arm_a))
                tb.append(timed(arm_b))
            aa, bb = float(np.median(ta)), float(np.median(tb))
            print(f'{interp:13s} {b:4d}^3 {n:6d} {K:3d} {str(tile):>12s} {launches:8d} {info.last_lds_bytes / 1024:7.1f} '
                  f'{per_launch * part_one / 2 ** 20:12.2f} {K * b ** 3 * 4 / 2 ** 20:13.2f} | {aa:8.2f} {max(ta) - min(ta):8.2f} | '
                  f'{bb:8.2f} {max(tb) - min(tb):8.2f} | {aa / bb:5.2f} | {"same" if same else "DIFF":>5s}', flush=True)
            del out_a, out_b
    sv.close()
print('A: K calls of extract_dot (kernel 14); B: one call of extract_dot_multi (kernel 15); both with device output and their per-call '
      'uploads.  partials MiB: float64 partials of one launch of B; templates MiB: what B uploads per call besides the mask and the table.  '
      'bits: columns 0, 1 and 2 + j of B against A\'s call j.')
