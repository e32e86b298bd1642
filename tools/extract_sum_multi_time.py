#!/usr/bin/env python3
"""G weighted sums of the same n boxes out of a resident 1024 x 1024 x 512 tomogram (class averages, half-set maps): one call of the
multi-column entry point against G calls of the single-sum one, the only way before it.

dense rows (random weights in (-1, 2)):
  arm A   G calls of vt_volume_extract_sum (kernel 13) on the columns, device output one box each: every call samples every box again
  arm B   one call of vt_volume_extract_sum_multi (kernel 16), device output G boxes
hard-label rows (one-hot weights, G = --hard-g):
  arm A'  G calls of vt_volume_extract_sum on the partitioned matrices (class j's matrices with weights 1), the caller's other option
  arm B   the one call with the one-hot matrix

Per row: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's
stream around REPS repetitions; the spread of an arm is max - min over its rounds.  Both arms' times include their per-call uploads
(table of matrices, weights).  In the dense rows the boxes of B are compared with A's bit for bit and the tool fails on a difference;
A' sums each class in its own segmentation, so the hard-label rows are compared to float32 rounding only.
usage: tools/extract_sum_multi_time.py [--reps 3] [--rounds 3] [--rows 32 64] [--g 1 4 16] [--hard-g 16] [--interp linear filt_bspline]"""
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
ap.add_argument('--g', type=int, nargs='*', default=[1, 4, 16])
ap.add_argument('--hard-g', type=int, default=16)
ap.add_argument('--n', type=int, default=1000)
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
ap.add_argument('--shape', type=int, nargs=3, default=[512, 1024, 1024])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('extract_sum_multi_time.py needs a GPU')
import torch

SHAPE = tuple(args.shape)                      # (D, H, W): 1024 x 1024 x 512 with the short axis slowest
lib = _native.load()

rs = np.random.RandomState(0)
vol = np.empty(SHAPE, np.float32)
for d in range(SHAPE[0]):
    vol[d] = rs.random_sample(SHAPE[1:])
print(f'source {SHAPE[2]} x {SHAPE[1]} x {SHAPE[0]} float32, RandomState(0); reps {args.reps}, rounds {args.rounds}; times in us per box')
print(f'{"interp":13s} {"box":>5s} {"n":>6s} {"weights":>7s} {"G":>3s} {"tile":>12s} {"segments":>8s} {"launches":>8s} {"lds KiB":>7s} '
      f'{"partials MiB":>12s} | {"A med":>8s} {"A spread":>8s} | {"B med":>8s} {"B spread":>8s} | {"A/B":>5s} | {"bits":>5s}')
CHUNK = {(16, 16, 16): 2, (8, 16, 16): 4, (8, 8, 16): 8}


def matrices(b, n):
    r = np.random.RandomState(1000 + b + n)
    rot = r.uniform(0.0, 360.0, (n, 3))                 # random 'sxyz' angles, seeded
    pos = r.uniform(0.0, 1.0, (n, 3)) * (np.asarray(SHAPE) - 1)     # uniform over the volume: some boxes straddle the faces
    return np.ascontiguousarray(vt.utils.box_matrices(pos, rot, (b, b, b), rotation_order='sxyz'), dtype=np.float32)


failed = False
for interp in args.interp:
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    h = sv._handle
    for b in args.rows:
        n = args.n
        box = (b, b, b)
        ms = matrices(b, n)
        for kind, G in [('dense', g) for g in args.g] + ([('hard', args.hard_g)] if args.hard_g > 0 else []):
            r = np.random.RandomState(7)
            if kind == 'dense':
                w = r.uniform(-1, 2, (n, G))
                cols = [np.ascontiguousarray(w[:, j]) for j in range(G)]
                parts = [ms] * G
            else:
                labels = r.randint(0, G, n)
                w = np.zeros((n, G))
                w[np.arange(n), labels] = 1.0
                parts = [np.ascontiguousarray(ms[labels == j]) for j in range(G)]
                cols = [np.ones(len(p)) for p in parts]
            out_a = torch.zeros((G,) + box, dtype=torch.float32, device='cuda:0')
            out_b = torch.zeros((G,) + box, dtype=torch.float32, device='cuda:0')

            def arm_a():
                for j in range(G):
                    if len(parts[j]):
                        _native.check(lib.vt_volume_extract_sum(h, len(parts[j]), parts[j].ctypes.data, cols[j].ctypes.data, *box,
                                                                ctypes.c_void_p(out_a[j].data_ptr()), _native.OUT_DEVICE), 'extract_sum')

            def arm_b():
                _native.check(lib.vt_volume_extract_sum_multi(h, n, ms.ctypes.data, G, w.ctypes.data, *box,
                                                              ctypes.c_void_p(out_b.data_ptr()), _native.OUT_DEVICE), 'extract_sum_multi')

            def timed(fn):
                sv.timer_start()
                for _ in range(args.reps):
                    fn()
                return sv.timer_stop() * 1e3 / args.reps / n    # us per box

            arm_a(); sv.synchronize()
            arm_b(); sv.synchronize()
            info = sv.info()
            tile = tuple(info.last_tile)
            tiles = int(np.prod([-(-b // t) for t in tile]))
            if info.last_kernel == 16:
                gc = CHUNK[tile]
                chunks = -(-G // gc)
                # one launch unless the partials pass 64 MiB: then last_grid counts the last launch's chunks only
                segments = max(1, min(n, -(-1024 // tiles)))
                per_seg = -(-n // segments)
                segments = -(-n // per_seg)
                part_chunk = gc * segments * b ** 3 * 8
                chunks_per = chunks if segments == 1 else max(1, min(chunks, (64 << 20) // part_chunk))
                launches = -(-chunks // chunks_per)
                part_mib = 0.0 if segments == 1 else min(G, chunks_per * gc) * segments * b ** 3 * 8 / 2 ** 20
            else:                                               # a shape routed to a loop over kernel 13
                segments, launches, part_mib = info.last_grid // tiles, G, 0.0
            a, bb_ = out_a.cpu().numpy(), out_b.cpu().numpy()
            if kind == 'dense':
                same = np.array_equal(a.view(np.uint32), bb_.view(np.uint32))
                verdict = 'same' if same else 'DIFF'
                failed = failed or not same
            else:
                close = bool((np.abs(a - bb_) <= 2.0 ** -22 * np.maximum(np.abs(a), np.abs(bb_)) + 1e-30).all())
                verdict = 'close' if close else 'FAR'
                failed = failed or not close
            ta, tb = [], []
            for _ in range(args.rounds):
                ta.append(timed(arm_a))
                tb.append(timed(arm_b))
            aa, bb = float(np.median(ta)), float(np.median(tb))
            print(f'{interp:13s} {b:4d}^3 {n:6d} {kind:>7s} {G:3d} {str(tile):>12s} {segments:8d} {launches:8d} {info.last_lds_bytes / 1024:7.1f} '
                  f'{part_mib:12.2f} | {aa:8.2f} {max(ta) - min(ta):8.2f} | {bb:8.2f} {max(tb) - min(tb):8.2f} | {aa / bb:5.2f} | '
                  f'{verdict:>5s} (kernel {info.last_kernel})', flush=True)
            del out_a, out_b
    sv.close()
print('dense: A = G calls of extract_sum (kernel 13) on the columns, B = one call of extract_sum_multi (kernel 16); hard: A = G calls of '
      'extract_sum on the partitioned matrices, B = the one call with one-hot weights; all with device output and their per-call uploads.  '
      'partials MiB: float64 partials of one launch of B.  bits: dense rows, B\'s boxes against A\'s bit for bit; hard rows, to float32 '
      'rounding (the classes\' own segmentations differ).')
if failed:
    sys.exit('extract_sum_multi_time.py: the arms disagree')
