#!/usr/bin/env python3
"""Weighted sum of n boxes out of a resident 1024 x 1024 x 512 tomogram (sub-tomogram averaging): the new entry point against
what the library offered before it for the same job.

  arm A   vt_volume_extract into a device buffer of n boxes, then torch.sum(dim=0) of it (float32, torch's reduction order)
  arm B   vt_volume_extract_sum (kernel 13), device output

Per row: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's
stream around REPS repetitions (torch runs its reduction on that stream too, so neither arm waits for the host); the spread of an
arm is max - min over its rounds.  The last
row (n = 20000 boxes of 32^3) has no arm A unless --big-a is given: its buffer alone is 2.6 GB.
usage: tools/extract_sum_time.py [--reps 10] [--rounds 3] [--rows 32 64 96 128] [--interp linear filt_bspline] [--no-big] [--big-a]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rows', type=int, nargs='*', default=[32, 64, 96, 128])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
ap.add_argument('--shape', type=int, nargs=3, default=[512, 1024, 1024])
ap.add_argument('--no-big', action='store_true')
ap.add_argument('--big-a', action='store_true')
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('extract_sum_time.py needs a GPU')
import torch

SHAPE = tuple(args.shape)                      # (D, H, W): 1024 x 1024 x 512 with the short axis slowest
N_FOR = {32: 1000, 64: 1000, 96: 1000, 128: 256}
BIG = (32, 20000)
lib = _native.load()

rs = np.random.RandomState(0)
vol = np.empty(SHAPE, np.float32)
for d in range(SHAPE[0]):
    vol[d] = rs.random_sample(SHAPE[1:])
rows = [(b, N_FOR[b], True) for b in args.rows] + ([] if args.no_big else [BIG + (args.big_a,)])
print(f'source {SHAPE[2]} x {SHAPE[1]} x {SHAPE[0]} float32, RandomState(0); reps {args.reps}, rounds {args.rounds}; times in us per box')
print(f'{"interp":13s} {"box":>5s} {"n":>6s} {"tile":>12s} {"segs":>5s} {"lds KiB":>7s} {"partials MiB":>12s} | {"A med":>8s} {"A spread":>8s} | '
      f'{"B med":>8s} {"B spread":>8s} | {"A/B":>5s} | {"max|A-B|":>9s}')


def matrices(b, n):
    r = np.random.RandomState(1000 + b + n)
    rot = r.uniform(0.0, 360.0, (n, 3))                 # random 'sxyz' angles, seeded
    pos = r.uniform(0.0, 1.0, (n, 3)) * (np.asarray(SHAPE) - 1)     # uniform over the volume: some boxes straddle the faces
    return np.ascontiguousarray(vt.utils.box_matrices(pos, rot, (b, b, b), rotation_order='sxyz'), dtype=np.float32)


for interp in args.interp:
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    h = sv._handle
    sptr = ctypes.c_void_p()
    _native.check(lib.vt_volume_stream(h, ctypes.byref(sptr)), 'vt_volume_stream')
    stream = torch.cuda.ExternalStream(sptr.value or 0)
    resident = sv.info().resident_bytes
    for b, n, with_a in rows:
        box = (b, b, b)
        ms = matrices(b, n)
        w = np.full(n, 1.0 / n)
        out_b = torch.empty(box, dtype=torch.float32, device='cuda:0')
        boxes = torch.empty((n,) + box, dtype=torch.float32, device='cuda:0') if with_a else None
        out_a = torch.empty(box, dtype=torch.float32, device='cuda:0') if with_a else None

        def arm_a():
            _native.check(lib.vt_volume_extract(h, n, ms.ctypes.data, *box, ctypes.c_void_p(boxes.data_ptr()), _native.OUT_DEVICE), 'extract')
            with torch.cuda.stream(stream):                   # the handle's stream: ordered after the extraction, no host wait
                torch.sum(boxes, dim=0, out=out_a)

        def arm_b():
            _native.check(lib.vt_volume_extract_sum(h, n, ms.ctypes.data, w.ctypes.data, *box, ctypes.c_void_p(out_b.data_ptr()),
                                                    _native.OUT_DEVICE), 'extract_sum')

        def timed(fn):
            sv.timer_start()
            for _ in range(args.reps):
                fn()
            return sv.timer_stop() * 1e3 / args.reps / n    # us per box

        arm_b(); sv.synchronize()
        info = sv.info()
        tile = tuple(info.last_tile)
        tiles = int(np.prod([-(-b // t) for t in tile]))
        segs = info.last_grid // tiles
        part_mib = (segs * b ** 3 * 8 / 2 ** 20) if segs > 1 else 0.0
        diff = float('nan')
        if with_a:
            arm_a(); sv.synchronize(); torch.cuda.synchronize()
            diff = float((out_a / n - out_b).abs().max())       # arm A sums with weight 1
        ta, tb = [], []
        for _ in range(args.rounds):
            if with_a:
                ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        bb = float(np.median(tb))
        a_txt = f'{np.median(ta):8.2f} {max(ta) - min(ta):8.2f}' if with_a else f'{"-":>8s} {"-":>8s}'
        r_txt = f'{np.median(ta) / bb:5.2f}' if with_a else f'{"-":>5s}'
        print(f'{interp:13s} {b:4d}^3 {n:6d} {str(tile):>12s} {segs:5d} {info.last_lds_bytes / 1024:7.1f} {part_mib:12.2f} | {a_txt} | '
              f'{bb:8.2f} {max(tb) - min(tb):8.2f} | {r_txt} | {diff:9.2e}')
        del boxes, out_a, out_b
    after = sv.info().resident_bytes
    print(f'{interp}: vt_volume_info.resident_bytes {resident} before the rows, {after} after them (the partials and the tables are '
          f'outside this figure: partials as listed per row, tables n x 200 bytes)')
    sv.close()
print('A: extract of n boxes into a device buffer + torch.sum(dim=0) on the same stream; B: extract_sum.  max|A-B|: arm A / n against arm B (weights 1 / n).')
