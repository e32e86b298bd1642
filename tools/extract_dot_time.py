#!/usr/bin/env python3
"""Template scores (sum mask b, sum mask b^2, sum tmpl b per box) of n boxes out of a resident 1024 x 1024 x 512 tomogram: the new entry
point against what the library offered before it for the same job.

  arm A   vt_volume_extract into a device buffer of n boxes, then three torch reductions over it on the same stream (float32, torch's
          reduction order): (boxes * mask).sum, (boxes * boxes * mask).sum, (boxes * tmpl).sum over the box axes
  arm B   vt_volume_extract_dot (kernel 14), device output (float64, fixed order)

Per row: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the handle's
stream around REPS repetitions (torch runs its reductions on that stream too, so neither arm waits for the host); the spread of an
arm is max - min over its rounds.  Arm B's time includes the upload of the template, the mask and the table of matrices on every call.
usage: tools/extract_dot_time.py [--reps 5] [--rounds 3] [--rows 32 64 96] [--interp linear filt_bspline] [--no-big]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rows', type=int, nargs='*', default=[32, 64, 96])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
ap.add_argument('--shape', type=int, nargs=3, default=[512, 1024, 1024])
ap.add_argument('--no-big', action='store_true')
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('extract_dot_time.py needs a GPU')
import torch

SHAPE = tuple(args.shape)                      # (D, H, W): 1024 x 1024 x 512 with the short axis slowest
BIG = (32, 20000)
lib = _native.load()

rs = np.random.RandomState(0)
vol = np.empty(SHAPE, np.float32)
for d in range(SHAPE[0]):
    vol[d] = rs.random_sample(SHAPE[1:])
rows = [(b, 1000) for b in args.rows] + ([] if args.no_big else [BIG])
print(f'source {SHAPE[2]} x {SHAPE[1]} x {SHAPE[0]} float32, RandomState(0); reps {args.reps}, rounds {args.rounds}; times in us per box')
print(f'{"interp":13s} {"box":>5s} {"n":>6s} {"tile":>12s} {"launches":>8s} {"lds KiB":>7s} {"partials MiB":>12s} {"boxes MiB (A)":>13s} | '
      f'{"A med":>8s} {"A spread":>8s} | {"B med":>8s} {"B spread":>8s} | {"A/B":>5s} | {"max rel |A-B|":>13s}')


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
    for b, n in rows:
        box = (b, b, b)
        ms = matrices(b, n)
        r = np.random.RandomState(7)
        tmpl = r.uniform(-1, 1, box).astype(np.float32)
        g = np.meshgrid(*[np.linspace(-1, 1, b)] * 3, indexing='ij')
        mask = np.clip((1.0 - np.sqrt(sum(x * x for x in g))) / 0.3, 0, 1).astype(np.float32)      # soft sphere
        d_tmpl, d_mask = torch.from_numpy(tmpl).to('cuda:0'), torch.from_numpy(mask).to('cuda:0')
        out_b = torch.empty((n, 3), dtype=torch.float64, device='cuda:0')
        boxes = torch.empty((n,) + box, dtype=torch.float32, device='cuda:0')
        out_a = torch.empty((3, n), dtype=torch.float32, device='cuda:0')

        def arm_a():
            _native.check(lib.vt_volume_extract(h, n, ms.ctypes.data, *box, ctypes.c_void_p(boxes.data_ptr()), _native.OUT_DEVICE), 'extract')
            with torch.cuda.stream(stream):                   # the handle's stream: ordered after the extraction, no host wait
                mb = boxes * d_mask
                torch.sum(mb, dim=(1, 2, 3), out=out_a[0])
                torch.sum(mb * boxes, dim=(1, 2, 3), out=out_a[1])
                torch.sum(boxes * d_tmpl, dim=(1, 2, 3), out=out_a[2])

        def arm_b():
            _native.check(lib.vt_volume_extract_dot(h, n, ms.ctypes.data, tmpl.ctypes.data, mask.ctypes.data, *box,
                                                    ctypes.c_void_p(out_b.data_ptr()), _native.OUT_DEVICE), 'extract_dot')

        def timed(fn):
            sv.timer_start()
            for _ in range(args.reps):
                fn()
            return sv.timer_stop() * 1e3 / args.reps / n    # us per box

        arm_b(); sv.synchronize()
        info = sv.info()
        tile = tuple(info.last_tile)
        tiles = int(np.prod([-(-b // t) for t in tile]))
        per_launch = max(1, min(n, (64 << 20) // (tiles * 24)))
        launches = -(-n // per_launch)
        part_mib = per_launch * tiles * 24 / 2 ** 20
        arm_a(); sv.synchronize(); torch.cuda.synchronize()
        ref = out_b.T
        diff = float(((out_a.double() - ref).abs() / ref.abs().clamp_min(1e-30)).max())
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        aa, bb = float(np.median(ta)), float(np.median(tb))
        print(f'{interp:13s} {b:4d}^3 {n:6d} {str(tile):>12s} {launches:8d} {info.last_lds_bytes / 1024:7.1f} {part_mib:12.2f} '
              f'{n * b ** 3 * 4 / 2 ** 20:13.1f} | {aa:8.2f} {max(ta) - min(ta):8.2f} | {bb:8.2f} {max(tb) - min(tb):8.2f} | {aa / bb:5.2f} | {diff:13.2e}',
              flush=True)
        del boxes, out_a, out_b
        torch.cuda.empty_cache()
    sv.close()
print('A: extract of n boxes into a device buffer + three float32 torch reductions on the same stream (its temporaries, each as large as the '
      'buffer of boxes, come from torch\'s caching allocator); B: extract_dot (float64).  max rel |A-B|: largest relative difference of a sum.')
