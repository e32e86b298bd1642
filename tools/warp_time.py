#!/usr/bin/env python3
"""StaticVolume.warp on a resident 512^3 volume, 512^3 device output: what the displacement grid costs on top of the sampling.

  arm A   vt_volume_extract with n = 1 and the same matrix: the sampling alone (kernel 11)
  arm B   vt_volume_warp with a zero grid of 8^3 nodes
  arm C   vt_volume_warp with random +-2-voxel grids of 8^3 and of 64^3 nodes
  arm D   arm C under VT_FORCE_DIRECT (every tile gathers from global memory)

Per (interpolation, matrix): every arm warmed, then ROUNDS rounds of the arms alternated inside this process, each timed with hip events on
the handle's stream around REPS calls (uploads of table and grid included); median and spread (max - min) over the rounds.  The host time
of a call -- the per-tile range pass, the staging copy of the grid and the enqueue; the call returns before the kernel ends -- is the wall
clock of REPS further calls, each issued on an idle stream.
usage: tools/warp_time.py [--reps 5] [--rounds 3] [--size 512] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--size', type=int, default=512)
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
args = ap.parse_args()

N = args.size
SHAPE = (N, N, N)
lib = _native.load()
rs = np.random.RandomState(0)
vol = np.empty(SHAPE, np.float32)
for d in range(N):
    vol[d] = rs.random_sample(SHAPE[1:])
out = vt.empty(SHAPE, device='gpu:0')
optr = ctypes.c_void_p(out.ptr)
centre = (np.asarray(SHAPE, np.float64) - 1) / 2
MATRICES = {'identity': np.eye(4, dtype=np.float32),
            'rot sxyz (25, 40, -15)': np.ascontiguousarray(vt.utils.transform_matrix(rotation=(25, 40, -15), rotation_order='sxyz',
                                                                                      center=centre), dtype=np.float32)}
GRIDS = {'B zero 8^3': np.zeros((8, 8, 8, 3), np.float32),
         'C +-2 8^3': np.random.RandomState(1).uniform(-2, 2, (8, 8, 8, 3)).astype(np.float32),
         'C +-2 64^3': np.random.RandomState(2).uniform(-2, 2, (64, 64, 64, 3)).astype(np.float32)}

print(f'source and output {N}^3 float32, RandomState(0), device output; reps {args.reps}, rounds {args.rounds}; times in ms per call')
print(f'{"interp":13s} {"matrix":22s} {"arm":14s} {"kernel":>6s} {"tile":>12s} {"lds dims":>14s} {"lds KiB":>7s} | {"gpu med":>8s} {"spread":>7s} | '
      f'{"host med":>8s} {"spread":>7s} | {"Gvox/s":>6s}')
for interp in args.interp:
    sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
    h = sv._handle
    for mname, m in MATRICES.items():
        arms = {}

        def arm_a(m=m):
            _native.check(lib.vt_volume_extract(h, 1, m.ctypes.data, *SHAPE, optr, _native.OUT_DEVICE), 'extract')
        arms['A extract n=1'] = arm_a
        for gname, g in GRIDS.items():
            def arm(flags=0, g=g, m=m):
                _native.check(lib.vt_volume_warp(h, m.ctypes.data, g.ctypes.data, *g.shape[:3], *SHAPE, optr, _native.OUT_DEVICE | flags), 'warp')
            arms[gname] = arm
            if gname.startswith('C'):
                arms['D' + gname[1:] + ' direct'] = lambda arm=arm: arm(_native.FORCE_DIRECT)
        rows = {}
        for name, fn in arms.items():                      # warm, and note what ran
            fn()
            sv.synchronize()
            info = sv.info()
            rows[name] = (info.last_kernel, tuple(info.last_tile), tuple(info.last_lds_dims), info.last_lds_bytes)
        gpu = {name: [] for name in arms}
        host = {name: [] for name in arms}
        for _ in range(args.rounds):
            for name, fn in arms.items():
                sv.timer_start()
                for _ in range(args.reps):
                    fn()
                gpu[name].append(sv.timer_stop() / args.reps)
                spent = 0.0
                for _ in range(args.reps):                 # the host's share: each call starts on an idle stream
                    sv.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    spent += time.perf_counter() - t0
                host[name].append(spent * 1e3 / args.reps)
        for name in arms:
            k, tile, ld, lb = rows[name]
            gm, hm = float(np.median(gpu[name])), float(np.median(host[name]))
            print(f'{interp:13s} {mname:22s} {name:14s} {k:6d} {str(tile):>12s} {str(ld):>14s} {lb / 1024:7.1f} | {gm:8.3f} {max(gpu[name]) - min(gpu[name]):7.3f} | '
                  f'{hm:8.3f} {max(host[name]) - min(host[name]):7.3f} | {N ** 3 / gm / 1e6:6.2f}')
    sv.close()
print('gpu: hip events on the handle\'s stream around the calls of a round (uploads included).  host: wall clock of a call issued on an idle '
      'stream, until it returned (the kernel is still running then).')
