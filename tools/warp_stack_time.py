#!/usr/bin/env python3
"""Every image of a resident stack through its own 2-D displacement grid: one vt_volume_warp_stack call (kernel 22) against the only route
before it, a loop of n vt_volume_warp calls on the stack handle (kernel 20: output (1, H, W), row 0 of the matrix (0, 0, 0, plane), a
(1, gH, gW, 3) grid whose component 0 is zero; linear handles only -- a stack=True handle with a filt_* interpolation refuses warp), and
against vt_volume_affine_stack with the same matrices, the sampling floor.

  arm A   for i in range(n): vt_volume_warp(matrix i with row 0 = plane i, grid i, output (1, H, W)) into image i of a device array
  arm F   vt_volume_affine_stack(matrices) into a second device array
  arm B   vt_volume_warp_stack(matrices, grids) into a third: a zero 8 x 8 grid per image, +-2 pixels on 8 x 8 per image, +-2 pixels
          dense per image, one +-2 pixel 8 x 8 grid shared by every image

Per case: the arms warmed, then ROUNDS rounds of A, F, B alternated inside this process, each timed with hip events on the handle's
stream around REPS repetitions; the figure is the median over the rounds, the spread max - min.  Every arm's time includes its per-call
uploads.  [host] is the share of a call spent on the host before the launch is queued: the wall-clock time of REPS asynchronous calls
(device output) over the event time.  B is compared with A at TOL (tests/test_gpu_extract.py; linear), B with a zero grid with F bit for
bit; the tool fails on a difference.
usage: tools/warp_stack_time.py [--reps 3] [--rounds 3] [--cases 1 2] [--interp linear filt_bspline]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

TOL = {'linear': 1e-6, 'bspline': 1e-6, 'bspline_simple': 1e-6, 'filt_bspline': 3e-6, 'filt_bspline_simple': 3e-6}
CASES = {1: (61, 512, 512), 2: (41, 1024, 1024)}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('warp_stack_time.py needs a GPU')
import torch

lib = _native.load()
print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call of n images onto the images\' own shape, [host share of the call]')
print(f'{"interp":13s} {"stack":>14s} {"grid":>16s} {"tile":>11s} {"lds KiB":>7s} | {"A med":>9s} {"spread":>7s} {"[host]":>6s} | {"F med":>8s} '
      f'{"spread":>7s} {"[host]":>6s} | {"B med":>8s} {"spread":>7s} {"[host]":>6s} | {"A/B":>6s} {"B/F":>5s} | check')

failed = False
for case in args.cases:
    shape = CASES[case]
    n, H, W = shape
    rs = np.random.RandomState(500 + case)
    series = rs.random_sample(shape).astype(np.float32)
    m3 = vt.utils.stack_matrices(shifts=rs.uniform(-2.0, 2.0, (n, 2)), rotations=np.full(n, 3.0), image_shape=shape)
    ms = np.zeros((n, 4, 4), np.float32)
    ms[:, 0, 0] = 1
    ms[:, 1:, 1:] = m3
    ms_a = ms.copy()                                       # arm A: row 0 = (0, 0, 0, plane), column 0 of rows 1 and 2 zero
    ms_a[:, 0] = 0
    ms_a[:, 0, 3] = np.arange(n)
    grids = {
        'zero 8x8': np.zeros((n, 8, 8, 2), np.float32),
        '+-2 px 8x8': rs.uniform(-2.0, 2.0, (n, 8, 8, 2)).astype(np.float32),
        '+-2 px dense': rs.uniform(-2.0, 2.0, (n, H, W, 2)).astype(np.float32),
        '+-2 px 8x8 shared': rs.uniform(-2.0, 2.0, (1, 8, 8, 2)).astype(np.float32),
    }
    out_a = torch.zeros(shape, dtype=torch.float32, device='cuda:0')
    out_f = torch.ones(shape, dtype=torch.float32, device='cuda:0')
    out_b = torch.ones(shape, dtype=torch.float32, device='cuda:0')
    for interp in args.interp:
        sv = vt.StaticVolume(series, interpolation=interp, device='gpu:0', stack=True)
        h = sv._handle
        with_a = interp == 'linear'
        for name, g in grids.items():
            n_grids, gh, gw = g.shape[0], g.shape[1], g.shape[2]
            g3 = np.zeros((n, gh, gw, 3), np.float32)
            g3[..., 1:] = g                                # (a shared grid: broadcast to every image's own copy for arm A)
            per = gh * gw * 3 * 4

            def arm_a():
                for i in range(n):
                    _native.check(lib.vt_volume_warp(h, ms_a.ctypes.data + i * 64, g3.ctypes.data + i * per, 1, gh, gw, 1, H, W,
                                                     ctypes.c_void_p(out_a.data_ptr() + 4 * H * W * i), _native.OUT_DEVICE), 'warp')

            def arm_f():
                _native.check(lib.vt_volume_affine_stack(h, n, ms.ctypes.data, None, None, H, W, ctypes.c_void_p(out_f.data_ptr()),
                                                         _native.OUT_DEVICE), 'affine_stack')

            def arm_b():
                _native.check(lib.vt_volume_warp_stack(h, n, ms.ctypes.data, g.ctypes.data, n_grids, gh, gw, None, None, H, W,
                                                       ctypes.c_void_p(out_b.data_ptr()), _native.OUT_DEVICE), 'warp_stack')

            def timed(fn):
                """(ms per call by hip events, host share of it)"""
                sv.synchronize()
                sv.timer_start()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                host = (time.perf_counter() - t0) * 1e3
                dev = sv.timer_stop()
                return dev / args.reps, min(1.0, host / dev)

            arm_f(); arm_b(); sv.synchronize()
            info = sv.info()
            failed = failed or info.last_kernel != 22
            check = ''
            if name.startswith('zero'):
                same = bool(torch.equal(out_f.view(torch.int32), out_b.view(torch.int32)))
                failed = failed or not same
                check = 'B == F bits' if same else 'B != F: DIFF'
            if with_a:
                arm_a(); sv.synchronize()
                failed = failed or sv.info().last_kernel != 20
                err = float((out_a - out_b).abs().max())
                failed = failed or not err <= TOL[interp]
                check = (check + ', ' if check else '') + f'max|B-A| {err:.2e}'
            ta, tf, tb = [], [], []
            for _ in range(args.rounds):
                if with_a:
                    ta.append(timed(arm_a))
                tf.append(timed(arm_f))
                tb.append(timed(arm_b))

            def stat(ts):
                if not ts:
                    return None, f'{"-":>9s} {"-":>7s} {"-":>6s}'
                med = float(np.median([t[0] for t in ts]))
                host = float(np.median([t[1] for t in ts]))
                return med, f'{med:9.3f} {max(t[0] for t in ts) - min(t[0] for t in ts):7.3f} [{100 * host:3.0f}%]'

            (aa, sa), (ff, sf), (bb, sb) = stat(ta), stat(tf), stat(tb)
            print(f'{interp:13s} {"x".join(str(s) for s in shape):>14s} {name:>16s} {str(tuple(info.last_tile)):>11s} '
                  f'{info.last_lds_bytes / 1024:7.1f} | {sa} | {sf[1:]} | {sb[1:]} | {(f"{aa / bb:6.2f}" if aa else "     -")} {bb / ff:5.2f} | {check}',
                  flush=True)
        sv.close()
    del out_a, out_f, out_b
print('A = a loop of n warp calls (kernel 20; linear only), F = one affine_stack call (kernel 21), B = one warp_stack call (kernel 22); device '
      'output, float32 matrices, per-call uploads included, hip events on the handle\'s stream.')
if failed:
    sys.exit('warp_stack_time.py: the arms disagree')
