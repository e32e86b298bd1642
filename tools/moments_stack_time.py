#!/usr/bin/env python3
"""The sum and the sum of squares under every patch at every shift of a resident series: one vt_volume_moments_stack call (kernel 25:
row sums from a register window over LDS, then one thread per value adds its patch's rows) against the only device route there was
before it, and against the scores the sums stand beside.

  A   the old route: two vt_volume_correlate_stack calls against a resident image of ones, the first on the series, the second on a
      second handle that holds the squared series.  pixels x shifts float64 fmas each.
  B   one moments_stack call.  pixels x (2 Rw + 1) additions and as many fmas, then rows x shifts additions.
  C   one correlate_stack call with the same arguments and a resident reference (image i against image i + 1): the scores a
      normalised search computes anyway.  By operation count B's float64 work is 2 / (2 Rh + 1) of C's.

All into device arrays, the per-call upload (8 bytes per entry) included, on hip events on the handle's stream, arms alternated in one
process: per round A, B, C, REPS repetitions each; the figure is the median over ROUNDS rounds, the spread max - min.  Every row runs
under a time limit of its own (--limit seconds, SIGALRM with its default action: the process ends).  The tool asserts that A's sums
agree with B's on data in [0, 1): the sums of the samples within 2 (N + 2) 2^-53 sum |s| <= 2 (N + 2) N 2^-53, each arm within its
derived bound of the exact sum; the sums of squares within that plus N 2^-24, since arm A's second handle holds the squares rounded to
float32 (2^-24 s^2 each) where B squares exactly in float64.  It exits non-zero if they disagree or if B is not faster than C in some
row.
usage: tools/moments_stack_time.py [--reps 3] [--rounds 3] [--cases 1 2] [--limit 120]"""
import argparse
import ctypes
import os
import signal
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

CASES = {1: (61, 512, 512), 2: (41, 1024, 1024)}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
ap.add_argument('--limit', type=int, default=120)
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('moments_stack_time.py needs a GPU')
import torch

lib = _native.load()
signal.signal(signal.SIGALRM, signal.SIG_DFL)

print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call on the whole series')
print(f'{"stack":>14s} {"R":>3s} {"grid":>5s} {"wgs":>7s} {"lds KiB":>7s} | {"B med":>8s} {"spread":>7s} | {"C med":>8s} {"spread":>7s} {"B/C":>6s} {"ops":>5s} | '
      f'{"A med":>8s} {"spread":>7s} {"A/B":>6s} | {"|A-B| s":>9s} {"/bound":>7s} {"|A-B| s^2":>9s} {"/bound":>7s}')
disagree = slower = False
for case in args.cases:
    shape = CASES[case]
    n, H, W = shape
    signal.alarm(args.limit)
    rs = np.random.RandomState(700 + case)
    series = np.concatenate([rs.random_sample(shape).astype(np.float32), np.ones((1, H, W), np.float32)])       # image n: ones
    sv = vt.StaticVolume(series, device='gpu:0', stack=True)
    series[:n] *= series[:n]
    sq = vt.StaticVolume(series, device='gpu:0', stack=True)
    del series
    planes = np.arange(n, dtype=np.int32)
    ones = np.full(n, n, np.int32)
    neighbour = np.clip(np.arange(n) + 1, 0, n - 1).astype(np.int32)
    neighbour[-1] = n - 2
    for R in (8, 16):
        for g in (1, 8):
            signal.alarm(args.limit)
            shifts = (n, g, g, 2 * R + 1, 2 * R + 1)
            out_b = torch.zeros(shifts + (2,), dtype=torch.float64, device='cuda:0')
            out_c = torch.zeros(shifts, dtype=torch.float64, device='cuda:0')
            out_a = [torch.zeros(shifts, dtype=torch.float64, device='cuda:0') for _ in range(2)]

            def correlate(handle, ref_planes, out):
                _native.check(lib.vt_volume_correlate_stack(handle, n, planes.ctypes.data, None, 0, ref_planes.ctypes.data, g, g, R, R,
                                                            ctypes.c_void_p(out.data_ptr()), _native.OUT_DEVICE), 'correlate_stack')

            def arm_a():
                correlate(sv._handle, ones, out_a[0])
                correlate(sq._handle, ones, out_a[1])

            def arm_b():
                _native.check(lib.vt_volume_moments_stack(sv._handle, n, planes.ctypes.data, g, g, R, R, ctypes.c_void_p(out_b.data_ptr()),
                                                          _native.OUT_DEVICE), 'moments_stack')

            def arm_c():
                correlate(sv._handle, neighbour, out_c)

            arm_a(); arm_c(); arm_b()
            sv.synchronize(); sq.synchronize()
            info = sv.info()
            disagree = disagree or info.last_kernel != 25
            ta, tb, tc = [], [], []
            for _ in range(args.rounds):
                for arm, times in ((arm_a, ta), (arm_b, tb), (arm_c, tc)):
                    sq.synchronize()
                    sv.timer_start()
                    for _ in range(args.reps):
                        arm()
                    sq.synchronize()                                   # arm A's second call runs on the other handle's stream
                    times.append(sv.timer_stop() / args.reps)
            sv.synchronize()
            fa, fb, fc = (float(np.median(t)) for t in (ta, tb, tc))
            got = out_b.cpu().numpy()
            err = [float(np.abs(got[..., k] - out_a[k].cpu().numpy()).max()) for k in (0, 1)]
            N = (H // g) * (W // g)
            bound = [2.0 * (N + 2) * N * 2.0 ** -53, 2.0 * (N + 2) * N * 2.0 ** -53 + N * 2.0 ** -24]
            disagree = disagree or not (err[0] <= bound[0] and err[1] <= bound[1])
            slower = slower or not fb < fc
            print(f'{"x".join(map(str, shape)):>14s} {R:3d} {g:2d}x{g:<2d} {info.last_grid:7d} {info.last_lds_bytes / 1024:7.1f} | '
                  f'{fb:8.3f} {max(tb) - min(tb):7.3f} | {fc:8.3f} {max(tc) - min(tc):7.3f} {fb / fc:6.2f} {2 / (2 * R + 1):5.2f} | '
                  f'{fa:8.3f} {max(ta) - min(ta):7.3f} {fa / fb:6.1f} | {err[0]:9.2e} {err[0] / bound[0]:7.4f} {err[1]:9.2e} {err[1] / bound[1]:7.4f}', flush=True)
            del out_a, out_b, out_c
    signal.alarm(0)
    sv.close()
    sq.close()
print('B = one moments_stack call (kernel 25).  C = one correlate_stack call (kernel 24) with the same arguments, image i against the '
      'resident image i + 1.  A = two correlate_stack calls against a resident image of ones, on the series and on a handle holding its '
      'squares.  All with device output and the per-call upload included, on hip events on the first handle\'s stream with the second '
      'handle\'s stream drained inside the timed region.  ops = 2 / (2 Rh + 1), B\'s float64 operations over C\'s.  bound = 2 (N + 2) N '
      '2^-53 for the sums, that plus N 2^-24 for the sums of squares (A squares in float32), N the pixels of a patch.')
if disagree:
    sys.exit('moments_stack_time.py: correlate_stack against ones and moments_stack disagree')
if slower:
    sys.exit('moments_stack_time.py: moments_stack is not faster than correlate_stack in some row')
