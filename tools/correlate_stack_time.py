#!/usr/bin/env python3
"""Shift scores of a resident series against references: one vt_volume_correlate_stack call (kernel 24: one workgroup per (entry, patch,
piece of 64 x 64 pixels, block of shifts), float64 fma from a register window over LDS) against the only device route there was
before it, vt_volume_extract_dot with one integer translation per shift and a box of depth 1.

  A   extract_dot: per patch one call with the reference patch as template and one matrix per (image, shift) when the reference is
      shared; per (image, patch) one call with one matrix per shift when every image has its own (resident) reference.  Matrices are
      built outside the timed region; host output (n x 3 float64 per call).
  B   one correlate_stack call into a device array, the per-call upload (8 bytes per entry; a host reference when there is one)
      included.

Both on hip events on the handle's stream, arms alternated in one process: per round A then B, REPS repetitions of B, one of A; the
figure is the median over ROUNDS rounds, the spread max - min.  "floor" is pixels x shifts float64 fmas at the spec peak of 78.6 TFLOP/s.
The tool asserts that A's scores agree with B's within 4 (N + 2) 2^-53 sum |r s| <= 4 (N + 2) N 2^-53 on data in [0, 1).
usage: tools/correlate_stack_time.py [--reps 3] [--rounds 3] [--cases 1 2] [--skip-a]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

PEAK_FP64_FLOPS = 78.6e12
CASES = {1: (61, 512, 512), 2: (41, 1024, 1024)}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
ap.add_argument('--skip-a', action='store_true')
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('correlate_stack_time.py needs a GPU')
import torch

lib = _native.load()


def shift_matrices(planes, y0, x0, R):
    """One pull matrix per (plane, shift): box voxel (0, y, x) -> (plane, y0 + y + u - R, x0 + x + v - R)."""
    u, v = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing='ij')
    ms = np.tile(np.eye(4), (len(planes), u.size, 1, 1))
    ms[:, :, 0, 3] = np.asarray(planes, np.float64)[:, None]
    ms[:, :, 1, 3] = y0 + u.ravel()
    ms[:, :, 2, 3] = x0 + v.ravel()
    return ms.reshape(-1, 4, 4)


print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call on the whole series')
print(f'{"stack":>14s} {"R":>3s} {"grid":>5s} {"refs":>8s} {"wgs":>7s} {"lds KiB":>7s} | {"B med":>8s} {"spread":>7s} | {"floor":>7s} {"B/floor":>7s} | '
      f'{"A med":>9s} {"spread":>8s} {"calls":>6s} {"A/B":>7s} | {"max|A-B|":>9s}')
failed = False
for case in args.cases:
    shape = CASES[case]
    n, H, W = shape
    rs = np.random.RandomState(600 + case)
    series = rs.random_sample(shape).astype(np.float32)
    shared = rs.random_sample((H, W)).astype(np.float32)
    neighbour = np.clip(np.arange(n) + 1, 0, n - 1).astype(np.int32)
    neighbour[-1] = n - 2
    sv = vt.StaticVolume(series, device='gpu:0', stack=True)
    h = sv._handle
    for R in (8, 16):
        for g in (1, 8):
            ph, pw = H // g, W // g
            for refs in ('resident', 'host'):
                out = torch.zeros((n, g, g, 2 * R + 1, 2 * R + 1), dtype=torch.float64, device='cuda:0')

                def arm_b():
                    _native.check(lib.vt_volume_correlate_stack(h, n, None, shared.ctypes.data if refs == 'host' else None,
                                                                1 if refs == 'host' else 0, neighbour.ctypes.data if refs == 'resident' else None,
                                                                g, g, R, R, ctypes.c_void_p(out.data_ptr()), _native.OUT_DEVICE), 'correlate_stack')

                # arm A's calls: (matrices, template, where its column 2 goes)
                calls = []
                if not args.skip_a:
                    for a in range(g):
                        for b in range(g):
                            ys, xs = slice(a * ph, (a + 1) * ph), slice(b * pw, (b + 1) * pw)
                            if refs == 'host':
                                calls.append((shift_matrices(np.arange(n), a * ph, b * pw, R), np.ascontiguousarray(shared[None, ys, xs]),
                                              (slice(None), a, b)))
                            else:
                                for i in range(n):
                                    calls.append((shift_matrices([i], a * ph, b * pw, R), np.ascontiguousarray(series[neighbour[i]][None, ys, xs]),
                                                  (slice(i, i + 1), a, b)))
                got_a = np.zeros(tuple(out.shape))

                def arm_a():
                    for ms, tmpl, where in calls:
                        got_a[where] = sv.extract_dot(ms, tmpl)[:, 2].reshape(-1, 2 * R + 1, 2 * R + 1)

                arm_b(); sv.synchronize()
                info = sv.info()
                failed = failed or info.last_kernel != 24
                if calls:
                    arm_a()
                ta, tb = [], []
                for _ in range(args.rounds):
                    if calls:
                        sv.timer_start(); arm_a(); ta.append(sv.timer_stop())
                    sv.timer_start()
                    for _ in range(args.reps):
                        arm_b()
                    tb.append(sv.timer_stop() / args.reps)
                sv.synchronize()
                fb = float(np.median(tb))
                floor = 2.0 * n * H * W * (2 * R + 1) ** 2 / PEAK_FP64_FLOPS * 1e3
                line = (f'{"x".join(map(str, shape)):>14s} {R:3d} {g:2d}x{g:<2d} {refs:>8s} {info.last_grid:7d} {info.last_lds_bytes / 1024:7.1f} | '
                        f'{fb:8.3f} {max(tb) - min(tb):7.3f} | {floor:7.3f} {fb / floor:7.2f} | ')
                if calls:
                    fa = float(np.median(ta))
                    err = float(np.abs(out.cpu().numpy() - got_a).max())
                    N = ph * pw
                    failed = failed or not err <= 4.0 * (N + 2) * N * 2.0 ** -53
                    line += f'{fa:9.2f} {max(ta) - min(ta):8.2f} {len(calls):6d} {fa / fb:7.1f} | {err:9.2e}'
                print(line, flush=True)
                del out
    sv.close()
print('B = one correlate_stack call (kernel 24), device output, per-call upload included.  A = extract_dot (kernel 14) with one translation '
      'per (image, shift), box (1, patch rows, patch columns), host output of n x 3 sums per call.  Both on hip events on the handle\'s '
      'stream.  floor = pixels x shifts x 2 flops at 78.6 TFLOP/s of vector FP64.  resident: image i against image i + 1 of the same '
      'stack; host: one shared reference uploaded per call.')
if failed:
    sys.exit('correlate_stack_time.py: extract_dot and correlate_stack disagree')
