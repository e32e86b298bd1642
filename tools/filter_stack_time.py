#!/usr/bin/env python3
"""A 1-D filter along one in-plane axis of every image of a resident stack: one vt_volume_filter_stack call (kernel 23: one workgroup per
(entry, strip of 64 lines, segment of 64 outputs), float64 fma over the non-zero taps) on a device-resident series, against what a
caller had to do before it -- copy the series to the host, filter there, upload again.

  B (baseline)  series.cpu() -> numpy rfft along the axis, product with the taps' transform, irfft -> back to the device (wall clock)
  F             vt_volume_filter_stack(taps, axis, pad) from the resident stack into a device array (hip events on the handle's stream,
                the per-call upload of the compacted taps included)

Per case: the full Ram-Lak row (K = 2L - 1, L non-zero taps) and its K = 65 middle, both axes, both pads.  F is warmed, then timed over
ROUNDS rounds of REPS repetitions; the figure is the median, the spread max - min.  "floor" is pixels x non-zero taps float64 fmas at the
spec peak of 78.6 TFLOP/s (2 flops per fma); pad 0 reaches fewer samples than that near the ends of a line, which the floor ignores.
"bp" is the time of backproject_tilts on the same series (the stage the filter feeds), "B" the baseline.  F is compared with the
baseline's result at 1e-4 of the largest sample (the baseline is an FFT in float64 of float32 data); the tool fails on a difference.
usage: tools/filter_stack_time.py [--reps 3] [--rounds 3] [--cases 1 2]"""
import argparse
import ctypes
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

PEAK_FP64_FLOPS = 78.6e12
CASES = {1: ((61, 512, 512), (256, 512, 512)), 2: ((41, 1024, 1024), (128, 1024, 1024))}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=3)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--cases', type=int, nargs='*', default=[1, 2])
args = ap.parse_args()

if _native.device_count() < 1:
    sys.exit('filter_stack_time.py needs a GPU')
import torch

lib = _native.load()


def host_filter(series, taps, axis, pad):
    """What a caller does without filter_stack: a zero- or edge-padded line, the product of the transforms, the middle of the result."""
    L, r = series.shape[axis], (taps.size - 1) // 2
    a = series.astype(np.float64)
    if pad == 'edge':
        width = [(0, 0)] * 3
        width[axis] = (r, r)
        a = np.pad(a, width, mode='edge')
    size = 1 << int(np.ceil(np.log2(a.shape[axis] + taps.size - 1)))
    prod = np.fft.rfft(a, size, axis=axis) * np.fft.rfft(taps, size).reshape([-1 if k == axis else 1 for k in range(3)])
    full = np.fft.irfft(prod, size, axis=axis)
    first = r + (r if pad == 'edge' else 0)
    return np.take(full, np.arange(first, first + L), axis=axis).astype(np.float32)


print(f'reps {args.reps}, rounds {args.rounds}; times in ms per call on the whole series')
print(f'{"stack":>14s} {"K":>5s} {"nnz":>5s} {"axis":>4s} {"pad":>5s} {"grid":>7s} {"lds KiB":>7s} | {"F med":>8s} {"spread":>7s} | {"floor":>7s} {"F/floor":>7s} | '
      f'{"bp":>8s} | {"B":>9s} {"B/F":>7s} | {"max|F-B|":>9s}')
failed = False
for case in args.cases:
    shape, vol_shape = CASES[case]
    n, H, W = shape
    rs = np.random.RandomState(500 + case)
    series = rs.random_sample(shape).astype(np.float32)
    angles = np.linspace(-60.0, 60.0, n)
    dev_in = torch.from_numpy(series).to('cuda:0')
    out = torch.zeros(shape, dtype=torch.float32, device='cuda:0')
    rec = torch.zeros(vol_shape, dtype=torch.float32, device='cuda:0')
    sv = vt.StaticVolume(series, device='gpu:0', stack=True)
    h = sv._handle

    def timed(fn):
        sv.timer_start()
        for _ in range(args.reps):
            fn()
        return sv.timer_stop() / args.reps

    bp = {}
    for tilt_axis in (1, 2):
        fn = lambda: sv.backproject_tilts(angles, tilt_axis, output_shape=vol_shape, output=rec)
        fn(); sv.synchronize()
        bp[3 - tilt_axis] = float(np.median([timed(fn) for _ in range(args.rounds)]))
    for axis in (2, 1):
        L = shape[axis]
        for taps in (vt.utils.ramp_taps(L), vt.utils.ramp_taps(L, half_width=32)):
            nnz = int(np.count_nonzero(taps))
            for pad in ('zero', 'edge'):
                def arm():
                    _native.check(lib.vt_volume_filter_stack(h, n, None, taps.ctypes.data, 1, taps.size, axis, 0 if pad == 'zero' else 1, None,
                                                             ctypes.c_void_p(out.data_ptr()), _native.OUT_DEVICE), 'filter_stack')
                arm(); sv.synchronize()
                info = sv.info()
                failed = failed or info.last_kernel != 23
                ts = [timed(arm) for _ in range(args.rounds)]
                sv.synchronize()
                t0 = time.perf_counter()
                want = torch.from_numpy(host_filter(dev_in.cpu().numpy(), taps, axis, pad)).to('cuda:0')
                torch.cuda.synchronize()
                base = (time.perf_counter() - t0) * 1e3
                err = float((out - want).abs().max())
                failed = failed or not err <= 1e-4
                f = float(np.median(ts))
                floor = 2.0 * n * H * W * nnz / PEAK_FP64_FLOPS * 1e3
                print(f'{"x".join(map(str, shape)):>14s} {taps.size:5d} {nnz:5d} {axis:4d} {pad:>5s} {info.last_grid:7d} {info.last_lds_bytes / 1024:7.1f} | '
                      f'{f:8.3f} {max(ts) - min(ts):7.3f} | {floor:7.3f} {f / floor:7.2f} | {bp[axis]:8.3f} | {base:9.1f} {base / f:7.1f} | {err:9.2e}',
                      flush=True)
                del want
    sv.close()
    del dev_in, out, rec
print('F = one filter_stack call (kernel 23), device output, per-call upload included, hip events on the handle\'s stream.  floor = pixels x '
      'non-zero taps x 2 flops at 78.6 TFLOP/s of vector FP64.  bp = backproject_tilts of the same series along the matching tilt axis '
      'into 256 x 512 x 512 (case 1) or 128 x 1024 x 1024 (case 2), linear.  B = device -> host, numpy rfft filter in float64, host -> '
      'device, wall clock, once.  max|F-B| on unit-range data (bound 1e-4).')
if failed:
    sys.exit('filter_stack_time.py: filter_stack and the host filter disagree')
