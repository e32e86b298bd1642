#!/usr/bin/env python3
"""A tilt series of projections out of one resident volume: the batched entry point against what the library offered before it
for the same job.

  arm A   a loop of vt_volume_project with VT_OUT_DEVICE, one call per angle (general matrices: transform into the handle's
          internal volume, then sum its planes)
  arm B   vt_volume_project_batch with VT_FORCE_TILED (kernel 12), device output

Per row: both arms warmed, then ROUNDS rounds of A, B alternated inside this process, each timed with hip events on the
handle's stream around REPS repetitions of the whole series; the spread of an arm is max - min over its rounds.  The two arms'
images are compared once per row (max |A - B| over every pixel).
usage: tools/project_batch_time.py [--reps 10] [--rounds 3] [--rows NAME ...] [--interp linear filt_bspline] [--out FILE]"""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ROWS = {                        # name: (cube edge, matrices)
    'tilt1_512': (512, lambda s: vt.utils.tilt_matrices(np.linspace(-60, 60, 61), 1, s)),
    'tilt2_512': (512, lambda s: vt.utils.tilt_matrices(np.linspace(-60, 60, 61), 2, s)),
    'tilt1_256': (256, lambda s: vt.utils.tilt_matrices(np.linspace(-60, 60, 61), 1, s)),
    'tilt1_128': (128, lambda s: vt.utils.tilt_matrices(np.linspace(-60, 60, 61), 1, s)),
    'tilt1_64': (64, lambda s: vt.utils.tilt_matrices(np.linspace(-60, 60, 61), 1, s)),
    'single_512': (512, lambda s: vt.utils.tilt_matrices([37.0], 1, s)),
    'random_512': (512, lambda s: np.stack([vt.utils.transform_matrix(rotation=tuple(r), rotation_order='sxyz',
                                                                      center=np.divide(np.subtract(s, 1), 2, dtype=np.float32))
                                            for r in np.random.RandomState(7).uniform(0.0, 360.0, (24, 3))])),
}

ap = argparse.ArgumentParser()
ap.add_argument('--reps', type=int, default=10)
ap.add_argument('--rounds', type=int, default=3)
ap.add_argument('--rows', nargs='*', default=list(ROWS))
ap.add_argument('--interp', nargs='*', default=['linear', 'filt_bspline'])
ap.add_argument('--out', default=None, help='also write the table to this file')
args = ap.parse_args()

lib = _native.load()
if _native.device_count() < 1:
    sys.exit('project_batch_time.py needs a GPU')
lines = []


def say(s=''):
    print(s, flush=True)
    lines.append(s)


say(f'device {_native.device_name(0)}; source cubes of float32, RandomState(0); reps {args.reps} (single_512: x20), rounds {args.rounds}; '
    f'times in ms per projection')
say(f'{"interp":13s} {"row":>11s} {"n":>3s} {"A kern":>6s} {"tile":>12s} {"lds KiB":>7s} {"wg/CU":>5s} {"grid":>7s} | {"A med":>7s} {"A spread":>8s} | '
    f'{"B med":>7s} {"B spread":>8s} | {"A/B":>5s} | {"max|A-B|":>9s}')

vols = {}
for interp in args.interp:
    for name in args.rows:
        edge, make = ROWS[name]
        shape = (edge, edge, edge)
        if edge not in vols:
            rs = np.random.RandomState(0)
            v = np.empty(shape, np.float32)
            for d in range(edge):
                v[d] = rs.random_sample(shape[1:])
            vols[edge] = v
        sv = vt.StaticVolume(vols[edge], interpolation=interp, device='gpu:0')
        h = sv._handle
        ms = np.ascontiguousarray(make(shape), dtype=np.float32)
        n = len(ms)
        reps = args.reps * (20 if n == 1 else 1)
        out_a = vt.empty((n,) + shape[1:], device='gpu:0')
        out_b = vt.empty((n,) + shape[1:], device='gpu:0')
        n2 = shape[1] * shape[2] * 4

        def arm_a():
            for i in range(n):
                _native.check(lib.vt_volume_project(h, ms[i].ctypes.data, ctypes.c_void_p(out_a.ptr + i * n2), _native.OUT_DEVICE), 'project')

        def arm_b():
            _native.check(lib.vt_volume_project_batch(h, n, ms.ctypes.data, *shape, ctypes.c_void_p(out_b.ptr),
                                                      _native.OUT_DEVICE | _native.FORCE_TILED), 'project_batch')

        def timed(fn):
            sv.timer_start()
            for _ in range(reps):
                fn()
            return sv.timer_stop() / reps / n      # ms per projection

        arm_a(); sv.synchronize()
        kern_a = sv.info().last_kernel
        arm_a(); arm_b(); sv.synchronize()             # warm both (arm A twice: its lazily built copies)
        info = sv.info()
        assert info.last_kernel == 12
        tile, lds, grid = tuple(info.last_tile), info.last_lds_bytes, info.last_grid
        wg = min(8, (160 * 1024) // max(lds, 1))
        diff = float(np.abs(out_a.get().astype(np.float64) - out_b.get()).max())
        ta, tb = [], []
        for _ in range(args.rounds):
            ta.append(timed(arm_a))
            tb.append(timed(arm_b))
        a, b = float(np.median(ta)), float(np.median(tb))
        say(f'{interp:13s} {name:>11s} {n:3d} {kern_a:6d} {str(tile):>12s} {lds / 1024:7.1f} {wg:5d} {grid:7d} | {a:7.3f} {max(ta) - min(ta):8.3f} | '
            f'{b:7.3f} {max(tb) - min(tb):8.3f} | {a / b:5.2f} | {diff:9.2e}')
        del out_a, out_b
        sv.close()
say('A kern: last_kernel of arm A\'s transform.  tile / lds KiB / grid: kernel 12\'s output tile, the launch\'s LDS allocation (the largest box of the '
    'batch) and the workgroups of its last launch.  wg/CU: workgroups per CU that allocation admits (the cubic instantiations hold at most 2 by '
    'registers).  max|A-B|: both arms sum 512 (256) samples per pixel; arm A rounds every sample to float32 in memory and sums in float32.')
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
