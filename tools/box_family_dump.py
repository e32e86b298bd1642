#!/usr/bin/env python3
"""Raw output bytes of the ten batched entry points (kernels 11-19 and the batched direct kernel) on small inputs, for comparing two
builds of the library bit for bit: run once per library (VT_LIB selects it, as for the timing tools) and `cmp` the two files.

Per interpolation and box shape one set of 7 pull matrices serves every call: 0 a small rotation about the middle of the source (tiles
wholly inside), 1 and 2 shifted over a face (tiles cut by the valid interval, tiles wholly outside), 3 wholly outside, 4 minifying 7 x (14 x for the stack:
no LDS box, the direct route), 5 and 6 general rotations.  The boxes are no multiple of any tile (tiles cut by the end of the box);
20 x 12 x 24 takes tile (8, 16, 16) for linear and 20 x 8 x 24 tile (8, 8, 16); every cubic box takes (8, 8, 16).  place, backproject
and backproject_boxes run a second pass with accumulate.  The launch record of info() is printed per call.
usage: VT_LIB=.../libvoltools_hip.so tools/box_family_dump.py OUT.bin [--interp linear bspline filt_bspline bspline_simple]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import voltools_amd as vt
from voltools_amd import _native

ap = argparse.ArgumentParser()
ap.add_argument('out')
ap.add_argument('--interp', nargs='*', default=['linear', 'bspline', 'filt_bspline', 'bspline_simple'])
args = ap.parse_args()
if _native.device_count() < 1:
    sys.exit('box_family_dump.py needs a GPU')

SRC = (48, 48, 48)
STACK = (5, 48, 40)                                  # the back-projection pair: 5 images of 48 x 40
BOXES = [(20, 12, 24), (20, 8, 24)]
rs = np.random.RandomState(7)
vol = rs.random_sample(SRC).astype(np.float32)
stack = rs.random_sample(STACK).astype(np.float32)


def rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    rz = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    rx = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return rz @ ry @ rx


def matrices(box, extent, shift=0.0, minify=7.0):
    """7 pull matrices (box voxel index -> source coordinate); `extent` = the source's shape (for the stack: plane, rows, columns)."""
    mid_box = (np.asarray(box) - 1) / 2.0
    mid = (np.asarray(extent) - 1) / 2.0
    spec = [((0.05, 0.03, -0.04), 1.0, mid), ((0.3, 0.0, 0.1), 1.0, mid + [shift, 0.45 * extent[1], 0]),
            ((0.0, 0.2, 0.0), 1.0, mid - [0, shift, 0.5 * extent[2]]), ((0.1, 0.1, 0.1), 1.0, mid + 3.0 * np.asarray(extent)),
            ((0.2, -0.1, 0.3), minify, mid + shift), ((0.9, 0.7, -1.1), 1.0, mid + [2.5, -3.25, 1.0]), ((-2.0, 0.4, 0.6), 0.8, mid - [4.0, 1.5, -shift])]
    ms = np.zeros((len(spec), 4, 4))
    for i, (ang, scale, centre) in enumerate(spec):
        a = rot(*ang) * scale
        ms[i, :3, :3] = a
        ms[i, :3, 3] = centre - a @ mid_box
        ms[i, 3, 3] = 1.0
    return ms


total = 0
with open(args.out, 'wb') as f:
    def dump(sv, name, interp, box, arr):
        global total
        info = sv.info()
        raw = np.ascontiguousarray(arr).tobytes()
        f.write(raw)
        total += len(raw)
        print(f'{name:22s} {interp:15s} box {str(box):13s} kernel {info.last_kernel:2d} tile {str(tuple(info.last_tile)):12s} grid {info.last_grid:5d} '
              f'lds {info.last_lds_bytes:6d}  {len(raw):8d} bytes')

    for interp in args.interp:
        sv = vt.StaticVolume(vol, interpolation=interp, device='gpu:0')
        st = vt.StaticVolume(stack, interpolation=interp, device='gpu:0', stack=True)     # filt_*: coefficients per image
        for box in BOXES:
            ms = matrices(box, SRC)
            n = len(ms)
            w = rs.uniform(-1.0, 1.0, n)
            wg = rs.uniform(-1.0, 1.0, (n, 5))
            tmpls = rs.random_sample((4,) + box).astype(np.float32)
            mask = (rs.random_sample(box) > 0.3).astype(np.float32)
            dump(sv, 'affine_batch', interp, SRC, sv.affine_batch(ms[:2].astype(np.float32)))
            dump(sv, 'extract', interp, box, sv.extract(ms, box))
            dump(sv, 'projection_batch', interp, box, sv.projection_batch(ms, box))
            dump(sv, 'extract_sum', interp, box, sv.extract_sum(ms, box, w))
            dump(sv, 'extract_dot', interp, box, sv.extract_dot(ms, tmpls[0], mask))
            dump(sv, 'extract_dot (no mask)', interp, box, sv.extract_dot(ms, tmpls[1]))
            dump(sv, 'extract_dot_multi', interp, box, sv.extract_dot_multi(ms, tmpls, mask))
            dump(sv, 'extract_sum_multi', interp, box, sv.extract_sum_multi(ms, box, wg))
            acc = sv.place(ms, box, w)
            dump(sv, 'place', interp, box, acc)
            sv.place(ms[::-1].copy(), box, w, output=acc, accumulate=True)
            dump(sv, 'place (accumulate)', interp, box, acc)
            # the stack: rows 1 and 2 of a matrix address image planes[i]; the minifying entry is steeper (two 2-D patches fit the LDS longer)
            mb = matrices(box, STACK, minify=14.0)
            planes = np.arange(n) % STACK[0]
            acc = st.backproject(mb, box, w, planes=planes)
            dump(st, 'backproject', interp, box, acc)
            st.backproject(mb[::-1].copy(), box, w, output=acc, planes=planes, accumulate=True)
            dump(st, 'backproject (accum.)', interp, box, acc)
            mbb = np.stack([matrices(box, STACK, s, minify=14.0) for s in (0.0, 1.75, -3.5)])
            wb = rs.uniform(-1.0, 1.0, (3, n))
            acc = st.backproject_boxes(mbb, box, wb, planes=planes)
            dump(st, 'backproject_boxes', interp, box, acc)
            st.backproject_boxes(mbb[:, ::-1].copy(), box, wb, output=acc, planes=planes, accumulate=True)
            dump(st, 'backproject_boxes (a.)', interp, box, acc)
        sv.close()
        st.close()
print(f'{total} bytes of outputs in {args.out}')
