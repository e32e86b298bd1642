"""A float64 numpy model of StaticVolume.warp_stack_sum (vt_volume_warp_stack_sum, kernel 26), written from the definition in
include/voltools_hip.h and sharing nothing with the library:

  * out[c] = float32(b + sum_i W[i, c] * B_i), i ascending, each product rounded to float64, then each sum (numpy's float64 arithmetic is
    that), with B_i the entries of tests/warp_stack_model.py (0 outside the skirt);
  * the launch: warp_stack's tile, node block and patch allocation (warp_stack_model.plan), one workgroup per (chunk of GC consecutive
    columns, tile), and the header's LDS formula  4 * NB * node_floats + 2 * allocation bytes  with NB = 1 for one grid, else 3;
  * which entries a chunk passes over: those whose weights are exactly 0 in all of the chunk's columns."""
import numpy as np

import warp_stack_model as wsm

GC = 4                                  # kWarpStackSumChunk
LDS_LIMIT = 160 * 1024                  # dynamic LDS a workgroup may have


def as_matrix(weights, n):
    w = np.ones((n, 1)) if weights is None else np.asarray(weights, np.float64)
    return w.reshape(n, -1)


def two_rounding_sum(images, weights, start=None):
    """(G, Ho, Wo) float64: acc = b; acc = acc + W[i, c] * images[i] for i ascending.  images: (n, Ho, Wo), float64 (or float32 widened)."""
    images = np.asarray(images, np.float64)
    W = as_matrix(weights, len(images))
    acc = np.zeros((W.shape[1],) + images.shape[1:]) if start is None else np.array(start, np.float64).reshape((W.shape[1],) + images.shape[1:])
    with np.errstate(invalid='ignore', over='ignore'):
        for i in range(len(images)):
            for c in range(W.shape[1]):
                t = W[i, c] * images[i]
                acc[c] = acc[c] + t
    return acc


def warp_stack_sum(stack, ms, grids, planes, out, interp, weights=None, start=None):
    """(sums (G, Ho, Wo) float64 before the final rounding, kept (Ho, Wo): farther than SKIRT_EPS from every skirt face in every entry)."""
    vols, masks, dist = wsm.warp_stack(stack, ms, grids, planes, out, interp)
    with np.errstate(invalid='ignore'):
        kept = ~(dist <= wsm.SKIRT_EPS).any(axis=0)
    return two_rounding_sum(vols, weights, start), kept


def chunks(g):
    return -(-g // GC)


def passed_over(weights, n):
    """(chunks, n) bool: entry i is not sampled by the workgroups of chunk k."""
    W = as_matrix(weights, n)
    return np.stack([(W[:, k * GC:(k + 1) * GC] == 0).all(axis=1) for k in range(chunks(W.shape[1]))])


def plan(ms, grids, n, out, interp, g=1, force_direct=False):
    """warp_stack_model.plan plus .sum_grid (workgroups), .sum_lds_dims and .sum_lds_bytes of kernel 26."""
    p = wsm.plan(ms, grids, n, out, interp, force_direct=force_direct)
    n_grids = 1 if np.ndim(grids) == 3 or n == 1 else n
    p.node_blocks = 1 if n_grids == 1 else 3
    p.sum_grid = chunks(g) * p.nT[0] * p.nT[1]
    p.sum_lds_dims = (2,) + tuple(p.lds_dims[1:]) if p.patch_bytes else (0, 0, 0)
    p.sum_lds_bytes = 4 * p.node_blocks * p.node_floats + 2 * p.patch_bytes
    return p
