// vt_warp_common.h -- what the displacement-grid kernels share (kind 20, vt_kernels_warp.hip: a 3-D grid on a volume; kind 22,
// vt_kernels_warpstack.hip: a 2-D grid per image of a stack): which nodes a tile touches, when a tile may bound its source box by the
// hull of those nodes, and the split of an output index into cell and fraction.  Each holds float64 additions, one multiplication followed
// by floor, and comparisons only -- nothing a compiler may contract -- so host and device agree to the bit.  An axis a kernel does not
// have (axis 0 of kind 22) carries a range of [0, 0].
#pragma once
#include "vt_box_common.h"

#include <cmath>

namespace vt {

// c_lo = cell of voxel `first`, n = nodes from there to the upper node of the cell of voxel `last` (first <= last).  r >= 0: monotone.
__host__ __device__ __forceinline__ void warp_cells(int first, int last, double r, int g, int& c_lo, int& n)
{
    if (g == 1) { c_lo = 0; n = 1; return; }
    const int a = (int)floor((double)first * r), b = (int)floor((double)last * r);
    c_lo = a < g - 2 ? a : g - 2;
    const int c_hi = b < g - 2 ? b : g - 2;
    n = c_hi - c_lo + 2;
}

// Whether a tile may bound its source box by the hull of its nodes (the header's bound): U (max_k g_k - 1) <= kWarpHullLimit.
__host__ __device__ __forceinline__ bool warp_hull_granted(const float (&umin)[3], const float (&umax)[3], int gm1_max)
{
    float U = 0.0f;
#pragma unroll
    for (int r = 0; r < 3; ++r) U = fmaxf(U, fmaxf(fabsf(umin[r]), fabsf(umax[r])));
    return (double)U * (double)gm1_max <= kWarpHullLimit;                    // (a 24-bit by 31-bit product: exact)
}

// cell and fraction of output index x on an axis: q = x r is a value of its own (no fma may absorb it into q - c)
__device__ __forceinline__ void warp_split(int x, double r, int gm2, int& c, double& f)
{
    const double q = rounded((double)x * r);
    const int fl = (int)floor(q);
    c = fl < gm2 ? fl : gm2;
    f = q - (double)c;
}

}  // namespace vt
