// vt_warp_common.h -- what the displacement-grid kernels share (kind 20, vt_kernels_warp.hip: a 3-D grid on a volume; kind 22,
// vt_kernels_warpstack.hip: a 2-D grid per image of a stack; kind 26, vt_kernels_warpstacksum.hip: those images summed): which nodes a
// tile touches, when a tile may bound its source box by the hull of those nodes, the split of an output index into cell and fraction,
// and for kinds 22 and 26 the tile's patch formula and the row lerp of the node block.  Each holds float64 additions, one multiplication followed
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

// ---------------------------------------------------------------------------------------------------
// kinds 22 and 26: a 2-D grid per image of a stack
// ---------------------------------------------------------------------------------------------------
// The staged patch (Ly, Lx) of a tile of entry e whose nodes span [umin, umax] per source axis (index 0 is not read): stack_patch_dims'
// formula on the affine extent pos - neg (with two terms per row the sum of their magnitudes, bit for bit) plus umax - umin.  False: the
// extent is absurd or the patch exceeds kStackAffinePatchCap.  Float64 additions, floor and comparisons only: host and device agree.
__host__ __device__ __forceinline__ bool warp_stack_patch(const ExtractEntry& e, const float (&umin)[3], const float (&umax)[3], int halo2,
                                                          int (&L)[2])
{
#pragma unroll
    for (int r = 1; r <= 2; ++r) {
        const double spread = (double)umax[r] - (double)umin[r];
        const double ext = (e.pos[r] - e.neg[r]) + spread;
        if (!(ext < 4096.0)) return false;
        L[r - 1] = (int)floor(ext + 2.0 * kBoxMargin) + 3 + halo2;
    }
    L[1] = (L[1] + 3 + 3) & ~3;                              // origin aligned down by up to 3, stride multiple of 4
    return (int64_t)L[0] * L[1] * 4 <= (int64_t)kStackAffinePatchCap;
}

// the tile's geometry, wave-uniform
struct WarpStackGeo {
    int cl1, cl2;              // first cell of the node block per axis
    int nn2;                   // nodes per row of the block
    int su1, su2;              // node strides (floats) of the block; 0 on an axis with one node
    int gm2_1, gm2_2;          // g_k - 2, at least 0
    int o1, o2;                // origin of the staged patch
    int Lx;                    // its row stride
};

// The lerps along axis 2 of the two node rows of cell row c1, per component: what the pixels of one column share while their cell row
// stays the same.
struct WarpStackRowLerp {
    int c1;                    // the cell row the values belong to (-1: none yet)
    double x0[2], x1[2];
};

__device__ __forceinline__ void warp_stack_row_lerp(const float* __restrict__ nodes, const WarpStackGeo& g, const int c1, const int c2,
                                                    const double f2, WarpStackRowLerp& rl)
{
    const float* const q = nodes + 2 * (g.nn2 * (c1 - g.cl1) + (c2 - g.cl2));
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double a00 = (double)q[c], a01 = (double)q[g.su2 + c], a10 = (double)q[g.su1 + c], a11 = (double)q[g.su1 + g.su2 + c];
        rl.x0[c] = fma(f2, a01 - a00, a00);
        rl.x1[c] = fma(f2, a11 - a10, a10);
    }
    rl.c1 = c1;
}

}  // namespace vt
