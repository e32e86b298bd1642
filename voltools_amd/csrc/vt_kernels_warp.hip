// vt_kernels_warp.hip -- resampling through a displacement grid (kind 20), hand-written for gfx950 (MI355X, CDNA4).
//
// out[v] = sample(src, s(v)),  s(v) = a(v) + u(v)  in float64, for every voxel v = (d, h, w) of an output of shape (oD, oH, oW):
//
//   a(v)   the canonical fma chain of the pull matrix (VT_CANONICAL_INSIDE's expression);
//   u(v)   the trilinear interpolation, in float64, of a control grid G of shape (gD, gH, gW, 3), float32, whose nodes span the output
//          corner to corner.  Per axis k:  r_k = (g_k - 1) / (o_k - 1)  (one float64 division on the host; 0 where g_k == 1),
//              q_k = v_k * r_k,   c_k = min(floor(q_k), g_k - 2),   f_k = q_k - c_k,
//          and per component  lerp(f, a, b) = fma(f, b - a, a)  along axis 2, then axis 1, then axis 0.  Where g_k == 1 the two nodes of
//          the lerp are the same node and f_k = 0 (fma(0, 0, a) = a).  Axis 0 goes last: a thread walks a column along the depth and keeps
//          the in-plane lerps of its two node planes while c_0 stays the same -- the same expression evaluated less often, so no bit moves.
//   inside the skirt rule on s, vlo <= s_r < vhi on every axis; outside voxels are written as +0;
//   value  the handle's interpolation at (int)floor(s_r), (float)(s_r - floor(s_r)) -- the split of extract's direct route, on BOTH routes
//          below.  sample_box<0> and direct_sample<0> are one expression, so the two routes of a trilinear handle agree bit for bit.  The
//          cubic kinds agree to tolerance only: cubic_gather_b64 (staged route) sums the 16 tap rows per column first, direct_sample sums
//          each row first.
//
// One 256-thread workgroup per output tile (the box family's tiles and thread mapping, vt_box_common.h), ids through xcd_contiguous.
// Per workgroup:
//   1. the nodes its voxels can touch -- per axis from the cell of the tile's first voxel to the cell of its last voxel inside the
//      output, plus one: at most floor((T_k - 1) r_k) + 2 <= T_k + 1 per axis -- go to LDS, three floats per node;
//   2. the per-component minimum and maximum over those nodes (umin, umax) are reduced across the workgroup;
//   3. trilinear interpolation stays inside the hull of its cell's nodes, so the tile's source bounding box is
//      [base + neg + umin, base + pos + umax] per axis.  The tile is classified against the valid interval with kTileMargin as
//      VT_BOX_TILE_GEOMETRY does; a tile wholly outside stores zeros;
//   4. the tile's own staged dims follow extract_box_dims' formula with the extent grown by umax - umin (warp_tile_box), the origin is
//      box_origin<HALO> of the widened lower corner.  A tile whose box fits kWarpBoxCap runs stage_box, a barrier, and per voxel s, its
//      split and sample_box<KIND> at (floor(s) - o, frac); the others gather from global memory in the same launch (extract_tiled's
//      !e.tiled branch plus the displacement).
//
// How far s can leave the hull box, and why kBoxMargin covers it.  q_k is the product of two rounded factors, so at the far end of an
// axis q_k <= (g_k - 1)(1 + 2^-52) and f_k exceeds 1 by at most (g_k - 1) 2^-52; each of the three lerp levels then extrapolates by at
// most that times the spread of its operands (<= 2 U, U the largest |node component| of the tile's nodes), and adds a rounding of at most
// 2^-53 relative to values bounded by 3 U.  The sum a + u and the corner sums base + neg + umin round at 2^-52 relative to coordinates that
// are below 2^14 on a tile that stages.  A tile takes the hull for granted only while  U (max_k g_k - 1) <= 2^20:  then s leaves
// [lo, hi] by less than 6 * 2^20 * 2^-52 + 2^-37 < 2^-29, far inside kBoxMargin = 2^-24 (and kTileMargin = 1e-6).  With that the proof of
// vt_device.h (kBoxMargin) carries over: floor(s) - o >= HALO and floor(s) + 1 + HALO - o <= L - 1 on every axis.  Beyond that magnitude
// -- for a dense 512^3 grid: displacements above 2051 voxels -- the tile is neither classified nor staged: it takes the global-memory
// route, where every voxel is tested and every tap is bounds-checked.
//
// The host sizes the launch from the same two functions (warp_cells of vt_warp_common.h, warp_tile_box), which hold float64 additions,
// one multiplication followed by floor, and comparisons only -- nothing a compiler may contract -- so host and device agree on every tile's dims to the bit.
// The rule depends on (M, G, shapes, interpolation) only; the source's valid interval decides what is SKIPPED, never what is sized.
#include "vt_box_common.h"
#include "vt_warp_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace vt {

// The staged box of a tile whose nodes span [umin, umax] per component: extract_box_dims' formula on the affine extent plus umax - umin.
// False: the tile gathers from global memory (hull bound not granted, extent absurd, or box beyond the cap).
__host__ __device__ __forceinline__ bool warp_tile_box(const double (&ext_affine)[3], const float (&umin)[3], const float (&umax)[3],
                                                       int halo2, int gm1_max, int (&L)[3])
{
    if (!warp_hull_granted(umin, umax, gm1_max)) return false;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double spread = (double)umax[r] - (double)umin[r];
        const double ext = ext_affine[r] + spread;
        if (!(ext < 4096.0)) return false;
        L[r] = (int)floor(ext + 2.0 * kBoxMargin) + 3 + halo2;
    }
    L[2] = (L[2] + 3 + 3) & ~3;
    return (int64_t)L[0] * L[1] * L[2] * 4 <= (int64_t)kWarpBoxCap;
}

// in-plane lerps of one node plane: axis 2, then axis 1, per component
__device__ __forceinline__ void warp_plane(const float* __restrict__ q, int su1, int su2, double f1, double f2, double (&y)[3])
{
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double a00 = (double)q[c], a01 = (double)q[su2 + c], a10 = (double)q[su1 + c], a11 = (double)q[su1 + su2 + c];
        const double x0 = fma(f2, a01 - a00, a00);
        const double x1 = fma(f2, a11 - a10, a10);
        y[c] = fma(f1, x1 - x0, x0);
    }
}

template <int KIND, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void warp_tiled(const float* __restrict__ src, float* __restrict__ out, const float* __restrict__ zeros16,
                                                   const WarpTable* __restrict__ tab, const float* __restrict__ grid, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT;
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const red = lds;                              // 4 waves x (3 minima, 3 maxima)
    float* const nodes = lds + kWarpScratchFloats;

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    int d0, h0, w0;
    M::tile_origin(t, p, d0, h0, w0);
    const WarpTable& wt = *tab;                          // wave-uniform: scalar loads
    const ExtractEntry& e = wt.e;
    const int64_t ostride = (int64_t)p.oH * p.oW;

    // ---- 1. the tile's nodes -> LDS, 2. their range per component ----
    int cl[3], nn[3];
    warp_cells(d0, min(d0 + TD, p.oD) - 1, wt.r[0], wt.g[0], cl[0], nn[0]);
    warp_cells(h0, min(h0 + TH, p.oH) - 1, wt.r[1], wt.g[1], cl[1], nn[1]);
    warp_cells(w0, min(w0 + TW, p.oW) - 1, wt.r[2], wt.g[2], cl[2], nn[2]);
    const int n12 = nn[1] * nn[2], total = nn[0] * n12;  // <= 17^3
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = tid; i < total; i += 256) {
        const int a = i / n12, rem = i - a * n12, b = rem / nn[2], c = rem - b * nn[2];
        const float* gp = grid + (((int64_t)(cl[0] + a) * wt.g[1] + (cl[1] + b)) * wt.g[2] + (cl[2] + c)) * 3;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float x = gp[k];
            nodes[3 * i + k] = x;
            mn[k] = fminf(mn[k], x);
            mx[k] = fmaxf(mx[k], x);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
        }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) { red[(tid >> 6) * 6 + k] = mn[k]; red[(tid >> 6) * 6 + 3 + k] = mx[k]; }
    }
    __syncthreads();                                     // nodes and the four partial ranges are in LDS
    float umin[3], umax[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float a = fminf(fminf(red[k], red[6 + k]), fminf(red[12 + k], red[18 + k]));
        const float b = fmaxf(fmaxf(red[3 + k], red[9 + k]), fmaxf(red[15 + k], red[21 + k]));
        umin[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a)));      // the same value in every lane: keep it scalar
        umax[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(b)));
    }

    // ---- 3. the widened bounding box, 4. the route ----
    const int gm1_max = max(max(wt.g[0], wt.g[1]), wt.g[2]) - 1;
    int L[3] = {0, 0, 0};
    const bool hull = warp_hull_granted(umin, umax, gm1_max);
    const bool stage = e.tiled && warp_tile_box(wt.ext, umin, umax, 2 * HALO, gm1_max, L);

    double base[3], lo[3];
    bool any_valid = true, all_valid = true;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        base[r] = fma(e.m[4 * r], (double)d0, fma(e.m[4 * r + 1], (double)h0, fma(e.m[4 * r + 2], (double)w0, e.m[4 * r + 3])));
        lo[r] = base[r] + e.neg[r] + (double)umin[r];
        const double hi = base[r] + e.pos[r] + (double)umax[r];
        any_valid = any_valid && (hi >= p.vlo[r] - kTileMargin) && (lo[r] < p.vhi[r] + kTileMargin);
        all_valid = all_valid && (lo[r] >= p.vlo[r] + kTileMargin) && (hi < p.vhi[r] - kTileMargin);
    }

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int nd = min(DPT, p.oD - d0 - i0);             // planes this thread owns (<= 0: none)
    out += (int64_t)(d0 + i0) * ostride;

    if (hull && !any_valid) {
        // the whole tile maps outside the valid interval
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h < p.oH && w < p.oW) {
                float* optr = out + (int64_t)h * p.oW + w;
                for (int i = 0; i < nd; ++i, optr += ostride) *optr = 0.0f;
            }
        }
        return;
    }

    int o[3] = {0, 0, 0};
    float* const box = nodes + wt.node_floats;           // 16-byte aligned: kWarpScratchFloats and node_floats are multiples of 4
    if (stage) {                                         // workgroup-uniform
        box_origin<HALO>(lo, o);
        stage_box(box, src, zeros16, p, o, L[0], L[1], L[2], tid);
        __syncthreads();     // hipcc drains the direct-to-LDS loads (vmcnt(0)) ahead of the barrier
    }
    const int Lx = L[2], LyLx = L[1] * L[2];
    const bool whole = stage && all_valid;

    // node strides (floats) of the LDS block; an axis with one node lerps the node with itself
    const int su2 = wt.g[2] > 1 ? 3 : 0, su1 = wt.g[1] > 1 ? 3 * nn[2] : 0, su0 = wt.g[0] > 1 ? 3 * n12 : 0;
    const int gm2_0 = max(wt.g[0] - 2, 0), gm2_1 = max(wt.g[1] - 2, 0), gm2_2 = max(wt.g[2] - 2, 0);

    const int w = w0 + kw;
    int c2;
    double f2;
    warp_split(w, wt.r[2], gm2_2, c2, f2);

#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h0 + jh0 + jj * RP;
        if (h >= p.oH || w >= p.oW) continue;
        int c1;
        double f1;
        warp_split(h, wt.r[1], gm2_1, c1, f1);
        const float* const col = nodes + (3 * nn[2] * (c1 - cl[1]) + 3 * (c2 - cl[2]));
        float* optr = out + (int64_t)h * p.oW + w;
        int cur = -1;
        double ya[3], yb[3];
        for (int i = 0; i < nd; ++i) {
            const int d = d0 + i0 + i;
            int c0;
            double f0;
            warp_split(d, wt.r[0], gm2_0, c0, f0);
            if (c0 != cur) {                             // wave-uniform: d is
                const float* q = col + 3 * n12 * (c0 - cl[0]);
                warp_plane(q, su1, su2, f1, f2, ya);
                warp_plane(q + su0, su1, su2, f1, f2, yb);
                cur = c0;
            }
            double s[3];
            bool inside = true;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const double a = fma(e.m[4 * r], (double)d, fma(e.m[4 * r + 1], (double)h, fma(e.m[4 * r + 2], (double)w, e.m[4 * r + 3])));
                const double u = fma(f0, yb[r] - ya[r], ya[r]);
                s[r] = a + u;
                inside = inside && (s[r] >= p.vlo[r]) && (s[r] < p.vhi[r]);
            }
            float val = 0.0f;
            if (stage) {
                // every voxel of the tile lies in the staged box, inside the valid interval or not: the flag masks the value
                const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                const float smp = sample_box<KIND>(box, Lx, LyLx, (int)fzd - o[0], (int)fyd - o[1], (int)fxd - o[2],
                                                   (float)(s[0] - fzd), (float)(s[1] - fyd), (float)(s[2] - fxd));
                val = (whole || inside) ? smp : 0.0f;
            } else if (inside) {
                const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                val = direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd), (float)(s[1] - fyd), (float)(s[2] - fxd));
            }
            optr[i * ostride] = val;
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side: the per-tile range pass that sizes the launch, and the launcher
// ---------------------------------------------------------------------------------------------------
// Fills wt (entry, r, ext, g, node_floats) for matrix m (folded) and the grid, and reports the largest staged box (the first in
// tile order among equals).  Every distinct node block is scanned once.
void warp_plan(const double m[12], const float* grid, const int g[3], const int out_shape[3], int cfg, bool cubic, bool force_direct,
               WarpTable* wt, int L_max[3], int* lds_bytes)
{
    const int T[3] = {kExtractTiles[cfg].td, kExtractTiles[cfg].th, kExtractTiles[cfg].tw};
    extract_fill_entry(m, cfg, cubic, 0x7fffffff, force_direct, &wt->e);     // m, tile reach (the Q32.32 steps and dims are not read)
    wt->e.Lz = wt->e.Ly = wt->e.Lx = 0;
    for (int r = 0; r < 3; ++r) {
        double ext = 0;
        for (int k = 0; k < 3; ++k) ext += std::fabs(m[4 * r + k]) * (T[k] - 1);
        wt->ext[r] = ext;
        wt->r[r] = g[r] > 1 ? (double)(g[r] - 1) / (double)(out_shape[r] - 1) : 0.0;
        wt->g[r] = g[r];
    }
    wt->e.tiled = !force_direct && wt->ext[0] < 4096.0 && wt->ext[1] < 4096.0 && wt->ext[2] < 4096.0;
    wt->pad_[0] = wt->pad_[1] = wt->pad_[2] = wt->pad_[3] = 0;
    const int gm1_max = std::max(std::max(g[0], g[1]), g[2]) - 1;
    const int halo2 = cubic ? 2 : 0;
    int nT[3];
    for (int k = 0; k < 3; ++k) nT[k] = (out_shape[k] + T[k] - 1) / T[k];

    // Cells and node counts of the tiles, per axis.  Neighbouring tiles inside one cell of a coarse grid see the same nodes, hence the same
    // box: only the distinct (first cell, count) pairs are kept, in tile order, and the pass below visits their combinations.
    std::vector<int> cl[3], cn[3];
    for (int k = 0; k < 3; ++k)
        for (int a = 0; a < nT[k]; ++a) {
            int c_lo, n;
            warp_cells(a * T[k], std::min((a + 1) * T[k], out_shape[k]) - 1, wt->r[k], g[k], c_lo, n);
            if (cl[k].empty() || cl[k].back() != c_lo || cn[k].back() != n) { cl[k].push_back(c_lo); cn[k].push_back(n); }
        }
    for (int k = 0; k < 3; ++k) nT[k] = (int)cl[k].size();
    int64_t best_bytes = 0;
    L_max[0] = L_max[1] = L_max[2] = 0;
    const int64_t nodes_max = (int64_t)*std::max_element(cn[0].begin(), cn[0].end()) * *std::max_element(cn[1].begin(), cn[1].end()) *
                              *std::max_element(cn[2].begin(), cn[2].end());      // the counts are per axis: the largest block is their product
    for (int a = 0; a < nT[0] && wt->e.tiled; ++a)
        for (int b = 0; b < nT[1]; ++b)
            for (int c = 0; c < nT[2]; ++c) {
                const int n0 = cn[0][a], n1 = cn[1][b], n2 = cn[2][c];
                // (the values are finite: plain comparisons are fmin / fmax)
                float umin[3] = {INFINITY, INFINITY, INFINITY}, umax[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int i = 0; i < n0; ++i)
                    for (int j = 0; j < n1; ++j) {
                        const float* row = grid + (((int64_t)(cl[0][a] + i) * g[1] + (cl[1][b] + j)) * g[2] + cl[2][c]) * 3;
                        for (int k = 0; k < n2; ++k, row += 3)
                            for (int q = 0; q < 3; ++q) {
                                umin[q] = row[q] < umin[q] ? row[q] : umin[q];
                                umax[q] = row[q] > umax[q] ? row[q] : umax[q];
                            }
                    }
                int L[3];
                if (!warp_tile_box(wt->ext, umin, umax, halo2, gm1_max, L)) continue;
                const int64_t bytes = (int64_t)L[0] * L[1] * L[2] * 4;
                if (bytes > best_bytes) { best_bytes = bytes; L_max[0] = L[0]; L_max[1] = L[1]; L_max[2] = L[2]; }
            }
    wt->node_floats = (int)((3 * nodes_max + 3) & ~(int64_t)3);
    *lds_bytes = (int)((kWarpScratchFloats + wt->node_floats) * 4 + best_bytes);
}

VT_BOX_KERNELS(warp, warp_tiled<KIND, T::TD, T::TH, T::TW>)

hipError_t launch_warp(int cfg, int interp, const float* src, float* out, const float* zeros16, const WarpTable* d_tab, const float* d_grid,
                       const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream)
{
    if (grid <= 0 || grid > 0x7fffffffLL || lds_bytes > 160 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_grid, p);
    return hipGetLastError();
}

}  // namespace vt
