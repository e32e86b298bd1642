// vt_kernels_warpstack.hip -- every image of a resident stack resampled through its own 2-D displacement grid (kind 22), hand-written for
// gfx950 (MI355X, CDNA4): patch-based motion correction of movie frames, per-tilt deformation, a lens distortion shared by every image.
//
// The handle holds T images of H x W as its planes.  For output pixel (h, w) of output image i, in float64,
//     a_y = fma(M_i[1,1], h, fma(M_i[1,2], w, M_i[1,3])),  a_x likewise with row 2                   (kind 21's chain)
//     u   = the bilinear interpolation of grid G_i (gH x gW x 2 float32; component 0 moves y, component 1 moves x), whose nodes span
//           the output image corner to corner.  Per in-plane axis k:  r_k = (g_k - 1) / (o_k - 1)  (one division on the host; 0 where
//           g_k == 1),  q_k = v_k * r_k (rounded),  c_k = min(floor(q_k), g_k - 2),  f_k = q_k - c_k,  and per component
//           lerp(f, a, b) = fma(f, b - a, a) along axis 2, then axis 1.  Where g_k == 1 both nodes of the lerp are the one node and f_k = 0.
//     y = a_y + u_y,  x = a_x + u_x
//     out[i, h, w] = float32(weighted_add(+0.0, w_i, B))  where -0.5 <= y < H - 0.5 and -0.5 <= x < W - 0.5, else +0
// with B kind 21's: the handle's interpolation in two dimensions in image planes[i] at ((int)floor(y), (float)(y - floor(y))), the same
// for x.  This is kind 20's grid rule on axes 1 and 2 added to kind 21's pixel.
//
// One 256-thread workgroup per (entry, 2-D output tile), grid = n x tiles entry-major through xcd_contiguous; tile, thread mapping and
// the staging of ONE patch are kind 21's (BoxTileMap<1, TH, TW>, stack_affine_pick_tile, stage_patch, kStackAffinePatchCap).  The entry,
// its weight and the grid header are read by wave-uniform scalar loads.  Per workgroup:
//   1. the nodes its pixels can touch (warp_cells on axes 1 and 2, from the cell of the tile's first pixel to the cell of its last pixel
//      inside the output, plus one: at most (TH + 1)(TW + 1) nodes of two floats) go to LDS behind the 128 bytes of reduction scratch;
//   2. the per-component minimum and maximum over those nodes are reduced across the workgroup (wave shuffles, four partials through
//      LDS, readfirstlane);
//   3. the tile's source bounding box [base + neg + umin, base + pos + umax] is classified against the valid interval with kTileMargin:
//      wholly outside -> zeros; cut -> every pixel is tested; whole -> none is;
//   4. the tile stages iff the entry's flag is set (host: affine extents below 4096, chain terms below 2^24 over the output, no
//      VT_FORCE_DIRECT), the hull is granted (U (max(gH, gW) - 1) <= kWarpHullLimit, U the largest |node component| of the tile's
//      nodes) and its own patch -- stack_patch_dims' formula with each extent grown by umax - umin -- fits kStackAffinePatchCap.  The
//      origin is floor(lo - kBoxMargin) - HALO, x & ~3.  A staged tile runs stage_patch, s_waitcnt vmcnt(0), one barrier; its loop is
//      branch-free as kind 21's is (the inside test selects).  Every other tile gathers with direct_sample_2d<KIND> in the same launch,
//      every pixel tested, every tap bounds-checked;
//   5. per pixel: the chain, the two splits (warp_split: q through rounded(), so that -ffp-contract=fast cannot fuse it into q - c), the
//      bilinear lerp of the LDS nodes in float64, the sums, floor and fraction, then sample_patch<KIND> or direct_sample_2d<KIND> on the
//      same (floor, fraction).  sample_patch<0> and direct_sample_2d<0> are one expression: a linear handle writes the same bits on both
//      routes.  A pixel of the tile beyond the output is evaluated at the last pixel inside it (its own cell may lie beyond the node
//      block) and not stored.  A thread's pixels share a column, so the lerps along axis 2 are formed again only when the cell row
//      changes: the same expression evaluated less often, as kind 20 does along the depth.
//
// Why every tap of a staged tile lies in its patch (the margin argument of vt_kernels_warp.hip in two dimensions).  q_k is the product of
// two rounded factors, so at the far end of an axis q_k <= (g_k - 1)(1 + 2^-52) and f_k exceeds 1 by at most (g_k - 1) 2^-52.  Each of the
// TWO lerp levels extrapolates by at most that times the spread of its operands (<= 2 U) and adds a rounding of at most 2^-53 relative to
// values bounded by 3 U.  With the same hull limit, U (max_k g_k - 1) <= 2^20, the interpolated u leaves [umin, umax] by less than
// 2 (2 * 2^20 * 2^-52 + 3 * 2^20 * 2^-53) < 2^-29.  The chain (kind 21's bound): its terms stay below 2^24 over the output on an entry that
// carries the flag, so the six roundings of a pixel's chain and of the tile's base together stay below 6 * 2^-29.  The sums a + u and
// base + neg + umin are three roundings of values below 2^25 + 2^20 (a single node, max_k g_k = 1, has no limit on U, but a tile that
// stages meets the valid interval, hence |u| < 2^26 there): at most 2^-27 each.  Together s leaves [lo, hi] by less than
// 3 * 2^-27 + 7 * 2^-29 < 2^-24 = kBoxMargin, and hi - lo = ext up to the same roundings.  With that the proof of vt_device.h (kBoxMargin)
// carries over per axis: o = floor(lo - kBoxMargin) - HALO gives floor(s) - o >= HALO, and L = floor(ext + 2 kBoxMargin) + 3 + 2 HALO gives
// floor(s) + 1 + HALO - o <= L - 1; on x the origin moves down by at most 3 for the 16-byte loads, which the + 3 of Lx pays for.
//
// The host sizes the launch without walking tiles x node blocks: the node block is (largest count over the tile rows) x (largest count
// over the tile columns), and the patch allocation is the largest bound over the entries that carry the flag, an entry's bound being the
// patch formula with the range of its WHOLE grid (found in the one pass over the nodes that also checks them and copies them to the
// tables).  A tile's range lies inside its grid's and the formula is monotone, so a tile that passes the cap fits the allocation; an
// entry whose bound exceeds the cap (or 4096) sets the allocation to the cap.
#include "vt_backproject_common.h"
#include "vt_warp_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vt {

// warp_stack_patch, WarpStackGeo and the row lerp live in vt_warp_common.h: kind 26 (vt_kernels_warpstacksum.hip) runs the same text.

// One pixel (h, w) of the output: the chain, the displacement from the node block in LDS, the inside test (WHOLE: none), the sample.
// A thread's pixels lie in one column, so the lerps along axis 2 are formed again only when the cell row changes (rl) -- the same
// expression evaluated less often, no bit moves; on a coarse grid that is most of the float64 work of a pixel.
// STAGED: every pixel of the tile has its taps in the staged patch, so the sample is taken without a branch and the test selects.
// !STAGED: taps from global memory, only for a pixel that passes the test (the caller passes pixels of the output only).
template <int KIND, bool STAGED, bool WHOLE>
__device__ __forceinline__ float warp_stack_pixel(const float* __restrict__ nodes, const float* __restrict__ patch,
                                                  const float* __restrict__ img, const ExtractEntry& e, const WarpStackHeader& hd,
                                                  const double wt, const AffineParams& p, const WarpStackGeo& g, const int h, const int w,
                                                  const int c2, const double f2, WarpStackRowLerp& rl)
{
    static_assert(STAGED || !WHOLE, "the global-memory route tests every pixel");
    int c1;
    double f1;
    warp_split(h, hd.r[0], g.gm2_1, c1, f1);
    if (c1 != rl.c1) warp_stack_row_lerp(nodes, g, c1, c2, f2, rl);
    const double uy = fma(f1, rl.x1[0] - rl.x0[0], rl.x0[0]);
    const double ux = fma(f1, rl.x1[1] - rl.x0[1], rl.x0[1]);
    const double y = fma(e.m[5], (double)h, fma(e.m[6], (double)w, e.m[7])) + uy;
    const double x = fma(e.m[9], (double)h, fma(e.m[10], (double)w, e.m[11])) + ux;
    const bool inside = WHOLE || ((y >= p.vlo[1]) && (y < p.vhi[1]) && (x >= p.vlo[2]) && (x < p.vhi[2]));
    const double fyd = floor(y), fxd = floor(x);
    const float fy = (float)(y - fyd), fx = (float)(x - fxd);
    if constexpr (STAGED) {
        const float val = sample_patch<KIND>(patch, g.Lx, (int)fyd - g.o1, (int)fxd - g.o2, fy, fx);
        return inside ? (float)weighted_add(0.0, wt, val) : 0.0f;
    } else {
        if (!inside) return 0.0f;
        return (float)weighted_add(0.0, wt, direct_sample_2d<KIND>(img, p, (int)fyd, (int)fxd, fy, fx));
    }
}

// The thread's NJ pixels (h_first + jj * RP, w).  Linear from the patch: unrolled, the NJ gathers in flight together, stores at the end.
// Cubic from the patch and the global-memory route: one pixel at a time (kind 21's finding on registers).
template <int KIND, int NJ, int RP, bool STAGED, bool WHOLE>
__device__ __forceinline__ void warp_stack_rows(const float* __restrict__ nodes, const float* __restrict__ patch,
                                                const float* __restrict__ img, float* __restrict__ out, const ExtractEntry& e,
                                                const WarpStackHeader& hd, const double wt, const AffineParams& p, const WarpStackGeo& g,
                                                const int h_first, const int w)
{
    // a pixel of the tile beyond the output is evaluated at the last pixel inside it: its taps lie in the patch, its nodes in the block
    const int wc = WHOLE ? w : min(w, p.oW - 1);
    int c2;
    double f2;
    warp_split(wc, hd.r[1], g.gm2_2, c2, f2);
    WarpStackRowLerp rl;
    rl.c1 = -1;
    rl.x0[0] = rl.x0[1] = rl.x1[0] = rl.x1[1] = 0.0;
    if constexpr (KIND == 0 && STAGED) {
        float r[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h_first + jj * RP;
            r[jj] = warp_stack_pixel<KIND, STAGED, WHOLE>(nodes, patch, img, e, hd, wt, p, g, WHOLE ? h : min(h, p.oH - 1), wc, c2, f2, rl);
        }
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h_first + jj * RP;
            if (WHOLE || (h < p.oH && w < p.oW)) out[(int64_t)h * p.oW + w] = r[jj];
        }
    } else {
#pragma unroll 1
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h_first + jj * RP;
            if (!WHOLE && !(h < p.oH && w < p.oW)) continue;
            out[(int64_t)h * p.oW + w] = warp_stack_pixel<KIND, STAGED, WHOLE>(nodes, patch, img, e, hd, wt, p, g, h, w, c2, f2, rl);
        }
    }
}

// p.nTh / nTw = tiles of one output image (p.nTd = 1), p.oH / oW = the image; gridDim.x = n x tiles, `tiles` = p.nTh * p.nTw.
// Dynamic LDS: kWarpScratchFloats of scratch, hd.node_floats of nodes, then the patch allocation.  grids: hd.n_grids grids of
// g[0] x g[1] x 2 floats; n_grids == 1: shared by every entry.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TH, int TW>
__global__ __launch_bounds__(256) void warp_stack_tiled(const float* __restrict__ src, float* __restrict__ out,
                                                         const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                         const double* __restrict__ wts, const WarpStackHeader* __restrict__ hdr,
                                                         const float* __restrict__ grids, const int tiles, const AffineParams p)
{
    using M = BoxTileMap<1, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP;
    constexpr int HALO = KIND != 0 ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* const red = lds;                                  // 4 waves x (2 minima, 2 maxima)
    float* const nodes = lds + kWarpScratchFloats;

    const int tid = threadIdx.x;
    int u = xcd_contiguous(blockIdx.x, gridDim.x);
    const int ent = u / tiles;                               // workgroup-uniform
    u -= ent * tiles;
    const ExtractEntry& e = tab[ent];                        // wave-uniform index: scalar loads
    const WarpStackHeader& hd = *hdr;
    const double wt = wts[ent];
    out += (int64_t)ent * ((int64_t)p.oH * p.oW);            // 64-bit: n images pass 2^31 pixels long before one does
    const int g1 = hd.g[0], g2 = hd.g[1];
    const float* const grid = grids + (hd.n_grids == 1 ? (int64_t)0 : (int64_t)ent * ((int64_t)g1 * g2 * 2));
    int d0, h0, w0;
    M::tile_origin(u, p, d0, h0, w0);
    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int w = w0 + kw;

    // ---- 1. the tile's nodes -> LDS, 2. their range per component ----
    WarpStackGeo g;
    int nn1;
    warp_cells(h0, min(h0 + TH, p.oH) - 1, hd.r[0], g1, g.cl1, nn1);
    warp_cells(w0, min(w0 + TW, p.oW) - 1, hd.r[1], g2, g.cl2, g.nn2);
    const int total = nn1 * g.nn2;                           // <= (TH + 1)(TW + 1)
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int i = tid; i < total; i += 256) {
        const int b = i / g.nn2, c = i - b * g.nn2;
        const float* gp = grid + ((int64_t)(g.cl1 + b) * g2 + (g.cl2 + c)) * 2;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float x = gp[k];
            nodes[2 * i + k] = x;
            mn[k] = fminf(mn[k], x);
            mx[k] = fmaxf(mx[k], x);
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            mn[k] = fminf(mn[k], __shfl_xor(mn[k], off, 64));
            mx[k] = fmaxf(mx[k], __shfl_xor(mx[k], off, 64));
        }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 2; ++k) { red[(tid >> 6) * 4 + k] = mn[k]; red[(tid >> 6) * 4 + 2 + k] = mx[k]; }
    }
    __syncthreads();                                         // nodes and the four partial ranges are in LDS
    float umin[3] = {0.0f, 0.0f, 0.0f}, umax[3] = {0.0f, 0.0f, 0.0f};       // indexed by source axis; an image has no axis 0
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float a = fminf(fminf(red[k], red[4 + k]), fminf(red[8 + k], red[12 + k]));
        const float b = fmaxf(fmaxf(red[2 + k], red[6 + k]), fmaxf(red[10 + k], red[14 + k]));
        umin[k + 1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a)));     // the same value in every lane: keep it scalar
        umax[k + 1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(b)));
    }

    // ---- 3. the widened bounding box and its class, 4. the route ----
    const bool hull = warp_hull_granted(umin, umax, hd.gm1_max);
    int L[2] = {0, 0};
    const bool stage = e.tiled && hull && warp_stack_patch(e, umin, umax, 2 * HALO, L);
    double lo[3] = {0.0, 0.0, 0.0};
    bool any_valid = true, all_valid = true;
#pragma unroll
    for (int r = 1; r <= 2; ++r) {
        const double base = fma(e.m[4 * r + 1], (double)h0, fma(e.m[4 * r + 2], (double)w0, e.m[4 * r + 3]));
        lo[r] = base + e.neg[r] + (double)umin[r];
        const double hi = base + e.pos[r] + (double)umax[r];
        any_valid = any_valid && (hi >= p.vlo[r] - kTileMargin) && (lo[r] < p.vhi[r] + kTileMargin);
        all_valid = all_valid && (lo[r] >= p.vlo[r] + kTileMargin) && (hi < p.vhi[r] - kTileMargin);
    }
    if (hull && !any_valid) {                                // the whole tile maps outside the image
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP;
            if (h < p.oH && w < p.oW) out[(int64_t)h * p.oW + w] = 0.0f;
        }
        return;
    }

    const float* img = src + (int64_t)(int)e.m[3] * ((int64_t)p.sH * p.sP);
    float* const patch = nodes + hd.node_floats;             // 16-byte aligned: kWarpScratchFloats and node_floats are multiples of 4
    g.o1 = g.o2 = 0;
    g.Lx = L[1];
    if (stage) {                                             // workgroup-uniform
        // finite and small: the tile meets the valid interval, its extent was bounded above
        g.o1 = (int)floor(lo[1] - kBoxMargin) - HALO;
        g.o2 = ((int)floor(lo[2] - kBoxMargin) - HALO) & ~3;
        stage_patch(patch, img, zeros16, p, g.o1, g.o2, L[0], L[1], tid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the LDS-DMA has landed ...
        __syncthreads();                                     // ... in every wave
    }
    g.su2 = g2 > 1 ? 2 : 0;
    g.su1 = g1 > 1 ? 2 * g.nn2 : 0;
    g.gm2_1 = max(g1 - 2, 0);
    g.gm2_2 = max(g2 - 2, 0);
    const bool whole = all_valid && (h0 + TH <= p.oH) && (w0 + TW <= p.oW);
    if (!stage)
        warp_stack_rows<KIND, NJ, RP, false, false>(nodes, patch, img, out, e, hd, wt, p, g, h0 + jh0, w);
    else if (whole)
        warp_stack_rows<KIND, NJ, RP, true, true>(nodes, patch, img, out, e, hd, wt, p, g, h0 + jh0, w);
    else
        warp_stack_rows<KIND, NJ, RP, true, false>(nodes, patch, img, out, e, hd, wt, p, g, h0 + jh0, w);
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace {

using WarpStackFn = void (*)(const float*, float*, const float*, const ExtractEntry*, const double*, const WarpStackHeader*, const float*, int,
                             AffineParams);
const WarpStackFn warp_stack_kernels[2][3] = {
    {warp_stack_tiled<0, 32, 32>, warp_stack_tiled<1, 32, 32>, warp_stack_tiled<2, 32, 32>},
    {warp_stack_tiled<0, 16, 16>, warp_stack_tiled<1, 16, 16>, warp_stack_tiled<2, 16, 16>},
};

}  // namespace

// One table entry: stack_affine_fill_entry's matrix rows, plane and tile reach.  `tiled` here is the entry's FLAG only -- affine extents
// below 4096, chain terms below 2^24 over the output, no VT_FORCE_DIRECT; whether a tile stages is decided by the tile, from its own nodes.
void warp_stack_fill_entry(const double rows[8], int plane, int cfg, bool cubic, int oh, int ow, bool force_direct, ExtractEntry* e)
{
    stack_affine_fill_entry(rows, plane, cfg, cubic, oh, ow, true, e);         // (its own cap does not apply)
    const bool small = std::fabs(e->m[5]) * oh + std::fabs(e->m[6]) * ow + std::fabs(e->m[7]) < 16777216.0 &&
                       std::fabs(e->m[9]) * oh + std::fabs(e->m[10]) * ow + std::fabs(e->m[11]) < 16777216.0;
    const bool bounded = e->pos[1] - e->neg[1] < 4096.0 && e->pos[2] - e->neg[2] < 4096.0;
    e->tiled = (!force_direct && small && bounded) ? 1 : 0;
}

// The range of `nodes` nodes (two floats each) folded into r = (min y, max y, min x, max x), which the caller starts at (+inf, -inf, +inf,
// -inf).  False: a component is not finite.  Eight independent lanes, so that the loop vectorises: a host pass over a dense field per image
// is what bounds such a call.  x * 0 is 0 for a finite x and NaN otherwise; comparisons drop a NaN, the sum keeps it.
bool warp_stack_grid_range(const float* q, size_t nodes, float r[4])
{
    float lo[8], hi[8], z[8];
    for (int j = 0; j < 8; ++j) { lo[j] = r[2 * (j & 1)]; hi[j] = r[2 * (j & 1) + 1]; z[j] = 0.0f; }
    const size_t nf = 2 * nodes;
    size_t k = 0;
    for (; k + 8 <= nf; k += 8)
        for (int j = 0; j < 8; ++j) {
            const float x = q[k + j];
            lo[j] = x < lo[j] ? x : lo[j];
            hi[j] = x > hi[j] ? x : hi[j];
            z[j] += x * 0.0f;
        }
    for (; k < nf; ++k) {                                    // (k and k & 7 have the same parity: the component)
        const float x = q[k];
        const int j = (int)(k & 7);
        lo[j] = x < lo[j] ? x : lo[j];
        hi[j] = x > hi[j] ? x : hi[j];
        z[j] += x * 0.0f;
    }
    bool finite = true;
    for (int j = 0; j < 8; ++j) {
        float& a = r[2 * (j & 1)];
        float& b = r[2 * (j & 1) + 1];
        a = lo[j] < a ? lo[j] : a;
        b = hi[j] > b ? hi[j] : b;
        finite = finite && z[j] == 0.0f;
    }
    return finite;
}

// The launch's node block and patch allocation (the header's sizing rule).  e: the n entries; ranges: warp_stack_grid_range's four floats
// per grid.  L_alloc: (Ly, Lx) of the allocation, (0, 0) when no entry carries the flag; *patch_bytes: its bytes.
void warp_stack_plan(const ExtractEntry* e, int n, const float* ranges, int n_grids, const int g[2], int cfg, bool cubic, int oh, int ow,
                     WarpStackHeader* hd, int L_alloc[2], int* patch_bytes)
{
    int T[2];
    stack_affine_tile(cfg, &T[0], &T[1]);
    const int o[2] = {oh, ow};
    int nn_max[2];
    for (int k = 0; k < 2; ++k) {
        hd->r[k] = g[k] > 1 ? (double)(g[k] - 1) / (double)(o[k] - 1) : 0.0;
        hd->g[k] = g[k];
        nn_max[k] = 0;
        for (int first = 0; first < o[k]; first += T[k]) {
            int c_lo, nn;
            warp_cells(first, std::min(first + T[k], o[k]) - 1, hd->r[k], g[k], c_lo, nn);
            nn_max[k] = std::max(nn_max[k], nn);
        }
    }
    hd->n_grids = n_grids;
    hd->gm1_max = std::max(g[0], g[1]) - 1;
    hd->node_floats = (2 * nn_max[0] * nn_max[1] + 3) & ~3;
    hd->pad_[0] = hd->pad_[1] = hd->pad_[2] = 0;

    L_alloc[0] = L_alloc[1] = 0;
    int64_t best = 0;
    bool capped = false;
    for (int i = 0; i < n; ++i) {
        if (!e[i].tiled) continue;
        const float* q = ranges + (n_grids > 1 ? 4 * (size_t)i : 0);
        const float lo[3] = {0.0f, q[0], q[2]}, hi[3] = {0.0f, q[1], q[3]};
        int L[2];
        if (!warp_stack_patch(e[i], lo, hi, cubic ? 2 : 0, L)) { capped = true; break; }
        const int64_t bytes = (int64_t)L[0] * L[1] * 4;
        if (bytes > best) { best = bytes; L_alloc[0] = L[0]; L_alloc[1] = L[1]; }
    }
    if (capped) { best = kStackAffinePatchCap; L_alloc[0] = kWarpStackCapLy; L_alloc[1] = kWarpStackCapLx; }
    *patch_bytes = (int)best;
}

// grid = n * p.nTh * p.nTw workgroups, entry-major.  lds_bytes = scratch + node block + patch allocation.
hipError_t launch_warp_stack(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                             const double* d_wts, const WarpStackHeader* d_hdr, const float* d_grids, int n, const AffineParams& p,
                             int lds_bytes, hipStream_t stream)
{
    const int64_t tiles = (int64_t)p.nTh * p.nTw;
    if (n <= 0 || tiles <= 0 || p.nTd != 1 || (int64_t)n * tiles > 0x7fffffffLL || lds_bytes < kWarpScratchFloats * 4 || lds_bytes > 64 * 1024)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_stack_kernels[cfg][interp_kind(interp)], dim3((unsigned)(n * tiles)), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, d_hdr, d_grids, (int)tiles, p);
    return hipGetLastError();
}

}  // namespace vt
