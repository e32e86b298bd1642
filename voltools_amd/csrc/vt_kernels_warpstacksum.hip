// vt_kernels_warpstacksum.hip -- the images of a resident stack, each resampled through its own 2-D displacement grid, summed under g
// weight columns without being written (kind 26), hand-written for gfx950 (MI355X, CDNA4): the motion-corrected sum of a movie, its
// even / odd half sums and exposure-window sums from one sampling of every frame.
//
// With B_i[h, w] exactly the float32 sample of kind 22 (vt_kernels_warpstack.hip: the chain, the grid rule, the inside test with 0
// outside, the same (floor, fraction), the same route per (entry, tile)),
//     out[c, h, w] = float32(b + sum_i W[i, c] * B_i[h, w]),   i ascending, every term added as weighted_add defines it (product rounded, sum rounded)
// with b = +0, or double(out[c, h, w]) as found with `accumulate`.  A pixel that maps outside image i adds nothing (kind 22 writes +0
// there, and +0 added to a sum that started at +0 moves no bit).  Column c is the host loop acc = b; acc = acc + W[i, c] * double(S_i)
// over kind 22's unweighted images S_i, rounded to float32 once.
//
// One 256-thread workgroup per (chunk of GC = kWarpStackSumChunk consecutive columns, 2-D output tile), grid = chunks x tiles chunk-major
// through xcd_contiguous; tile and thread mapping are kind 22's (BoxTileMap<1, TH, TW>, stack_affine_pick_tile).  The workgroup walks the
// n entries in ascending order and keeps acc[GC][NJ] float64 in registers.  Per entry the steps are kind 22's: the tile's nodes in LDS,
// their range per component, the class of the widened bounding box, the route (the entry's flag, warp_hull_granted, the tile's own patch
// by warp_stack_patch against kStackAffinePatchCap), stage_patch or the global-memory gather, per pixel warp_split, the shared row lerp,
// sample_patch<KIND> / direct_sample_2d<KIND>.  The node range is reduced by every wave for itself over the whole block (minima and
// maxima do not depend on the order), so no scratch and no barrier go into it.
//
// An entry is PASSED OVER -- not staged, not sampled -- when its weights are exactly 0 in all of the workgroup's columns (where the host
// loop would add 0 x B: nothing for a finite B, NaN for a non-finite one) or when its tile is classified wholly outside.  Otherwise
// every column of the chunk takes the weighted addition, a zero weight included, as the host loop does.
//
// Dynamic LDS: NB node blocks of hd.node_floats floats (NB = 1 with a shared grid, else 3), then two patch buffers of patch_floats each:
//     lds_bytes = 4 * (NB * node_floats + 2 * patch_floats)
// node_floats and the patch allocation are warp_stack_plan's.
//
// Schedule.  N[k] are the node blocks, P[k] the patch buffers, round i serves entry i:
//     prologue   node DMA of entry 0 -> N[0] and of entry 1 -> N[1]; wait, barrier; range, class and route of entry 0; its patch DMA
//                -> P[0]; wait, barrier
//     round i    (a) range, class and route of entry i + 1 from N[(i + 1) % 3]; its patch DMA -> P[(i + 1) & 1]
//                (b) node DMA of entry i + 2 -> N[(i + 2) % 3]
//                (c) entry i sampled from N[i % 3] and P[i & 1] into the accumulators
//                (d) s_waitcnt vmcnt(0), one barrier
// so the next patch and the nodes after next are in flight while the current entry is sampled.  With a shared grid the one block is
// loaded and ranged in the prologue and (b) falls away.  Why no buffer is overwritten while it is read: P[(i + 1) & 1] was last read in
// step (c) of round i - 1 and N[(i + 2) % 3] = N[(i - 1) % 3] in steps (a) of round i - 2 and (c) of round i - 1, all before the barrier
// (d) of round i - 1, which every wave has passed before round i issues anything.  Why everything read has landed: what round i reads in
// (a) and (c) was issued in round i - 1 or earlier, and every wave waited for its own DMA before the barrier (d) of round i - 1.
// Every condition on the way (an entry passed over, gathered or staged) is workgroup-uniform -- entries, weights and header come by
// scalar loads, the ranges through readfirstlane -- and the barrier (d) is executed in every round whatever the entry did.  The schedule
// moves loads in time and nothing else: no value that reaches an accumulator depends on it.
#include "vt_backproject_common.h"
#include "vt_warp_common.h"

#include <algorithm>

namespace vt {

// The tile's nodes, nn1 rows of nn2 nodes from cell (cl1, cl2) of a g1 x g2 grid, to blk by LDS-DMA, lane-linear (float f of the block
// lands at blk + f).  Every address read lies inside the grid: warp_cells ends at node g_k - 1.
__device__ __forceinline__ void stage_nodes(float* blk, const float* __restrict__ grid, const int g2, const int cl1, const int cl2,
                                            const int nn1, const int nn2, const int tid)
{
    const int row_f = 2 * nn2, total = nn1 * row_f;
    const int wave_first = __builtin_amdgcn_readfirstlane(tid & ~63);
    int f = tid;
    for (int fb = wave_first; fb < total; fb += 256, f += 256) {
        const int b = f / row_f, c = f - b * row_f;
        const float* gp = grid + (((int64_t)(cl1 + b) * g2 + cl2) * 2 + c);
        if (f < total)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)gp,
                                             (__attribute__((address_space(3))) void*)(blk + fb), 4, 0, 0);
    }
}

// The range per component of the `total` nodes of blk, by this wave alone, the same value in every lane (kept scalar).  Indexed by source
// axis as kind 22's are; an image has no axis 0.
__device__ __forceinline__ void node_range(const float* blk, const int total, const int lane, float (&umin)[3], float (&umax)[3])
{
    float mn[2] = {INFINITY, INFINITY}, mx[2] = {-INFINITY, -INFINITY};
    for (int i = lane; i < total; i += 64) {
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const float x = blk[2 * i + k];
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
    umin[0] = umax[0] = 0.0f;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        umin[k + 1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mn[k])));
        umax[k + 1] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(mx[k])));
    }
}

// what a round knows of its entry on this tile, workgroup-uniform
struct WarpSumRound {
    bool active;               // sampled: a non-zero weight in the chunk and the tile not wholly outside
    bool stage;                // from the staged patch (else gathered from global memory)
    bool whole;                // no pixel needs a test
    int o1, o2;                // origin of the staged patch
    int Ly, Lx;                // its dims
};

// Class and route of entry e on the tile at (h0, w0) whose nodes span [umin, umax]: kind 22's steps 3 and 4, the same expressions.
// patch_floats: the allocation, which a tile that passes the cap fits (warp_stack_plan); the comparison only keeps a staged patch inside
// its buffer whatever the host did.
template <int HALO, int TH, int TW>
__device__ __forceinline__ WarpSumRound warp_sum_round(const ExtractEntry& e, const AffineParams& p, const float (&umin)[3],
                                                       const float (&umax)[3], const int gm1_max, const int h0, const int w0,
                                                       const bool nonzero, const int patch_floats)
{
    WarpSumRound r;
    const bool hull = warp_hull_granted(umin, umax, gm1_max);
    int L[2] = {0, 0};
    const bool stage = e.tiled && hull && warp_stack_patch(e, umin, umax, 2 * HALO, L);
    double lo[3] = {0.0, 0.0, 0.0};
    bool any_valid = true, all_valid = true;
#pragma unroll
    for (int k = 1; k <= 2; ++k) {
        const double base = fma(e.m[4 * k + 1], (double)h0, fma(e.m[4 * k + 2], (double)w0, e.m[4 * k + 3]));
        lo[k] = base + e.neg[k] + (double)umin[k];
        const double hi = base + e.pos[k] + (double)umax[k];
        any_valid = any_valid && (hi >= p.vlo[k] - kTileMargin) && (lo[k] < p.vhi[k] + kTileMargin);
        all_valid = all_valid && (lo[k] >= p.vlo[k] + kTileMargin) && (hi < p.vhi[k] - kTileMargin);
    }
    r.active = nonzero && !(hull && !any_valid);
    r.stage = r.active && stage && L[0] * L[1] <= patch_floats;
    r.whole = all_valid && (h0 + TH <= p.oH) && (w0 + TW <= p.oW);
    r.o1 = r.o2 = 0;
    r.Ly = L[0];
    r.Lx = L[1];
    if (r.stage) {                                           // finite and small: the tile meets the valid interval, its extent is bounded
        r.o1 = (int)floor(lo[1] - kBoxMargin) - HALO;
        r.o2 = ((int)floor(lo[2] - kBoxMargin) - HALO) & ~3;
    }
    return r;
}

// weighted_add's expression, acc + w * v with the product rounded to float64 and then the sum, with the product passed through
// rounded(): here the accumulator lives in registers across the walk over the entries, and with -ffp-contract=fast the backend fused
// weighted_add's product into the addition (v_fma_f64) although its pragma forbids the contraction -- one rounding, and a float32 result
// that differs from the host loop's wherever the float64 sum lands on a float32 tie.  The empty asm makes the product a value of its own.
__device__ __forceinline__ double weighted_add_kept(double acc, double w, float v)
{
    return acc + rounded(w * (double)v);
}

// One pixel (h, w) of the output: kind 22's warp_stack_pixel up to the sample, which is returned unweighted.  False: the pixel maps
// outside the image (val is not to be read).
template <int KIND, bool STAGED, bool WHOLE>
__device__ __forceinline__ bool warp_sum_sample(const float* __restrict__ nodes, const float* __restrict__ patch,
                                                const float* __restrict__ img, const ExtractEntry& e, const WarpStackHeader& hd,
                                                const AffineParams& p, const WarpStackGeo& g, const int h, const int w, const int c2,
                                                const double f2, WarpStackRowLerp& rl, float& val)
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
        val = sample_patch<KIND>(patch, g.Lx, (int)fyd - g.o1, (int)fxd - g.o2, fy, fx);
        return inside;
    } else {
        if (!inside) return false;
        val = direct_sample_2d<KIND>(img, p, (int)fyd, (int)fxd, fy, fx);
        return true;
    }
}

// The thread's NJ pixels (h_first + jj * RP, w) of one entry added into the accumulators.  A pixel of the tile beyond the output is
// passed over (its column split is taken at the last column inside, so that no node beyond the block is named).
template <int KIND, int GC, int NJ, int RP, bool STAGED, bool WHOLE>
__device__ __forceinline__ void warp_sum_rows(const float* __restrict__ nodes, const float* __restrict__ patch,
                                              const float* __restrict__ img, const ExtractEntry& e, const WarpStackHeader& hd,
                                              const double (&wt)[GC], const AffineParams& p, const WarpStackGeo& g, const int h_first,
                                              const int w, double (&acc)[GC][NJ])
{
    const int wc = WHOLE ? w : min(w, p.oW - 1);
    int c2;
    double f2;
    warp_split(wc, hd.r[1], g.gm2_2, c2, f2);
    WarpStackRowLerp rl;
    rl.c1 = -1;
    rl.x0[0] = rl.x0[1] = rl.x1[0] = rl.x1[1] = 0.0;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h_first + jj * RP;
        if (!WHOLE && !(h < p.oH && w < p.oW)) continue;
        float val = 0.0f;
        if (warp_sum_sample<KIND, STAGED, WHOLE>(nodes, patch, img, e, hd, p, g, h, w, c2, f2, rl, val)) {
#pragma unroll
            for (int k = 0; k < GC; ++k) acc[k][jj] = weighted_add_kept(acc[k][jj], wt[k], val);
        }
    }
}

// p.nTh / nTw = tiles of one output image (p.nTd = 1), p.oH / oW = the image; gridDim.x = column chunks x tiles, `tiles` = p.nTh * p.nTw.
// wts: n x gcols, C order.  out: gcols images.  grids: hd.n_grids grids of g[0] x g[1] x 2 floats; n_grids == 1: shared by every entry.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TH, int TW>
__global__ __launch_bounds__(256) void warp_stack_sum_tiled(const float* __restrict__ src, float* __restrict__ out,
                                                             const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                             const double* __restrict__ wts, const WarpStackHeader* __restrict__ hdr,
                                                             const float* __restrict__ grids, const int n, const int gcols,
                                                             const int tiles, const int patch_floats, const int accumulate,
                                                             const AffineParams p)
{
    using M = BoxTileMap<1, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP;
    constexpr int HALO = KIND != 0 ? 1 : 0;
    constexpr int GC = kWarpStackSumChunk;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x, lane = tid & 63;
    int u = xcd_contiguous(blockIdx.x, gridDim.x);
    const int chunk = u / tiles;                             // workgroup-uniform
    u -= chunk * tiles;
    const int c0 = chunk * GC, cnt = min(GC, gcols - c0);
    const WarpStackHeader& hd = *hdr;
    const int g1 = hd.g[0], g2 = hd.g[1];
    const bool own = hd.n_grids != 1;                        // a grid per entry: three node blocks in rotation
    const int64_t per_grid = (int64_t)g1 * g2 * 2;
    const int64_t image = (int64_t)p.oH * p.oW;
    const int64_t istride = (int64_t)p.sH * p.sP;
    out += (int64_t)c0 * image;                              // 64-bit: g images pass 2^31 pixels long before one does
    wts += c0;
    int d0, h0, w0;
    M::tile_origin(u, p, d0, h0, w0);
    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int w = w0 + kw;

    WarpStackGeo g;
    int nn1;
    warp_cells(h0, min(h0 + TH, p.oH) - 1, hd.r[0], g1, g.cl1, nn1);
    warp_cells(w0, min(w0 + TW, p.oW) - 1, hd.r[1], g2, g.cl2, g.nn2);
    const int total = nn1 * g.nn2;                           // <= (TH + 1)(TW + 1)
    g.su2 = g2 > 1 ? 2 : 0;
    g.su1 = g1 > 1 ? 2 * g.nn2 : 0;
    g.gm2_1 = max(g1 - 2, 0);
    g.gm2_2 = max(g2 - 2, 0);
    g.o1 = g.o2 = g.Lx = 0;

    float* const pbuf = lds + (own ? 3 : 1) * hd.node_floats;     // 16-byte aligned: node_floats is a multiple of 4
    float* nb_cur = lds;                                     // N[i % 3], N[(i + 1) % 3], N[(i + 2) % 3] of round i
    float* nb_nxt = own ? lds + hd.node_floats : lds;
    float* nb_aft = own ? lds + 2 * hd.node_floats : lds;

    double acc[GC][NJ];                                      // statically indexed throughout: registers
#pragma unroll
    for (int k = 0; k < GC; ++k)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) acc[k][jj] = 0.0;

    // ---- prologue ----
    stage_nodes(nb_cur, grids, g2, g.cl1, g.cl2, nn1, g.nn2, tid);
    if (own && n > 1) stage_nodes(nb_nxt, grids + per_grid, g2, g.cl1, g.cl2, nn1, g.nn2, tid);
    if (accumulate) {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP;
            if (h >= p.oH || w >= p.oW) continue;
#pragma unroll
            for (int k = 0; k < GC; ++k)
                if (k < cnt) acc[k][jj] = (double)out[k * image + (int64_t)h * p.oW + w];
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");         // the node DMA has landed (and accumulate's pre-load) ...
    __syncthreads();                                         // ... in every wave

    float umin[3], umax[3];
    node_range(nb_cur, total, lane, umin, umax);             // shared grid: the range of every round
    WarpSumRound cur;
    {
        bool nz = false;
#pragma unroll
        for (int k = 0; k < GC; ++k) nz = nz || (k < cnt && wts[k] != 0.0);
        cur = warp_sum_round<HALO, TH, TW>(tab[0], p, umin, umax, hd.gm1_max, h0, w0, nz, patch_floats);
        if (cur.stage)
            stage_patch(pbuf, src + (int64_t)(int)tab[0].m[3] * istride, zeros16, p, cur.o1, cur.o2, cur.Ly, cur.Lx, tid);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();

    bool touched = false;                                    // workgroup-uniform: some entry was sampled
    int cur_buf = 0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        // ---- (a) the next entry: range, class, route, its patch sets off into the other buffer ----
        WarpSumRound nxt;
        nxt.active = nxt.stage = nxt.whole = false;
        nxt.o1 = nxt.o2 = nxt.Ly = nxt.Lx = 0;
        if (i + 1 < n) {
            const ExtractEntry& en = tab[i + 1];             // wave-uniform index: scalar loads
            const double* wn = wts + (int64_t)(i + 1) * gcols;
            bool nz = false;
#pragma unroll
            for (int k = 0; k < GC; ++k) nz = nz || (k < cnt && wn[k] != 0.0);
            if (own) node_range(nb_nxt, total, lane, umin, umax);
            nxt = warp_sum_round<HALO, TH, TW>(en, p, umin, umax, hd.gm1_max, h0, w0, nz, patch_floats);
            if (nxt.stage)
                stage_patch(pbuf + (cur_buf ^ 1) * patch_floats, src + (int64_t)(int)en.m[3] * istride, zeros16, p, nxt.o1, nxt.o2, nxt.Ly,
                            nxt.Lx, tid);
        }
        // ---- (b) the nodes of the entry after next ----
        if (own && i + 2 < n) stage_nodes(nb_aft, grids + (int64_t)(i + 2) * per_grid, g2, g.cl1, g.cl2, nn1, g.nn2, tid);

        // ---- (c) entry i ----
        if (cur.active) {
            touched = true;
            const ExtractEntry& e = tab[i];
            const double* wi = wts + (int64_t)i * gcols;
            double wt[GC];
#pragma unroll
            for (int k = 0; k < GC; ++k) wt[k] = k < cnt ? wi[k] : 0.0;
            const float* img = src + (int64_t)(int)e.m[3] * istride;
            const float* patch = pbuf + cur_buf * patch_floats;
            g.o1 = cur.o1;
            g.o2 = cur.o2;
            g.Lx = cur.Lx;
            if (!cur.stage)
                warp_sum_rows<KIND, GC, NJ, RP, false, false>(nb_cur, patch, img, e, hd, wt, p, g, h0 + jh0, w, acc);
            else if (cur.whole)
                warp_sum_rows<KIND, GC, NJ, RP, true, true>(nb_cur, patch, img, e, hd, wt, p, g, h0 + jh0, w, acc);
            else
                warp_sum_rows<KIND, GC, NJ, RP, true, false>(nb_cur, patch, img, e, hd, wt, p, g, h0 + jh0, w, acc);
        }

        // ---- (d) ----
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next patch and the nodes after next have landed ...
        __syncthreads();                                     // ... in every wave, and every read of this round's buffers is done
        cur = nxt;
        cur_buf ^= 1;
        float* const t = nb_cur;
        nb_cur = nb_nxt;
        nb_nxt = nb_aft;
        nb_aft = t;
    }

    if (accumulate && !touched) return;                      // the output holds b already
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h0 + jh0 + jj * RP;
        if (h >= p.oH || w >= p.oW) continue;
#pragma unroll
        for (int k = 0; k < GC; ++k)
            if (k < cnt) out[k * image + (int64_t)h * p.oW + w] = (float)acc[k][jj];
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace {

using WarpStackSumFn = void (*)(const float*, float*, const float*, const ExtractEntry*, const double*, const WarpStackHeader*, const float*,
                                int, int, int, int, int, AffineParams);
const WarpStackSumFn warp_stack_sum_kernels[2][3] = {
    {warp_stack_sum_tiled<0, 32, 32>, warp_stack_sum_tiled<1, 32, 32>, warp_stack_sum_tiled<2, 32, 32>},
    {warp_stack_sum_tiled<0, 16, 16>, warp_stack_sum_tiled<1, 16, 16>, warp_stack_sum_tiled<2, 16, 16>},
};

}  // namespace

// every instantiation may allocate the whole 160 KiB of dynamic LDS (three node blocks and two patches at the cap pass 64 KiB)
hipError_t init_warp_stack_sum_kernels()
{
    for (int cfg = 0; cfg < 2; ++cfg)
        for (int kind = 0; kind < 3; ++kind) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(warp_stack_sum_kernels[cfg][kind]),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

int warp_stack_sum_lds_bytes(const WarpStackHeader& hd, int patch_bytes)
{
    return 4 * (hd.n_grids == 1 ? 1 : 3) * hd.node_floats + 2 * patch_bytes;
}

// grid = column chunks x p.nTh x p.nTw workgroups, chunk-major.  lds_bytes = warp_stack_sum_lds_bytes.
hipError_t launch_warp_stack_sum(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                                 const double* d_wts, const WarpStackHeader* d_hdr, const float* d_grids, int n, int g, int patch_bytes,
                                 bool accumulate, const AffineParams& p, int lds_bytes, hipStream_t stream)
{
    const int64_t tiles = (int64_t)p.nTh * p.nTw;
    const int64_t chunks = ((int64_t)g + kWarpStackSumChunk - 1) / kWarpStackSumChunk;
    if (n <= 0 || g <= 0 || tiles <= 0 || p.nTd != 1 || chunks * tiles > 0x7fffffffLL || patch_bytes < 0 || (patch_bytes & 15) ||
        lds_bytes < 2 * patch_bytes || lds_bytes > 160 * 1024)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(warp_stack_sum_kernels[cfg][interp_kind(interp)], dim3((unsigned)(chunks * tiles)), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, d_hdr, d_grids, n, g, (int)tiles, patch_bytes / 4, accumulate ? 1 : 0, p);
    return hipGetLastError();
}

}  // namespace vt
