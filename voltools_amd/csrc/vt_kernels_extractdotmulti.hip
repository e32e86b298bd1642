// vt_kernels_extractdotmulti.hip -- per-box scores of n extracted boxes against k templates in one launch (kind 15), hand-written for gfx950
// (MI355X, CDNA4).
//
// out[i] = (sum_v mask[v] * B_i[v], sum_v mask[v] * B_i[v]^2, sum_v tmpls[0][v] * B_i[v], .., sum_v tmpls[k-1][v] * B_i[v]) in float64, with
// B_i the float32 box extract_tiled (vt_kernels_extract.hip) writes for matrix i: what classifying n candidate (position, orientation)
// pairs against k references under one mask needs.  Columns 0, 1 and 2 + j hold the bits extract_dot_tiled (vt_kernels_extractdot.hip,
// kind 14) writes into its columns 0, 1, 2 for template j; the difference is that each (matrix, box tile) is staged once and each
// (matrix, voxel) sampled once, whatever k is:
//
//   * One 256-thread workgroup per (matrix, box tile) pair, ids, entries, tile, staging, stepping and inside tests as extract_dot_tiled
//     (vt_box_common.h holds them once, with rounded() and wave_tree_sum()).
//   * Sampling phase: a thread owns NJ x DPT voxels (4, 8 or 16) and keeps their samples in registers (every loop over them is fully
//     unrolled).  A voxel that maps outside, or lies beyond the end of the box, is held as +0.
//   * Scoring phase, without the LDS box: columns are served three at a time (S0, S1 and template 0 first, then templates 1..3, 4..6,
//     ..), each by the accumulation extract_dot_tiled performs -- products through rounded(), every addition rounded, a thread's voxels
//     in (in-plane pass, plane) order, the fixed 256-lane tree -- and one write into part[matrix][tile][2 + k].  A held +0 adds a
//     term of +-0 (template and mask are finite), which leaves the bits of a sum that started at +0 as they are: the sums never become
//     -0 in round-to-nearest.  Voxels beyond the end of the box read template voxel 0 instead of their own, for the same +-0.
//   * Template j is addressed by a 64-bit scalar base (tmpls + j * box voxels) plus extract_dot_tiled's 32-bit voxel offset.
//   * The cross-wave step overlays the first 96 bytes of the staged box once every gather is done, three columns per pass: the launch
//     allocates no LDS beyond extract_tiled's (at least 96 bytes), and the entries are routed exactly as extract_tiled routes them.
//   * extract_dot_multi_reduce adds the tiles of a box in ascending tile index, one thread per output number.  No atomics.
#include "vt_box_common.h"

#include <algorithm>

namespace vt {

// Sixteen held samples times three columns are 48 template loads with 48 64-bit addresses: 226 VGPRs.  The offsets of the second eight
// voxels are made to wait for the sums over the first eight, so that only 24 loads and their addresses are live at a time.
template <int NV>
__device__ __forceinline__ void score_fence(double& a0, double& a1, double& a2, int (&off)[NV])
{
    if constexpr (NV == 16)
        asm volatile("" : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(off[8]), "+v"(off[9]), "+v"(off[10]), "+v"(off[11]), "+v"(off[12]), "+v"(off[13]),
                     "+v"(off[14]), "+v"(off[15]));
}

// p.nTd / nTh / nTw = box tiles, p.oD / oH / oW = box shape; part holds [box][tile][2 + k] doubles of this launch.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void extract_dot_multi_tiled(const float* __restrict__ src, double* __restrict__ part,
                                                                const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                                const float* __restrict__ tmpls, const float* __restrict__ mask,
                                                                const int k, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT, NV = M::NV;
    static_assert(NV <= 16, "held samples per thread");
    constexpr int SCORE_CHUNK = 8;                       // voxels whose template loads (three columns each) are in flight together
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tiles = p.nTd * p.nTh * p.nTw;
    const int box = t / tiles;                           // wave-uniform: the entry is read with scalar loads
    int d0, h0, w0;
    M::tile_origin(t - box * tiles, p, d0, h0, w0);
    const ExtractEntry& e = tab[box];
    const int ostride = p.oH * p.oW;                     // the box has fewer than 2^31 voxels (checked on the host): 32-bit voxel offsets
    const int ncol = 2 + k;
    double* const my_part = part + (int64_t)t * ncol;

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int nd = min(DPT, p.oD - d0 - i0);             // planes this thread owns (<= 0: none)

    float val[NV];                                       // the samples of this thread's voxels, (in-plane pass, plane) order; +0: none
#pragma unroll
    for (int q = 0; q < NV; ++q) val[q] = 0.0f;

    if (!e.tiled) {
        // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
#pragma unroll
            for (int i = 0; i < DPT; ++i) {
                if (i >= nd) continue;
                const int d = d0 + i0 + i;
                double s[3];
                bool inside = true;
                VT_CANONICAL_INSIDE(inside, s[r_], e, p, d, h, w);
                if (inside) {
                    const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                    val[jj * DPT + i] = direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd), (float)(s[1] - fyd), (float)(s[2] - fxd));
                }
            }
        }
    } else {
        double base[3], lo[3];
        bool any_valid = true, all_valid = true;
        VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0);

        if (!any_valid) {                                // the whole tile maps outside the valid interval: nothing staged, a zero partial
            for (int c = tid; c < ncol; c += 256) my_part[c] = 0.0;      // workgroup-uniform exit, ahead of every barrier
            return;
        }
        int o[3];
        box_origin<HALO>(lo, o);

        const int Lx = e.Lx, Ly = e.Ly, Lz = e.Lz;
        stage_box(lds, src, zeros16, p, o, Lz, Ly, Lx, tid);
        __syncthreads();     // hipcc drains the direct-to-LDS loads (vmcnt(0)) ahead of the barrier

        double b[3];
        box_base(base, o, b);
        const int LyLx = Ly * Lx;
        const FxInc3 inc = fx_inc3(e);
        const bool whole = all_valid && (p.oD - d0 >= TD);   // wave-uniform

#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = jh0 + jj * RP;
            const int h = h0 + j, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            Fx c0, c1, c2;
            fx_start3(e, b, i0, j, kw, c0, c1, c2);
            if (whole) {
#pragma unroll
                for (int i = 0; i < DPT; ++i) {
                    float s = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                    // one cubic sample in flight: the next plane's coordinates wait for this sample (two cost kernel 14 250 VGPRs)
                    // (four trilinear ones, kernel 14's UNR)
                    if (CUBIC || (i & 3) == 3) asm volatile("" : "+v"(s), "+v"(c0.hi), "+v"(c1.hi), "+v"(c2.hi));
                    val[jj * DPT + i] = s;
                    fx_step3(c0, c1, c2, inc);
                }
            } else {
                // tiles cut by the valid interval or by the end of the box: the inside test is the canonical chain, the taps still come
                // from the fixed-point split
#pragma unroll
                for (int i = 0; i < DPT; ++i) {
                    if (i >= nd) continue;
                    float s = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                    int d = d0 + i0 + i;
                    // the float64 chain starts once the sample is complete, and so do the next plane's taps
                    asm volatile("" : "+v"(d), "+v"(s), "+v"(c0.hi), "+v"(c1.hi), "+v"(c2.hi));
                    double sd;
                    bool inside = true;
                    VT_CANONICAL_INSIDE(inside, sd, e, p, d, h, w);
                    val[jj * DPT + i] = inside ? s : 0.0f;
                    fx_step3(c0, c1, c2, inc);
                }
            }
        }
    }

    // ---- scoring: no LDS box from here on ----
    // voxel offsets of the held samples; a voxel beyond the end of the box (its sample is +0) reads voxel 0, which exists
    int off[NV];                                         // (not const: score_fence passes some through an asm statement)
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h0 + jh0 + jj * RP, w = w0 + kw;
        const bool in_plane = h < p.oH && w < p.oW;
        const int vox = ((d0 + i0) * p.oH + h) * p.oW + w;
#pragma unroll
        for (int i = 0; i < DPT; ++i) off[jj * DPT + i] = (in_plane && i < nd) ? vox + i * ostride : 0;
    }
    const int64_t tvox = (int64_t)p.oD * ostride;        // voxels of one template
    const bool has_mask = mask != nullptr;               // uniform
    double* red = reinterpret_cast<double*>(lds);
    const int wv = tid >> 6;

    for (int c = 0; c < ncol; c += 3) {                  // uniform: columns c, c + 1, c + 2 in one pass through the tree and the scratch
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
        if (c == 0) {                                    // S0, S1 and template 0: extract_dot_tiled's dot_add
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                if (q == SCORE_CHUNK) score_fence(a0, a1, a2, off);
                const float mk = has_mask ? mask[off[q]] : 1.0f;
                const float tp = tmpls[off[q]];
                const double bq = (double)val[q];
                const double mb = rounded((double)mk * bq);      // exact
                const double tb = rounded((double)tp * bq);      // exact
                const double mbb = rounded(mb * bq);             // rounded once
                a0 = a0 + mb;
                a1 = a1 + mbb;
                a2 = a2 + tb;
            }
        } else {                                         // templates c - 2, c - 1, c; a missing one repeats template c - 2 and is not written
            const float* __restrict__ t0 = tmpls + (int64_t)(c - 2) * tvox;
            const float* __restrict__ t1 = c + 1 < ncol ? t0 + tvox : t0;
            const float* __restrict__ t2 = c + 2 < ncol ? t0 + 2 * tvox : t0;
#pragma unroll
            for (int q = 0; q < NV; ++q) {
                if (q == SCORE_CHUNK) score_fence(a0, a1, a2, off);
                const double bq = (double)val[q];
                a0 = a0 + rounded((double)t0[off[q]] * bq);
                a1 = a1 + rounded((double)t1[off[q]] * bq);
                a2 = a2 + rounded((double)t2[off[q]] * bq);
            }
        }
        // 256 partial triples -> one, by extract_dot_tiled's tree
        a0 = wave_tree_sum(a0);
        a1 = wave_tree_sum(a1);
        a2 = wave_tree_sum(a2);
        __syncthreads();         // first pass: every gather of the staged box is done, its first 96 bytes become the cross-wave scratch;
                                 // later passes: the previous pass has read the scratch
        if ((tid & 63) == 0) { red[3 * wv] = a0; red[3 * wv + 1] = a1; red[3 * wv + 2] = a2; }
        __syncthreads();
        if (tid < 3 && c + tid < ncol) my_part[c + tid] = (red[tid] + red[3 + tid]) + (red[6 + tid] + red[9 + tid]);
    }
}

// out[i][c] = part[i][0][c] + part[i][1][c] + ... in ascending tile index; one thread per (box, column)
__global__ __launch_bounds__(256) void extract_dot_multi_reduce(const double* __restrict__ part, double* __restrict__ out, const int tiles,
                                                                 const int ncol, const int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int64_t i = g / ncol;
    const int c = (int)(g - i * ncol);
    const double* q = part + i * tiles * ncol + c;
    double acc = 0.0;
    for (int u = 0; u < tiles; ++u) acc = acc + q[(int64_t)u * ncol];
    out[g] = acc;
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

VT_BOX_KERNELS(extractdotmulti, extract_dot_multi_tiled<KIND, T::TD, T::TH, T::TW>)

// grid = box tiles x cnt workgroups, then one thread per output number; `part` holds cnt x tiles x (2 + k) doubles, `out` cnt x (2 + k).
hipError_t launch_extract_dot_multi(int cfg, int interp, const float* src, double* out, double* part, const float* zeros16,
                                    const ExtractEntry* d_tab, const float* d_tmpls, const float* d_mask, int k, int cnt,
                                    const AffineParams& p, int lds_bytes, hipStream_t stream)
{
    const int64_t tiles = (int64_t)p.nTd * p.nTh * p.nTw;
    const int64_t grid = tiles * cnt;
    if (cnt <= 0 || k <= 0 || k > 0x7fffffff - 2 || tiles <= 0 || grid > 0x7fffffffLL || !part || !out || !d_tmpls ||
        lds_bytes < extract_dot_min_lds() || lds_bytes > 160 * 1024)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(extractdotmulti_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, part, zeros16, d_tab, d_tmpls, d_mask, k, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t total = (int64_t)cnt * (2 + k);
    const int64_t blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extract_dot_multi_reduce, dim3((unsigned)blocks), dim3(256), 0, stream, part, out, (int)tiles, 2 + k, total);
    return hipGetLastError();
}

}  // namespace vt
