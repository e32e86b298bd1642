// vt_kernels_extractsummulti.hip -- g weighted sums of the same n extracted boxes in one launch (kind 16), hand-written for gfx950
// (MI355X, CDNA4).
//
// out[j][d, h, w] = float32(sum_i weights[i][j] * B_i[d, h, w]) with B_i the float32 box extract_tiled (vt_kernels_extract.hip) writes for
// matrix i: the class averages of a classification round, half-set maps, bootstrap replicas.  Box j holds the bits extract_sum_tiled
// (vt_kernels_extractsum.hip, kind 13) writes for column j of the weights alone; the difference is that a (matrix, box tile) pair is
// staged and sampled once per chunk of GC columns instead of once per column:
//
//   * One 256-thread workgroup per (segment of consecutive matrices, chunk of GC consecutive columns, box tile); ids are XCD-contiguous,
//     segment-major, then chunk, the tile fastest: the chunks of one segment are neighbours on one XCD and walk the same matrices, hence
//     the same source voxels, at about the same time.  Segments and tile are extract_sum_shape_plan's, whatever g is.
//   * Per matrix, in ascending order: ExtractEntry and the chunk's GC weights (contiguous in the row-major table) by scalar loads; a
//     matrix whose GC weights are all zero is passed over before anything is staged.  Otherwise geometry, staging, stepping and inside
//     tests as extract_sum_tiled (vt_box_common.h holds them once, with weighted_add), entries that gather from global memory included.
//   * Sampling phase: a thread owns NJ x DPT voxels (4, 8 or 16) and keeps their samples in registers (every loop over them is fully
//     unrolled).  A voxel that maps outside, or lies beyond the end of the box, is held as +0.
//   * Accumulation phase, without the LDS box: acc[c][q] = weighted_add(acc[c][q], w[c], val[q]) for the chunk's columns, GC x NV float64
//     accumulators in registers, statically indexed.  A held +0 adds a term of +-0 where extract_sum_tiled adds nothing; a sum that
//     started at +0 never becomes -0 in round-to-nearest, so its bits stay as they are.  No two lanes share a voxel: no atomics, no
//     exchange through LDS.
//   * A launch with one segment rounds to float32 and stores into out[j]; otherwise the workgroup stores float64 partials
//     part[j][segment][d][h][w] and project_reduce adds the segments of each box in ascending order and rounds once.  Both are addressed
//     from a 64-bit base per column.  The columns a ragged last chunk lacks take weight 0 and are not stored.
#include "vt_box_common.h"

#include <algorithm>

namespace vt {

// direct_sample<KIND> (vt_device.h) with its arithmetic and order kept, and the four tap planes of a cubic sample made to follow one another:
// the finished plane sum and the tap origin pass through one empty asm statement, so that the next plane's 16 addresses wait for it.  All
// 64 loads in flight at once set kernel 13's register peak; here the accumulators of GC columns sit on top of it.
template <int KIND>
__device__ __forceinline__ float direct_sample_by_planes(const float* __restrict__ src, const AffineParams& p, int iz, int iy, int ix,
                                                         float fz, float fy, float fx)
{
    if constexpr (KIND == 0) {
        return direct_sample<0>(src, p, iz, iy, ix, fz, fy, fx);
    } else {
        float wx[4], wy[4], wz[4];
        cubic_weights<KIND == 2>(fx, wx);
        cubic_weights<KIND == 2>(fy, wy);
        cubic_weights<KIND == 2>(fz, wz);
        float val = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float accy = 0.f;
#pragma unroll
            for (int bb = 0; bb < 4; ++bb) {
                float accx = wx[0] * fetch0(src, p, iz - 1 + c, iy - 1 + bb, ix - 1);
                accx = fmaf(wx[1], fetch0(src, p, iz - 1 + c, iy - 1 + bb, ix), accx);
                accx = fmaf(wx[2], fetch0(src, p, iz - 1 + c, iy - 1 + bb, ix + 1), accx);
                accx = fmaf(wx[3], fetch0(src, p, iz - 1 + c, iy - 1 + bb, ix + 2), accx);
                accy = fmaf(wy[bb], accx, accy);
            }
            val = fmaf(wz[c], accy, val);
            asm volatile("" : "+v"(val), "+v"(iz), "+v"(iy), "+v"(ix));
        }
        return val;
    }
}

// p.nTd / nTh / nTw = box tiles, p.oD / oH / oW = box shape; n matrices in nseg segments of per_seg consecutive ones; wts[i * g + j] with
// gc columns j served by this launch (wts, out and part already point at its first column).
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW, int GC>
__global__ __launch_bounds__(256) void extract_sum_multi_tiled(const float* __restrict__ src, float* __restrict__ out, double* __restrict__ part,
                                                                const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                                const double* __restrict__ wts, const int n, const int per_seg,
                                                                const int nseg, const int g, const int gc, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT, NV = M::NV;
    static_assert(NV <= 16, "held samples per thread");
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tiles = p.nTd * p.nTh * p.nTw;
    const int nchunk = (gc + GC - 1) / GC;
    const int sc = t / tiles;                            // segment-major, then chunk, then tile
    const int u = t - sc * tiles;
    const int seg = sc / nchunk;
    const int c0 = __builtin_amdgcn_readfirstlane((sc - seg * nchunk) * GC);      // first column of the chunk (within the launch)
    int d0, h0, w0;
    M::tile_origin(u, p, d0, h0, w0);
    const int64_t ostride = (int64_t)p.oH * p.oW;

    double acc[GC * NV];                                 // statically indexed throughout: registers
#pragma unroll
    for (int k = 0; k < GC * NV; ++k) acc[k] = 0.0;

    const int m_first = seg * per_seg;
    const int m_end = min(m_first + per_seg, n);
#pragma unroll 1
    for (int mi = m_first; mi < m_end; ++mi) {
        const ExtractEntry& e = tab[mi];                 // wave-uniform index: scalar loads
        const double* wrow = wts + (int64_t)mi * g + c0;
        bool any_w = false;
#pragma unroll
        for (int c = 0; c < GC; ++c) any_w = any_w || (c0 + c < gc && wrow[c] != 0.0);
        if (!any_w) continue;                            // workgroup-uniform, ahead of every barrier: nothing staged, nothing added
        // the weights are read again once the samples are held: GC scalar pairs would otherwise stay live across the whole sampling phase
        int c0w = c0;
        asm volatile("" : "+s"(c0w));
        wrow = wts + (int64_t)mi * g + c0w;

        // the thread's place in the tile is worked out again for every matrix (a few integer operations): derived from an opaque copy of
        // tid, it and the float64 forms of it are not carried through the loop in registers next to the accumulators
        int tl = tid;
        asm volatile("" : "+v"(tl));
        int kw, jh0, i0;
        M::thread_origin(tl, kw, jh0, i0);
        const int nd = min(DPT, p.oD - d0 - i0);         // planes this thread owns (<= 0: none)
        float val[NV];                                   // the samples of this thread's voxels, (in-plane pass, plane) order; +0: none
#pragma unroll
        for (int q = 0; q < NV; ++q) val[q] = 0.0f;

        if (!e.tiled) {
            // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int h = h0 + jh0 + jj * RP, w = w0 + kw;
                if (h >= p.oH || w >= p.oW) continue;
                // the plane loop is not unrolled (DPT cubic global gathers, extract_sum_tiled's reason); the held samples rotate by one per
                // plane instead so that they stay statically indexed, DPT steps = identity
#pragma unroll 1
                for (int i = 0; i < DPT; ++i) {
                    float a = 0.0f;
                    if (i < nd) {
                        const int d = d0 + i0 + i;
                        double s[3];
                        bool inside = true;
                        VT_CANONICAL_INSIDE(inside, s[r_], e, p, d, h, w);
                        if (inside) {
                            const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                            a = direct_sample_by_planes<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd), (float)(s[1] - fyd), (float)(s[2] - fxd));
                        }
                    }
#pragma unroll
                    for (int k = 0; k + 1 < DPT; ++k) val[jj * DPT + k] = val[jj * DPT + k + 1];
                    val[jj * DPT + DPT - 1] = a;
                }
            }
        } else {
            double base[3], lo[3];
            bool any_valid = true, all_valid = true;
            VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0);
            if (!any_valid) continue;                    // the whole tile maps outside the valid interval: nothing staged, nothing added

            int o[3];
            box_origin<HALO>(lo, o);

            const int Lx = e.Lx, Ly = e.Ly, Lz = e.Lz;
            stage_box(lds, src, zeros16, p, o, Lz, Ly, Lx, tl);
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
                        // one cubic sample in flight: the next plane's coordinates wait for this sample (kernels 14 and 15's fence; four
                        // trilinear ones, kernel 13's UNR)
                        if (CUBIC || (i & 3) == 3) asm volatile("" : "+v"(s), "+v"(c0.hi), "+v"(c1.hi), "+v"(c2.hi));
                        val[jj * DPT + i] = s;
                        fx_step3(c0, c1, c2, inc);
                    }
                } else {
                    // tiles cut by the valid interval or by the end of the box: the inside test is the canonical chain, the taps still
                    // come from the fixed-point split
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
            __syncthreads();     // every gather of this box is done before the next one is staged
        }

        // ---- accumulation: no LDS box from here on ----
#pragma unroll
        for (int c = 0; c < GC; ++c) {
            const double wt = c0 + c < gc ? wrow[c] : 0.0;      // a ragged chunk's missing columns: weight 0, never stored
#pragma unroll
            for (int q = 0; q < NV; ++q) acc[c * NV + q] = weighted_add(acc[c * NV + q], wt, val[q]);
        }
    }

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int nd = min(DPT, p.oD - d0 - i0);
    const int64_t nvox = (int64_t)p.oD * ostride;
#pragma unroll
    for (int c = 0; c < GC; ++c) {
        if (c0 + c >= gc) continue;                      // uniform
        float* __restrict__ out_c = out + (int64_t)(c0 + c) * nvox;                          // 64-bit bases per column
        double* __restrict__ part_c = part + ((int64_t)(c0 + c) * nseg + seg) * nvox;
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            const int64_t vox = ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
#pragma unroll
            for (int i = 0; i < DPT; ++i) {
                if (i >= nd) continue;
                if (nseg == 1) out_c[vox + i * ostride] = (float)acc[c * NV + jj * DPT + i];
                else part_c[vox + i * ostride] = acc[c * NV + jj * DPT + i];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

// columns per workgroup for each tile of the extraction kernel's table: GC x voxels per thread = 32 float64 accumulators
constexpr int sum_multi_chunk(int cfg) { return cfg == 0 ? 2 : (cfg == 1 ? 4 : 8); }
int extract_sum_multi_chunk(int cfg) { return sum_multi_chunk(cfg); }

VT_BOX_KERNELS(extractsummulti, extract_sum_multi_tiled<KIND, T::TD, T::TH, T::TW, sum_multi_chunk(CFG)>)

// grid = box tiles x column chunks x nseg workgroups for the gc columns that start at d_wts[0] (row stride g); `out` is the first of
// their boxes; with nseg > 1 `part` holds gc x nseg x box voxels doubles and the caller follows with
// launch_project_reduce(part, out, nseg, box voxels, gc, stream).
hipError_t launch_extract_sum_multi(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                                    const ExtractEntry* d_tab, const double* d_wts, int n, int per_seg, int nseg, int g, int gc,
                                    const AffineParams& p, int lds_bytes, hipStream_t stream)
{
    const int GC = extract_sum_multi_chunk(cfg);
    if (gc <= 0 || g < gc) return hipErrorInvalidValue;
    const int64_t chunks = ((int64_t)gc + GC - 1) / GC;
    const int64_t tiles = (int64_t)p.nTd * p.nTh * p.nTw;
    if (tiles <= 0 || tiles > 0x7fffffffLL || nseg <= 0 || tiles * nseg > 0x7fffffffLL) return hipErrorInvalidValue;
    const int64_t grid = tiles * nseg * chunks;
    if (grid > 0x7fffffffLL || n <= 0 || per_seg <= 0 || (int64_t)per_seg * nseg < n || (nseg > 1 && !part)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extractsummulti_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, part, zeros16, d_tab, d_wts, n, per_seg, nseg, g, gc, p);
    return hipGetLastError();
}

}  // namespace vt
