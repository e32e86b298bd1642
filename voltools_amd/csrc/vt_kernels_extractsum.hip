// vt_kernels_extractsum.hip -- weighted sum of n extracted boxes in one launch (kind 13), hand-written for gfx950 (MI355X, CDNA4).
//
// out[d, h, w] = float32(sum_i weights[i] * B_i[d, h, w]) with B_i the float32 box extract_tiled (vt_kernels_extract.hip) writes for
// matrix i: sub-tomogram averaging, or symmetrisation with the whole volume as the box, without ever writing the boxes.  The
// reference has no counterpart.  The kernel is extract_tiled with the store replaced by float64 registers, the reduction axis
// being the matrices (project_tiled, vt_kernels_projbatch.hip, reduces along the output depth instead):
//
//   * One 256-thread workgroup per (segment of consecutive matrices, box tile); ids are XCD-contiguous and segment-major, so
//     the tiles of one segment are neighbours on one XCD and walk the same matrices at about the same time.
//   * The thread mapping is extract_tiled's: a thread owns NJ * DPT output voxels of its tile and keeps one float64
//     accumulator for each (16 / 8 / 4 for the 16^3 / 8x16x16 / 8x8x16 tiles).  No two lanes share a voxel: no atomics, no
//     exchange through LDS.
//   * Per matrix, in ascending order: ExtractEntry and weight by scalar loads, float64 tile bounding box; a tile that clears
//     the valid interval adds nothing and stages nothing; otherwise stage_box, barrier, sample_box<KIND> with extract_tiled's
//     Q32.32 stepping (same restart points, hence the same float32 samples), barrier.  Tiles cut by the valid interval or by
//     the end of the box take the canonical float64 inside test.  Entries whose box fits no LDS allocation gather from global
//     memory (direct_sample<KIND>) inside the same loop.
//   * Every sample is widened to float64, multiplied by the float64 weight and added to its accumulator (two roundings, not a
//     fused multiply-add: the expression is the one a host loop in float64 evaluates).  A launch with one segment rounds to
//     float32 and stores; otherwise the workgroup stores float64 partials [segment][d][h][w] and project_reduce adds the
//     segments in ascending order and rounds once.
#include "vt_internal.h"
#include "vt_device.h"

#include <algorithm>

namespace vt {

// acc + w * v in float64 with both roundings (the translation unit is compiled with -ffp-contract=fast)
__device__ __forceinline__ double weighted_add(double acc, double w, float v)
{
#pragma clang fp contract(off)
    const double t = w * (double)v;
    return acc + t;
}

// p.nTd / nTh / nTw = box tiles, p.oD / oH / oW = box shape; n matrices in segments of per_seg consecutive ones.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void extract_sum_tiled(const float* __restrict__ src, float* __restrict__ out, double* __restrict__ part,
                                                          const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                          const double* __restrict__ wts, const int n, const int per_seg,
                                                          const AffineParams p)
{
    constexpr int NPOS = TH * TW;
    static_assert(256 % TW == 0 && (NPOS >= 256 ? NPOS % 256 == 0 : 256 % NPOS == 0), "tile/thread mapping");
    constexpr int DG = NPOS >= 256 ? 1 : 256 / NPOS;     // depth groups
    constexpr int NJ = NPOS >= 256 ? NPOS / 256 : 1;     // in-plane passes
    constexpr int RP = NPOS >= 256 ? 256 / TW : TH;      // tile rows covered per pass
    constexpr int DPT = TD / DG;                         // planes per thread
    static_assert(TD % DG == 0, "tile depth / lane groups");
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    constexpr int UNR = CUBIC ? 2 : 4;                   // samples in flight (project_tiled's: four cubic ones take one wave per SIMD)
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tiles = p.nTd * p.nTh * p.nTw;
    const int seg = t / tiles;                           // segment-major
    const int u = t - seg * tiles;
    const int tw_i = u % p.nTw;
    const int u2 = u / p.nTw;
    const int th_i = u2 % p.nTh;
    const int td_i = u2 / p.nTh;
    const int d0 = td_i * TD, h0 = th_i * TH, w0 = tw_i * TW;
    const int64_t ostride = (int64_t)p.oH * p.oW;

    const int pos = DG > 1 ? tid % NPOS : tid;
    const int kw = pos % TW;
    const int jh0 = pos / TW;
    const int i0 = DG > 1 ? (tid / NPOS) * DPT : 0;
    const int nd = min(DPT, p.oD - d0 - i0);             // planes this thread owns (<= 0: none)

    double acc[NJ * DPT];                                // statically indexed throughout: registers
#pragma unroll
    for (int k = 0; k < NJ * DPT; ++k) acc[k] = 0.0;

    const int m_first = seg * per_seg;
    const int m_end = min(m_first + per_seg, n);
#pragma unroll 1
    for (int mi = m_first; mi < m_end; ++mi) {
        const ExtractEntry& e = tab[mi];                 // wave-uniform index: scalar loads
        const double wt = wts[mi];

        if (!e.tiled) {
            // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct).  The plane loop
            // is not unrolled (DPT cubic global gathers); the accumulators rotate by one per plane instead, DPT steps = identity.
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int h = h0 + jh0 + jj * RP, w = w0 + kw;
                if (h >= p.oH || w >= p.oW) continue;
#pragma unroll 1
                for (int i = 0; i < DPT; ++i) {
                    double a = acc[jj * DPT];
                    if (i < nd) {
                        const int d = d0 + i0 + i;
                        double s[3];
                        bool inside = true;
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            s[r] = fma(e.m[4 * r], (double)d, fma(e.m[4 * r + 1], (double)h, fma(e.m[4 * r + 2], (double)w, e.m[4 * r + 3])));
                            inside = inside && (s[r] >= p.vlo[r]) && (s[r] < p.vhi[r]);
                        }
                        if (inside) {
                            const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                            a = weighted_add(a, wt, direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd),
                                                                        (float)(s[1] - fyd), (float)(s[2] - fxd)));
                        }
                    }
#pragma unroll
                    for (int k = 0; k + 1 < DPT; ++k) acc[jj * DPT + k] = acc[jj * DPT + k + 1];
                    acc[jj * DPT + DPT - 1] = a;
                }
            }
            continue;
        }

        // ---- tile geometry (wave-uniform, float64), as extract_tiled ----
        double base[3], lo[3], hi[3];
        bool any_valid = true, all_valid = true;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            base[r] = fma(e.m[4 * r], (double)d0, fma(e.m[4 * r + 1], (double)h0, fma(e.m[4 * r + 2], (double)w0, e.m[4 * r + 3])));
            lo[r] = base[r] + e.neg[r];
            hi[r] = base[r] + e.pos[r];
            any_valid = any_valid && (hi[r] >= p.vlo[r] - kTileMargin) && (lo[r] < p.vhi[r] + kTileMargin);
            all_valid = all_valid && (lo[r] >= p.vlo[r] + kTileMargin) && (hi[r] < p.vhi[r] - kTileMargin);
        }
        if (!any_valid) continue;                        // the whole tile maps outside the valid interval: nothing staged, nothing added

        // integer origin of the staged box (finite and small: the tile meets the valid interval, its extent was bounded on the host)
        int o[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) o[r] = (int)floor(lo[r] - kBoxMargin) - HALO;     // (vt_device.h: kBoxMargin)
        o[2] &= ~3;

        const int Lx = e.Lx, Ly = e.Ly, Lz = e.Lz;
        stage_box(lds, src, zeros16, p, o, Lz, Ly, Lx, tid);
        __syncthreads();     // hipcc drains the direct-to-LDS loads (vmcnt(0)) ahead of the barrier

        double b[3];
#pragma unroll
        for (int r = 0; r < 3; ++r) b[r] = base[r] - (double)o[r];
        const int LyLx = Ly * Lx;
        const int inc_hi0 = e.inc_hi[0], inc_hi1 = e.inc_hi[1], inc_hi2 = e.inc_hi[2];
        const unsigned inc_lo0 = e.inc_lo[0], inc_lo1 = e.inc_lo[1], inc_lo2 = e.inc_lo[2];
        const bool whole = all_valid && (p.oD - d0 >= TD);   // wave-uniform

#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = jh0 + jj * RP;
            const int h = h0 + j, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            const double s0 = fma(e.m[0], (double)i0, fma(e.m[1], (double)j, fma(e.m[2], (double)kw, b[0])));
            const double s1 = fma(e.m[4], (double)i0, fma(e.m[5], (double)j, fma(e.m[6], (double)kw, b[1])));
            const double s2 = fma(e.m[8], (double)i0, fma(e.m[9], (double)j, fma(e.m[10], (double)kw, b[2])));
            Fx c0 = to_fx(s0), c1 = to_fx(s1), c2 = to_fx(s2);
            // Every plane of the tile is sampled (the staged box covers the whole tile, as in extract_tiled, where cut tiles sample
            // before they mask); planes beyond the box and voxels that fail the inside test are not added.  UNR samples per trip; the
            // accumulators rotate by UNR per trip so that they are indexed statically (registers), DPT / UNR trips = identity.
            static_assert(DPT % UNR == 0, "planes per thread / unroll");
#pragma unroll 1
            for (int ib = 0; ib < DPT; ib += UNR) {
                double a[UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    bool inside = true;
                    if (!whole) {
                        // tiles cut by the valid interval or by the end of the box: the inside test is the canonical float64 chain
                        // (affine_direct's and the oracle's), the taps still come from the fixed-point split
                        const int d = d0 + i0 + ib + k;
                        inside = ib + k < nd;
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const double s = fma(e.m[4 * r], (double)d, fma(e.m[4 * r + 1], (double)h, fma(e.m[4 * r + 2], (double)w, e.m[4 * r + 3])));
                            inside = inside && (s >= p.vlo[r]) && (s < p.vhi[r]);
                        }
                    }
                    const float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                    a[k] = inside ? weighted_add(acc[jj * DPT + k], wt, val) : acc[jj * DPT + k];
                    fx_step(c0, inc_hi0, inc_lo0);
                    fx_step(c1, inc_hi1, inc_lo1);
                    fx_step(c2, inc_hi2, inc_lo2);
                }
#pragma unroll
                for (int k = 0; k + UNR < DPT; ++k) acc[jj * DPT + k] = acc[jj * DPT + k + UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) acc[jj * DPT + DPT - UNR + k] = a[k];
            }
        }
        __syncthreads();     // every gather of this box is done before the next one is staged
    }

    const int nseg = gridDim.x / tiles;
    const int64_t nvox = (int64_t)p.oD * ostride;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h0 + jh0 + jj * RP, w = w0 + kw;
        if (h >= p.oH || w >= p.oW) continue;
        const int64_t vox = ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
#pragma unroll
        for (int i = 0; i < DPT; ++i) {
            if (i >= nd) continue;
            if (nseg == 1) out[vox + i * ostride] = (float)acc[jj * DPT + i];
            else part[(int64_t)seg * nvox + vox + i * ostride] = acc[jj * DPT + i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

// Tile and matrix segments of a (box shape, interpolation, n) triple -- never of the matrices or the weights.  The tile is the
// extraction kernel's (extract_pick_tile: it fixes where the fixed-point stepping restarts, hence the samples' last bits).
// Segments: project_batch_shape_plan's rule on the other axis.  A box of 1024 tiles or more offers four workgroups for each of
// the chip's 256 CUs by itself and sums all n matrices in one workgroup per tile; a smaller box splits the matrices into
// consecutive segments until tiles x segments reaches about that many, never more segments than matrices.  The float64
// partial sums depend on the split, which is why it is a function of (n, box shape, interpolation) alone.
void extract_sum_shape_plan(bool cubic, const int box[3], int n, int* cfg, int* nseg, int* per_seg)
{
    *cfg = extract_pick_tile(cubic, box, nullptr);
    int T[3];
    extract_tile(*cfg, &T[0], &T[1], &T[2]);
    int64_t tiles = 1;
    for (int k = 0; k < 3; ++k) tiles *= (box[k] + T[k] - 1) / T[k];
    const int64_t want = std::max<int64_t>(1, (1024 + tiles - 1) / tiles);
    const int64_t seg = std::max<int64_t>(1, std::min<int64_t>(n, want));
    *per_seg = (int)((n + seg - 1) / seg);
    *nseg = (int)((n + *per_seg - 1) / *per_seg);
}

typedef void (*extract_sum_fn)(const float*, float*, double*, const float*, const ExtractEntry*, const double*, int, int, const AffineParams);

template <int TD, int TH, int TW>
static extract_sum_fn pick_extract_sum(int kind)
{
    switch (kind) {
        case 0: return extract_sum_tiled<0, TD, TH, TW>;
        case 1: return extract_sum_tiled<1, TD, TH, TW>;
        default: return extract_sum_tiled<2, TD, TH, TW>;
    }
}

static extract_sum_fn extract_sum_entry_point(int cfg, int kind)      // the extraction kernel's tile table (extract_tile)
{
    switch (cfg) {
        case 0: return pick_extract_sum<16, 16, 16>(kind);
        case 1: return pick_extract_sum<8, 16, 16>(kind);
        default: return pick_extract_sum<8, 8, 16>(kind);
    }
}

hipError_t init_extractsum_kernels()
{
    for (int cfg = 0; cfg < extract_tile_count(); ++cfg)
        for (int kind = 0; kind < 3; ++kind) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(extract_sum_entry_point(cfg, kind)),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// grid = box tiles x nseg workgroups; with nseg > 1 `part` holds nseg x box voxels doubles and the caller follows with
// launch_project_reduce(part, out, nseg, box voxels, 1, stream).
hipError_t launch_extract_sum(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                              const ExtractEntry* d_tab, const double* d_wts, int n, int per_seg, int nseg, const AffineParams& p,
                              int lds_bytes, hipStream_t stream)
{
    const int64_t grid = (int64_t)p.nTd * p.nTh * p.nTw * nseg;
    if (grid <= 0 || grid > 0x7fffffffLL || n <= 0 || per_seg <= 0 || (int64_t)per_seg * nseg < n || (nseg > 1 && !part))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(extract_sum_entry_point(cfg, interp_kind(interp)), dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, part, zeros16, d_tab, d_wts, n, per_seg, p);
    return hipGetLastError();
}

}  // namespace vt
