// vt_kernels_extractsum.hip -- weighted sum of n extracted boxes in one launch (kind 13), hand-written for gfx950 (MI355X, CDNA4).
//
// out[d, h, w] = float32(sum_i weights[i] * B_i[d, h, w]) with B_i the float32 box extract_tiled (vt_kernels_extract.hip) writes for
// matrix i: sub-tomogram averaging, or symmetrisation with the whole volume as the box, without ever writing the boxes.  The
// reference has no counterpart.  The kernel is extract_tiled with the store replaced by float64 registers, the reduction axis
// being the matrices (project_tiled, vt_kernels_projbatch.hip, reduces along the output depth instead):
//
//   * One 256-thread workgroup per (segment of consecutive matrices, box tile); ids are XCD-contiguous and segment-major, so
//     the tiles of one segment are neighbours on one XCD and walk the same matrices at about the same time.
//   * The thread mapping is the box family's (vt_box_common.h: BoxTileMap): a thread owns NJ * DPT output voxels of its tile and keeps one float64
//     accumulator for each (16 / 8 / 4 for the 16^3 / 8x16x16 / 8x8x16 tiles).  No two lanes share a voxel: no atomics, no
//     exchange through LDS.
//   * Per matrix, in ascending order: ExtractEntry and weight by scalar loads, float64 tile bounding box; a tile that clears
//     the valid interval adds nothing and stages nothing; otherwise stage_box, barrier, sample_box<KIND> with the family's
//     Q32.32 stepping (same restart points, hence the same float32 samples), barrier.  Tiles cut by the valid interval or by
//     the end of the box take the canonical float64 inside test.  Entries whose box fits no LDS allocation gather from global
//     memory (direct_sample<KIND>) inside the same loop.
//   * Every sample is widened to float64, multiplied by the float64 weight and added to its accumulator (two roundings, not a
//     fused multiply-add: the expression is the one a host loop in float64 evaluates).  A launch with one segment rounds to
//     float32 and stores; otherwise the workgroup stores float64 partials [segment][d][h][w] and project_reduce adds the
//     segments in ascending order and rounds once.
#include "vt_box_common.h"

#include <algorithm>

namespace vt {

// p.nTd / nTh / nTw = box tiles, p.oD / oH / oW = box shape; n matrices in segments of per_seg consecutive ones.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void extract_sum_tiled(const float* __restrict__ src, float* __restrict__ out, double* __restrict__ part,
                                                          const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                          const double* __restrict__ wts, const int n, const int per_seg,
                                                          const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT;
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    constexpr int UNR = CUBIC ? 2 : 4;                   // samples in flight (project_tiled's: four cubic ones take one wave per SIMD)
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tiles = p.nTd * p.nTh * p.nTw;
    const int seg = t / tiles;                           // segment-major
    int d0, h0, w0;
    M::tile_origin(t - seg * tiles, p, d0, h0, w0);
    const int64_t ostride = (int64_t)p.oH * p.oW;

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
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
                        VT_CANONICAL_INSIDE(inside, s[r_], e, p, d, h, w);
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

        double base[3], lo[3];
        bool any_valid = true, all_valid = true;
        VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0);
        if (!any_valid) continue;                        // the whole tile maps outside the valid interval: nothing staged, nothing added

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
                        // tiles cut by the valid interval or by the end of the box: the inside test is the canonical chain, the taps
                        // still come from the fixed-point split
                        const int d = d0 + i0 + ib + k;
                        double s;
                        inside = ib + k < nd;
                        VT_CANONICAL_INSIDE(inside, s, e, p, d, h, w);
                    }
                    const float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                    a[k] = inside ? weighted_add(acc[jj * DPT + k], wt, val) : acc[jj * DPT + k];
                    fx_step3(c0, c1, c2, inc);
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

VT_BOX_KERNELS(extractsum, extract_sum_tiled<KIND, T::TD, T::TH, T::TW>)

// grid = box tiles x nseg workgroups; with nseg > 1 `part` holds nseg x box voxels doubles and the caller follows with
// launch_project_reduce(part, out, nseg, box voxels, 1, stream).
hipError_t launch_extract_sum(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                              const ExtractEntry* d_tab, const double* d_wts, int n, int per_seg, int nseg, const AffineParams& p,
                              int lds_bytes, hipStream_t stream)
{
    const int64_t grid = (int64_t)p.nTd * p.nTh * p.nTw * nseg;
    if (grid <= 0 || grid > 0x7fffffffLL || n <= 0 || per_seg <= 0 || (int64_t)per_seg * nseg < n || (nseg > 1 && !part))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(extractsum_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, part, zeros16, d_tab, d_wts, n, per_seg, p);
    return hipGetLastError();
}

}  // namespace vt
