// vt_kernels_projbatch.hip -- a stack of axis-0 projections in one launch (kind 12), hand-written for gfx950 (MI355X, CDNA4).
//
// image_i[h, w] = sum_d affine(M_i)[d, h, w] for n pull matrices against one resident volume: a tilt series
// (examples/projections.py:20-26 with the rotation about an axis perpendicular to the beam) without ever writing the
// transformed volumes.  The kernel is extract_tiled (vt_kernels_extract.hip) with the store replaced by a register:
//
//   * One 256-thread workgroup per (matrix, h-tile, w-tile, depth segment); ids are XCD-contiguous and matrix-major.  The
//     workgroup reads its matrix's ExtractEntry with scalar loads and marches over the TD-deep tiles of its segment.
//   * Per tile: float64 bounding box (vt_box_common.h, as every kernel of the box family), skipped outright when it clears the valid interval; otherwise
//     stage_box, barrier, sample_box<KIND> with the Q32.32 stepping, barrier.  Tiles cut by the valid interval or by the
//     end of the depth range take the canonical float64 inside test.
//   * Every sample goes into a per-thread float64 accumulator in depth order; lane groups that split a tile's depth
//     (tiles of fewer than 256 pixels) are combined through LDS in group order.  A launch with one segment rounds to
//     float32 and stores; otherwise the workgroup stores float64 partials [matrix][segment][h][w] and project_reduce sums
//     the segments in ascending order and rounds once.  No atomics: the result is a fixed expression of (M_i, source,
//     output shape, interpolation).
//   * Entries whose box fits no LDS allocation (strong minification) gather from global memory inside the same launch
//     (direct_sample<KIND>), with the same accumulation.
#include "vt_box_common.h"

#include <algorithm>

namespace vt {

// p.nTd = depth segments per image, p.dch = depth tiles per segment, p.nTh / p.nTw = in-plane tiles, p.oD/oH/oW = output shape.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void project_tiled(const float* __restrict__ src, float* __restrict__ out, double* __restrict__ part,
                                                      const float* __restrict__ zeros16,
                                                      const ExtractEntry* __restrict__ tab, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NPOS = M::NPOS, DG = M::DG, NJ = M::NJ, RP = M::RP, DPT = M::DPT;
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    constexpr int UNR = CUBIC ? 2 : 4;                   // samples in flight: four cubic ones take 400 registers (one wave per SIMD), two take 210
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int nseg = p.nTd;
    const int units = nseg * p.nTh * p.nTw;
    const int img = t / units;                           // wave-uniform: the entry is read with scalar loads
    const int u = t - img * units;
    int dseg, h0, w0;                                    // the slowest tile index counts depth segments here: dseg = seg * TD
    M::tile_origin(u, p, dseg, h0, w0);
    const int seg = dseg / TD;
    const ExtractEntry& e = tab[img];

    int kw, jh0, i0;
    const int pos = M::thread_origin(tid, kw, jh0, i0);
    const int grp = DG > 1 ? tid / NPOS : 0;

    const int tile_first = seg * p.dch;
    const int tile_end = min(tile_first + p.dch, (p.oD + TD - 1) / TD);

    double acc[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) acc[jj] = 0.0;

    const int Lx = e.Lx, Ly = e.Ly, Lz = e.Lz;
    const int LyLx = Ly * Lx;
    const FxInc3 inc = fx_inc3(e);

    if (!e.tiled) {
        // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct)
        for (int td_i = tile_first; td_i < tile_end; ++td_i) {
            const int d0 = td_i * TD;
            const int nd = min(DPT, p.oD - d0 - i0);     // planes of this tile the thread owns (<= 0: none)
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int h = h0 + jh0 + jj * RP, w = w0 + kw;
                if (h >= p.oH || w >= p.oW) continue;
#pragma unroll 1
                for (int i = 0; i < nd; ++i) {
                    const int d = d0 + i0 + i;
                    double s[3];
                    bool inside = true;
                    VT_CANONICAL_INSIDE(inside, s[r_], e, p, d, h, w);
                    if (inside) {
                        const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                        acc[jj] += (double)direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd), (float)(s[1] - fyd),
                                                               (float)(s[2] - fxd));
                    }
                }
            }
        }
    } else {
        for (int td_i = tile_first; td_i < tile_end; ++td_i) {
            const int d0 = td_i * TD;
            const int nd = min(DPT, p.oD - d0 - i0);         // planes of this tile the thread owns (<= 0: none)

            double base[3], lo[3];
            bool any_valid = true, all_valid = true;
            VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0);
            if (!any_valid) continue;                        // the whole tile maps outside the valid interval: nothing staged, nothing added

            int o[3];
            box_origin<HALO>(lo, o);

            stage_box(lds, src, zeros16, p, o, Lz, Ly, Lx, tid);
            __syncthreads();     // hipcc drains the direct-to-LDS loads (vmcnt(0)) ahead of the barrier

            double b[3];
            box_base(base, o, b);
            const bool whole = all_valid && (p.oD - d0 >= TD);   // wave-uniform

#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int j = jh0 + jj * RP;
                const int h = h0 + j, w = w0 + kw;
                if (h >= p.oH || w >= p.oW) continue;
                Fx c0, c1, c2;
                fx_start3(e, b, i0, j, kw, c0, c1, c2);
                double a = acc[jj];
                if (whole) {
#pragma unroll UNR
                    for (int i = 0; i < DPT; ++i) {
                        a += (double)sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                        fx_step3(c0, c1, c2, inc);
                    }
                } else {
                    // tiles cut by the valid interval or by the end of the depth range: the inside test is the canonical chain, the taps
                    // still come from the fixed-point split
                    for (int i = 0; i < nd; ++i) {
                        const int d = d0 + i0 + i;
                        double s;
                        bool inside = true;
                        VT_CANONICAL_INSIDE(inside, s, e, p, d, h, w);
                        const float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                        a += inside ? (double)val : 0.0;
                        fx_step3(c0, c1, c2, inc);
                    }
                }
                acc[jj] = a;
            }
            __syncthreads();     // every gather of this box is done before the next one is staged (or the groups meet below)
        }
    }

    if constexpr (DG > 1) {
        // lane groups 1 .. DG-1 hand their sums to group 0, which adds them in group order (NJ == 1 here: the launcher's
        // LDS allocation holds at least 256 doubles; every barrier above was passed by all lanes)
        double* xch = reinterpret_cast<double*>(lds);
        if (grp > 0) xch[tid] = acc[0];
        __syncthreads();
        if (grp > 0) return;
#pragma unroll
        for (int g = 1; g < DG; ++g) acc[0] += xch[g * NPOS + pos];
    }

    const int64_t plane = (int64_t)p.oH * p.oW;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h0 + jh0 + jj * RP, w = w0 + kw;
        if (h >= p.oH || w >= p.oW) continue;
        const int64_t px = (int64_t)h * p.oW + w;
        if (nseg == 1) out[(int64_t)img * plane + px] = (float)acc[jj];
        else part[((int64_t)img * nseg + seg) * plane + px] = acc[jj];
    }
}

// out[i][px] = float(part[i][0][px] + part[i][1][px] + ...): the segments in ascending order, one rounding
__global__ __launch_bounds__(256) void project_reduce(const double* __restrict__ part, float* __restrict__ out, int nseg, int64_t plane,
                                                       int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int64_t img = g / plane, px = g - img * plane;
    const double* q = part + img * nseg * plane + px;
    double s = q[0];
    for (int k = 1; k < nseg; ++k) s += q[k * plane];
    out[g] = (float)s;
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

// Tile and depth segments of an (output shape, interpolation) pair -- never of n or the matrices.  The tile is the
// extraction kernel's choice for a box of the output's shape (staged bytes per useful voxel under the typical rotation).
// Segments: a 512 x 512 image has 1024 tiles of 16 x 16, four workgroups for each of the chip's 256 CUs, and marches its
// whole depth in one workgroup; smaller images split their depth until an image alone offers about that many workgroups,
// so that n = 1 still fills the machine.  Segments are whole tiles, so the tile sequence of a pixel (where the
// fixed-point stepping restarts) does not depend on the split; the float64 partial sums do, which is why the split is a
// function of the shape alone.
void project_batch_shape_plan(bool cubic, int depth, int height, int width, int* cfg, int* nseg, int* tiles_per_seg)
{
    const int box[3] = {depth, height, width};
    *cfg = extract_pick_tile(cubic, box, nullptr);
    int T[3];
    extract_tile(*cfg, &T[0], &T[1], &T[2]);
    const int64_t ntd = (depth + T[0] - 1) / T[0];
    const int64_t inplane = (int64_t)((height + T[1] - 1) / T[1]) * ((width + T[2] - 1) / T[2]);
    const int64_t want = std::max<int64_t>(1, (1024 + inplane - 1) / inplane);
    const int64_t seg = std::min<int64_t>(ntd, want);
    *tiles_per_seg = (int)((ntd + seg - 1) / seg);
    *nseg = (int)((ntd + *tiles_per_seg - 1) / *tiles_per_seg);
}

VT_BOX_KERNELS(projbatch, project_tiled<KIND, T::TD, T::TH, T::TW>)

hipError_t launch_project_tiled(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                                const ExtractEntry* d_tab, const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream)
{
    if (grid <= 0 || grid > 0x7fffffffLL || (p.nTd > 1 && !part)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(projbatch_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, part, zeros16, d_tab, p);
    return hipGetLastError();
}

hipError_t launch_project_reduce(const double* part, float* out, int nseg, int64_t plane, int images, hipStream_t stream)
{
    const int64_t total = plane * images;
    const int64_t grid = (total + 255) / 256;
    if (grid <= 0 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(project_reduce, dim3((unsigned)grid), dim3(256), 0, stream, part, out, nseg, plane, total);
    return hipGetLastError();
}

}  // namespace vt
