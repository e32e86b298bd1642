// vt_kernels_projbatch.hip -- a stack of axis-0 projections in one launch (kind 12), hand-written for gfx950 (MI355X, CDNA4).
//
// image_i[h, w] = sum_d affine(M_i)[d, h, w] for n pull matrices against one resident volume: a tilt series
// (examples/projections.py:20-26 with the rotation about an axis perpendicular to the beam) without ever writing the
// transformed volumes.  The kernel is extract_tiled (vt_kernels_extract.hip) with the store replaced by a register:
//
//   * One 256-thread workgroup per (matrix, h-tile, w-tile, depth segment); ids are XCD-contiguous and matrix-major.  The
//     workgroup reads its matrix's ExtractEntry with scalar loads and marches over the TD-deep tiles of its segment.
//   * Per tile: float64 bounding box (extract_tiled's), skipped outright when it clears the valid interval; otherwise
//     stage_box, barrier, sample_box<KIND> with the Q32.32 stepping, barrier.  Tiles cut by the valid interval or by the
//     end of the depth range take the canonical float64 inside test.
//   * Every sample goes into a per-thread float64 accumulator in depth order; lane groups that split a tile's depth
//     (tiles of fewer than 256 pixels) are combined through LDS in group order.  A launch with one segment rounds to
//     float32 and stores; otherwise the workgroup stores float64 partials [matrix][segment][h][w] and project_reduce sums
//     the segments in ascending order and rounds once.  No atomics: the result is a fixed expression of (M_i, source,
//     output shape, interpolation).
//   * Entries whose box fits no LDS allocation (strong minification) gather from global memory inside the same launch
//     (direct_sample<KIND>), with the same accumulation.
#include "vt_internal.h"
#include "vt_device.h"

#include <algorithm>

namespace vt {

// p.nTd = depth segments per image, p.dch = depth tiles per segment, p.nTh / p.nTw = in-plane tiles, p.oD/oH/oW = output shape.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void project_tiled(const float* __restrict__ src, float* __restrict__ out, double* __restrict__ part,
                                                      const float* __restrict__ zeros16,
                                                      const ExtractEntry* __restrict__ tab, const AffineParams p)
{
    constexpr int NPOS = TH * TW;
    static_assert(256 % TW == 0 && (NPOS >= 256 ? NPOS % 256 == 0 : 256 % NPOS == 0), "tile/thread mapping");
    constexpr int DG = NPOS >= 256 ? 1 : 256 / NPOS;     // depth groups
    constexpr int NJ = NPOS >= 256 ? NPOS / 256 : 1;     // in-plane passes
    constexpr int RP = NPOS >= 256 ? 256 / TW : TH;      // tile rows covered per pass
    constexpr int DPT = TD / DG;                         // planes per thread and tile
    static_assert(TD % DG == 0, "tile depth / lane groups");
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
    const int tw_i = u % p.nTw;
    const int u2 = u / p.nTw;
    const int th_i = u2 % p.nTh;
    const int seg = u2 / p.nTh;
    const int h0 = th_i * TH, w0 = tw_i * TW;
    const ExtractEntry& e = tab[img];

    const int pos = DG > 1 ? tid % NPOS : tid;
    const int kw = pos % TW;
    const int jh0 = pos / TW;
    const int grp = DG > 1 ? tid / NPOS : 0;
    const int i0 = grp * DPT;

    const int tile_first = seg * p.dch;
    const int tile_end = min(tile_first + p.dch, (p.oD + TD - 1) / TD);

    double acc[NJ];
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) acc[jj] = 0.0;

    const int Lx = e.Lx, Ly = e.Ly, Lz = e.Lz;
    const int LyLx = Ly * Lx;
    const int inc_hi0 = e.inc_hi[0], inc_hi1 = e.inc_hi[1], inc_hi2 = e.inc_hi[2];
    const unsigned inc_lo0 = e.inc_lo[0], inc_lo1 = e.inc_lo[1], inc_lo2 = e.inc_lo[2];

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
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        s[r] = fma(e.m[4 * r], (double)d, fma(e.m[4 * r + 1], (double)h, fma(e.m[4 * r + 2], (double)w, e.m[4 * r + 3])));
                        inside = inside && (s[r] >= p.vlo[r]) && (s[r] < p.vhi[r]);
                    }
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

            stage_box(lds, src, zeros16, p, o, Lz, Ly, Lx, tid);
            __syncthreads();     // hipcc drains the direct-to-LDS loads (vmcnt(0)) ahead of the barrier

            double b[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) b[r] = base[r] - (double)o[r];
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
                double a = acc[jj];
                if (whole) {
#pragma unroll UNR
                    for (int i = 0; i < DPT; ++i) {
                        a += (double)sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                        fx_step(c0, inc_hi0, inc_lo0);
                        fx_step(c1, inc_hi1, inc_lo1);
                        fx_step(c2, inc_hi2, inc_lo2);
                    }
                } else {
                    // tiles cut by the valid interval or by the end of the depth range: the inside test is the canonical float64 chain
                    // (affine_direct's and the oracle's), the taps still come from the fixed-point split
                    for (int i = 0; i < nd; ++i) {
                        const int d = d0 + i0 + i;
                        bool inside = true;
#pragma unroll
                        for (int r = 0; r < 3; ++r) {
                            const double s = fma(e.m[4 * r], (double)d, fma(e.m[4 * r + 1], (double)h, fma(e.m[4 * r + 2], (double)w, e.m[4 * r + 3])));
                            inside = inside && (s >= p.vlo[r]) && (s < p.vhi[r]);
                        }
                        const float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                        a += inside ? (double)val : 0.0;
                        fx_step(c0, inc_hi0, inc_lo0);
                        fx_step(c1, inc_hi1, inc_lo1);
                        fx_step(c2, inc_hi2, inc_lo2);
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

typedef void (*project_fn)(const float*, float*, double*, const float*, const ExtractEntry*, const AffineParams);

template <int TD, int TH, int TW>
static project_fn pick_project(int kind)
{
    switch (kind) {
        case 0: return project_tiled<0, TD, TH, TW>;
        case 1: return project_tiled<1, TD, TH, TW>;
        default: return project_tiled<2, TD, TH, TW>;
    }
}

static project_fn project_entry_point(int cfg, int kind)      // the extraction kernel's tile table (extract_tile)
{
    switch (cfg) {
        case 0: return pick_project<16, 16, 16>(kind);
        case 1: return pick_project<8, 16, 16>(kind);
        default: return pick_project<8, 8, 16>(kind);
    }
}

hipError_t init_projbatch_kernels()
{
    for (int cfg = 0; cfg < extract_tile_count(); ++cfg)
        for (int kind = 0; kind < 3; ++kind) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(project_entry_point(cfg, kind)),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

hipError_t launch_project_tiled(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                                const ExtractEntry* d_tab, const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream)
{
    if (grid <= 0 || grid > 0x7fffffffLL || (p.nTd > 1 && !part)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(project_entry_point(cfg, interp_kind(interp)), dim3((unsigned)grid), dim3(256), lds_bytes, stream,
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
