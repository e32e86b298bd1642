// vt_kernels_extract.hip -- batched box extraction (kind 11), hand-written for gfx950 (MI355X, CDNA4).
//
// n small boxes cut out of one large resident volume, each with its own pull matrix, in ONE launch: sub-tomogram
// extraction, particle re-extraction, local template-matching windows.  The reference has no counterpart beyond scipy's
// `output_shape` argument at its CPU call site (transforms.py:136-150).
//
//   * One 256-thread workgroup per (matrix, box tile) pair.  The host uploads one table entry per matrix (ExtractEntry:
//     the folded 3x4 matrix, the tile reach, the Q32.32 depth steps, the staged box dims); the workgroup reads its entry
//     with scalar loads, so everything per-matrix lives in SGPRs exactly as the kernarg block does for affine_tiled.
//   * Thread mapping, float64 tile bounding box, staged-box origin, canonical float64 inside test (tiles cut by the valid
//     interval or by the end of the box) and Q32.32 stepping are the box family's, written once in vt_box_common.h for
//     kinds 11-19.  Staging and gather are affine_tiled's: stage_box (16-byte direct-to-LDS loads, zero vector outside
//     the volume), sample_box<KIND> (same weights, same association).
//   * Box i is a function of its own entry only.  The tile shape -- it fixes where the fixed-point stepping restarts,
//     hence last bits -- comes from (box shape, interpolation); whether an entry stages into LDS or gathers from global
//     memory comes from its own footprint against a fixed cap.  Nothing depends on the batch: the LDS strides are per
//     entry, only the size of the launch's LDS allocation is a batch-wide maximum (speed, not arithmetic).
//   * Entries whose footprint fits no LDS box (strong minification) gather their taps from global memory inside the
//     same launch, with the arithmetic of affine_direct: same output order, no second launch.
//   * Workgroup ids are XCD-contiguous and box-major: the tiles of one box are neighbours on one XCD, so the halves
//     of the staged boxes that adjacent tiles of a rotated box share can hit that XCD's L2.
#include "vt_box_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vt {

template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void extract_tiled(const float* __restrict__ src, float* __restrict__ out,
                                                      const float* __restrict__ zeros16,
                                                      const ExtractEntry* __restrict__ tab, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT;
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
    const int64_t ostride = (int64_t)p.oH * p.oW;
    out += (int64_t)box * p.oD * ostride;

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int nd = min(DPT, p.oD - d0 - i0);             // planes this thread owns (<= 0: none)

    if (!e.tiled) {
        // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            float* optr = out + ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
            for (int i = 0; i < nd; ++i) {
                const int d = d0 + i0 + i;
                double s[3];
                bool inside = true;
                VT_CANONICAL_INSIDE(inside, s[r_], e, p, d, h, w);
                float val = 0.0f;
                if (inside) {
                    const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                    val = direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd), (float)(s[1] - fyd), (float)(s[2] - fxd));
                }
                optr[i * ostride] = val;
            }
        }
        return;
    }

    double base[3], lo[3];
    bool any_valid = true, all_valid = true;
    VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0);

    if (!any_valid) {
        // the whole tile maps outside the valid interval
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h < p.oH && w < p.oW) {
                float* optr = out + ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
                for (int i = 0; i < nd; ++i, optr += ostride) *optr = 0.0f;
            }
        }
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
        float* optr = out + ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
        if (whole) {
#pragma unroll 4
            for (int i = 0; i < DPT; ++i) {
                optr[i * ostride] = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                fx_step3(c0, c1, c2, inc);
            }
        } else {
            // tiles cut by the valid interval or by the end of the box: the inside test is the canonical chain, the taps still come
            // from the fixed-point split
            for (int i = 0; i < nd; ++i) {
                const int d = d0 + i0 + i;
                double s;
                bool inside = true;
                VT_CANONICAL_INSIDE(inside, s, e, p, d, h, w);
                const float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                optr[i * ostride] = inside ? val : 0.0f;
                fx_step3(c0, c1, c2, inc);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side: tile table, per-entry planning, launcher
// ---------------------------------------------------------------------------------------------------
int extract_tile_count() { return kExtractTileCount; }
void extract_tile(int idx, int* td, int* th, int* tw) { *td = kExtractTiles[idx].td; *th = kExtractTiles[idx].th; *tw = kExtractTiles[idx].tw; }

// Staged box of tile T under matrix m (pick_box_tile's formula): false when the extent is absurd.
static bool extract_box_dims(const double m[12], const int T[3], int halo2, int L[3])
{
    for (int r = 0; r < 3; ++r) {
        double ext = 0;
        for (int k = 0; k < 3; ++k) ext += std::fabs(m[4 * r + k]) * (T[k] - 1);
        if (!(ext < 4096.0)) return false;
        // floor(hi + drift) - floor(lo - kBoxMargin) <= floor(ext + 2 kBoxMargin) + 1 origin indices, + 1 for the count, + 1 upper tap
        L[r] = (int)std::floor(ext + 2.0 * kBoxMargin) + 3 + halo2;
    }
    L[2] = (L[2] + 3 + 3) & ~3;                              // origin aligned down by up to 3, stride multiple of 4
    return true;
}

// The tile of a (box shape, interpolation) pair -- never of the matrices: staged bytes per USEFUL output voxel (tiles that
// hang over the end of the box count in full) for the typical rotation, |m[r][k]| = 1/2 (the mean magnitude of an entry of
// a uniformly drawn rotation), with pick_box_tile's penalty where fewer than three workgroups fit a CU's LDS.
int extract_pick_tile(bool cubic, const int box[3], int* wg_per_cu)
{
    const double typical[12] = {0.5, 0.5, 0.5, 0, 0.5, 0.5, 0.5, 0, 0.5, 0.5, 0.5, 0};
    int best = 0, best_wg = 1;
    double best_cost = 1e300;
    for (int cfg = 0; cfg < extract_tile_count(); ++cfg) {
        const int T[3] = {kExtractTiles[cfg].td, kExtractTiles[cfg].th, kExtractTiles[cfg].tw};
        int L[3];
        if (!extract_box_dims(typical, T, cubic ? 2 : 0, L)) continue;
        const int64_t bytes = (int64_t)L[0] * L[1] * L[2] * 4;
        const int wg = (int)std::min<int64_t>(8, (160 * 1024) / bytes);
        double tiles = 1;
        for (int k = 0; k < 3; ++k) tiles *= (double)((box[k] + T[k] - 1) / T[k]);
        const double useful = (double)box[0] * box[1] * box[2];
        const double cost = (double)bytes * tiles / useful * (wg >= 3 ? 1.0 : (wg == 2 ? 1.25 : 2.0));
        if (cost < best_cost) { best_cost = cost; best = cfg; best_wg = wg; }
    }
    if (wg_per_cu) *wg_per_cu = best_wg;
    return best;
}

// One table entry from the folded matrix.  `tiled` iff this matrix's own box fits lds_cap (and force_direct is off).
void extract_fill_entry(const double m[12], int cfg, bool cubic, int lds_cap, bool force_direct, ExtractEntry* e)
{
    const int T[3] = {kExtractTiles[cfg].td, kExtractTiles[cfg].th, kExtractTiles[cfg].tw};
    std::memset(e, 0, sizeof(*e));
    std::memcpy(e->m, m, sizeof(double) * 12);
    for (int r = 0; r < 3; ++r) {
        double neg = 0, pos = 0;                             // set_tile_reach
        for (int k = 0; k < 3; ++k) {
            const double x = m[4 * r + k] * (T[k] - 1);
            if (x < 0) neg += x; else pos += x;
        }
        e->neg[r] = neg; e->pos[r] = pos;
        const double step = m[4 * r];                        // Q32.32 split of the depth step (plan_prepare)
        const double fl = std::floor(step);
        e->inc_hi[r] = (std::fabs(step) < 2.0e9) ? (int32_t)fl : 0;
        e->inc_lo[r] = (uint32_t)std::min(4294967295.0, std::floor((step - fl) * 4294967296.0 + 0.5));
        if ((step - fl) * 4294967296.0 + 0.5 >= 4294967296.0) { e->inc_lo[r] = 0; e->inc_hi[r] += 1; }
    }
    int L[3];
    if (!force_direct && extract_box_dims(m, T, cubic ? 2 : 0, L) && (int64_t)L[0] * L[1] * L[2] * 4 <= lds_cap) {
        e->Lz = L[0]; e->Ly = L[1]; e->Lx = L[2];
        e->tiled = 1;
    }
}

VT_BOX_KERNELS(extract, extract_tiled<KIND, T::TD, T::TH, T::TW>)

hipError_t launch_extract(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                          const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream)
{
    if (grid <= 0 || grid > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(extract_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, p);
    return hipGetLastError();
}

}  // namespace vt
