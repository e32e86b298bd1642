// vt_kernels_place.hip -- n posed, weighted copies of the resident map summed into one large output (kind 17), hand-written for
// gfx950 (MI355X, CDNA4).
//
// out[v] = float32(b[v] + sum_i weights[i] * A_i[v]) with A_i the float32 volume affine_direct / extract_tiled write for matrix i at
// the output shape and b = +0, or the output's current value (accumulate): "place-back" of a small map at n poses, the inverse step
// of extract_sum_tiled (vt_kernels_extractsum.hip).  The arithmetic is that kernel's with the large map as "the box"; what differs is
// who walks which matrices.  There every tile walks all n table entries and rejects nearly all of them; here the host bins the
// entries into per-tile lists (do_place, vt_api.hip) and only the tiles with a non-empty list are launched:
//
//   * One 256-thread workgroup per NON-EMPTY output tile: blockIdx goes through xcd_contiguous to an index into the compact array
//     of tile ids, so neighbouring tiles (which share list entries and source lines) run on one XCD.
//   * The workgroup loops over its tile's list (CSR: offs[t] .. offs[t + 1] into idx[], entry indices ascending) and does per
//     listed entry exactly what extract_sum_tiled does per matrix: ExtractEntry and weight by scalar loads (the list index is one
//     more wave-uniform load), float64 tile bounding box, skip when the tile clears the valid interval, stage_box, barrier,
//     sample_box<KIND> with the Q32.32 stepping, barrier; the canonical float64 inside test on cut tiles; direct_sample<KIND> from
//     global memory for entries whose footprint fits no LDS box.  The tile is extract_pick_tile's, so the restart points of the
//     fixed-point stepping, hence the last bits of the samples, are extract_sum_tiled's.
//   * One float64 accumulator per owned voxel in registers, extract_sum_tiled's accumulation step, one rounding to float32 at the store.  No
//     atomics, no exchange through LDS, no segments: one workgroup per tile whatever n is, the order fixed by the list.  A list only
//     has to be a superset of the entries that pass the tile test (the test is still made), so the result does not depend on the
//     binning: with every entry listed for every tile and an output of 1024 tiles or more it is extract_sum_tiled's, bit for bit.
//   * Accumulate: the accumulators start from the output's current values, loaded once, coalesced, before the loop.  A workgroup
//     none of whose entries reaches its tile stores nothing (the output already holds b, zeroed by the caller's memset otherwise).
#include "vt_internal.h"
#include "vt_device.h"

#include <algorithm>

namespace vt {

// acc + w * v in float64: extract_sum_tiled's weighted_add, text and compile flags, so that both kernels assemble to the same instructions
// (the translation unit is compiled with -ffp-contract=fast)
__device__ __forceinline__ double place_weighted_add(double acc, double w, float v)
{
#pragma clang fp contract(off)
    const double t = w * (double)v;
    return acc + t;
}

// p.nTd / nTh / nTw = output tiles, p.oD / oH / oW = output shape; gridDim.x = non-empty tiles = entries of tile_ids.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void place_tiled(const float* __restrict__ src, float* __restrict__ out, const float* __restrict__ zeros16,
                                                    const ExtractEntry* __restrict__ tab, const double* __restrict__ wts,
                                                    const int* __restrict__ tile_ids, const int* __restrict__ offs,
                                                    const int* __restrict__ idx, const int accumulate, const AffineParams p)
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
    constexpr int UNR = CUBIC ? 2 : 4;                   // samples in flight (extract_sum_tiled's)
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int u = tile_ids[t];                           // wave-uniform: scalar loads
    const int l_first = offs[t], l_end = offs[t + 1];
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
    if (accumulate) {
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            const int64_t vox = ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
#pragma unroll
            for (int i = 0; i < DPT; ++i)
                if (i < nd) acc[jj * DPT + i] = (double)out[vox + i * ostride];
        }
    }

    bool touched = false;                                // workgroup-uniform: some listed entry reaches the tile
#pragma unroll 1
    for (int li = l_first; li < l_end; ++li) {
        const int mi = __builtin_amdgcn_readfirstlane(idx[li]);
        const ExtractEntry& e = tab[mi];                 // wave-uniform index: scalar loads
        const double wt = wts[mi];

        if (!e.tiled) {
            // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct).  The plane loop
            // is not unrolled (DPT cubic global gathers); the accumulators rotate by one per plane instead, DPT steps = identity.
            touched = true;
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
                            a = place_weighted_add(a, wt, direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd),
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
        if (!any_valid) continue;                        // listed, but the whole tile maps outside the valid interval: nothing staged, nothing added
        touched = true;

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
            // Every plane of the tile is sampled (the staged box covers the whole tile); planes beyond the output and voxels that fail
            // the inside test are not added.  UNR samples per trip; the accumulators rotate by UNR per trip so that they are indexed
            // statically (registers), DPT / UNR trips = identity.
            static_assert(DPT % UNR == 0, "planes per thread / unroll");
#pragma unroll 1
            for (int ib = 0; ib < DPT; ib += UNR) {
                double a[UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    bool inside = true;
                    if (!whole) {
                        // tiles cut by the valid interval or by the end of the output: the inside test is the canonical float64 chain
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
                    a[k] = inside ? place_weighted_add(acc[jj * DPT + k], wt, val) : acc[jj * DPT + k];
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

    if (!touched) return;                                // the output holds b already
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) {
        const int h = h0 + jh0 + jj * RP, w = w0 + kw;
        if (h >= p.oH || w >= p.oW) continue;
        const int64_t vox = ((int64_t)(d0 + i0) * p.oH + h) * p.oW + w;
#pragma unroll
        for (int i = 0; i < DPT; ++i) {
            if (i >= nd) continue;
            out[vox + i * ostride] = (float)acc[jj * DPT + i];
        }
    }
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
typedef void (*place_fn)(const float*, float*, const float*, const ExtractEntry*, const double*, const int*, const int*, const int*, int,
                         const AffineParams);

template <int TD, int TH, int TW>
static place_fn pick_place(int kind)
{
    switch (kind) {
        case 0: return place_tiled<0, TD, TH, TW>;
        case 1: return place_tiled<1, TD, TH, TW>;
        default: return place_tiled<2, TD, TH, TW>;
    }
}

static place_fn place_entry_point(int cfg, int kind)      // the extraction kernel's tile table (extract_tile)
{
    switch (cfg) {
        case 0: return pick_place<16, 16, 16>(kind);
        case 1: return pick_place<8, 16, 16>(kind);
        default: return pick_place<8, 8, 16>(kind);
    }
}

hipError_t init_place_kernels()
{
    for (int cfg = 0; cfg < extract_tile_count(); ++cfg)
        for (int kind = 0; kind < 3; ++kind) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(place_entry_point(cfg, kind)),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// grid = n_tiles workgroups (the non-empty tiles; the caller launches nothing when there are none).  d_tile_ids: n_tiles tile ids
// inside p.nTd x nTh x nTw; d_offs: n_tiles + 1 ascending offsets into d_idx; d_idx: entry indices inside [0, n), ascending per tile.
hipError_t launch_place(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                        const double* d_wts, const int* d_tile_ids, const int* d_offs, const int* d_idx, int n_tiles, bool accumulate,
                        const AffineParams& p, int lds_bytes, hipStream_t stream)
{
    if (n_tiles <= 0 || (int64_t)n_tiles > (int64_t)p.nTd * p.nTh * p.nTw || !d_tile_ids || !d_offs || !d_idx) return hipErrorInvalidValue;
    hipLaunchKernelGGL(place_entry_point(cfg, interp_kind(interp)), dim3((unsigned)n_tiles), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, d_tile_ids, d_offs, d_idx, accumulate ? 1 : 0, p);
    return hipGetLastError();
}

}  // namespace vt
