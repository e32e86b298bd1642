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
//     fixed-point stepping, hence the last bits of the samples, are extract_sum_tiled's (both kernels take these fragments and
//     weighted_add from vt_box_common.h).
//   * One float64 accumulator per owned voxel in registers, extract_sum_tiled's accumulation step, one rounding to float32 at the store.  No
//     atomics, no exchange through LDS, no segments: one workgroup per tile whatever n is, the order fixed by the list.  A list only
//     has to be a superset of the entries that pass the tile test (the test is still made), so the result does not depend on the
//     binning: with every entry listed for every tile and an output of 1024 tiles or more it is extract_sum_tiled's, bit for bit.
//   * Accumulate: the accumulators start from the output's current values, loaded once, coalesced, before the loop.  A workgroup
//     none of whose entries reaches its tile stores nothing (the output already holds b, zeroed by the caller's memset otherwise).
#include "vt_box_common.h"

#include <algorithm>

namespace vt {

// p.nTd / nTh / nTw = output tiles, p.oD / oH / oW = output shape; gridDim.x = non-empty tiles = entries of tile_ids.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void place_tiled(const float* __restrict__ src, float* __restrict__ out, const float* __restrict__ zeros16,
                                                    const ExtractEntry* __restrict__ tab, const double* __restrict__ wts,
                                                    const int* __restrict__ tile_ids, const int* __restrict__ offs,
                                                    const int* __restrict__ idx, const int accumulate, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT;
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    constexpr int UNR = CUBIC ? 2 : 4;                   // samples in flight (extract_sum_tiled's)
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int u = tile_ids[t];                           // wave-uniform: scalar loads
    const int l_first = offs[t], l_end = offs[t + 1];
    int d0, h0, w0;
    M::tile_origin(u, p, d0, h0, w0);
    const int64_t ostride = (int64_t)p.oH * p.oW;

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
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
        if (!any_valid) continue;                        // listed, but the whole tile maps outside the valid interval: nothing staged, nothing added
        touched = true;

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
                        // tiles cut by the valid interval or by the end of the output: the inside test is the canonical chain, the taps
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
VT_BOX_KERNELS(place, place_tiled<KIND, T::TD, T::TH, T::TW>)

// grid = n_tiles workgroups (the non-empty tiles; the caller launches nothing when there are none).  d_tile_ids: n_tiles tile ids
// inside p.nTd x nTh x nTw; d_offs: n_tiles + 1 ascending offsets into d_idx; d_idx: entry indices inside [0, n), ascending per tile.
hipError_t launch_place(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                        const double* d_wts, const int* d_tile_ids, const int* d_offs, const int* d_idx, int n_tiles, bool accumulate,
                        const AffineParams& p, int lds_bytes, hipStream_t stream)
{
    if (n_tiles <= 0 || (int64_t)n_tiles > (int64_t)p.nTd * p.nTh * p.nTw || !d_tile_ids || !d_offs || !d_idx) return hipErrorInvalidValue;
    hipLaunchKernelGGL(place_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)n_tiles), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, d_tile_ids, d_offs, d_idx, accumulate ? 1 : 0, p);
    return hipGetLastError();
}

}  // namespace vt
