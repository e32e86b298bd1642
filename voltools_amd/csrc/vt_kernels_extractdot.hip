// vt_kernels_extractdot.hip -- per-box template scores of n extracted boxes in one launch (kind 14), hand-written for gfx950 (MI355X, CDNA4).
//
// out[i] = (sum_v mask[v] * B_i[v], sum_v mask[v] * B_i[v]^2, sum_v tmpl[v] * B_i[v]) in float64, with B_i the float32 box extract_tiled
// (vt_kernels_extract.hip) writes for matrix i: the three sums a locally normalised cross-correlation of n candidate (position,
// orientation) pairs with one template needs, without ever writing the boxes.  The reference has no counterpart.  The kernel is
// extract_tiled with the store replaced by three float64 accumulators per thread, the reduction running over the voxels of a box
// (extract_sum_tiled, vt_kernels_extractsum.hip, reduces across the boxes instead):
//
//   * One 256-thread workgroup per (matrix, box tile) pair; ids are XCD-contiguous and box-major, the tile is extract_pick_tile's and
//     the Q32.32 stepping restarts where extract_tiled's does, so every sample is extract_tiled's bit for bit (one text, vt_box_common.h).
//   * A tile that maps wholly outside the valid interval stages nothing and writes a zero partial; tiles cut by the valid interval or
//     by the end of the box take the canonical float64 inside test; entries whose box fits no LDS allocation gather from global memory
//     (direct_sample<KIND>) in the same launch.
//   * tmpl[v] and mask[v] are read from global memory by the thread that owns voxel v (coalesced along w; both arrays are box-sized
//     and stay in L2).  mask == nullptr stands for a mask of ones.
//   * Each sample is widened to float64; mask * b and tmpl * b are exact (two float32 factors), (mask * b) * b is rounded once, every
//     addition is rounded; no product is contracted into an addition.  A thread adds its voxels in the order (in-plane pass, plane); the 256 partial triples are
//     reduced by a tree of fixed shape (within a wave by lane offsets 32, 16, .. 1, then (w0 + w1) + (w2 + w3)); the tiles of a box
//     are added in ascending tile index by extract_dot_reduce.  No atomics: out[i] is a fixed expression of its own entry.
//   * The cross-wave step overlays the first 96 bytes of the staged box once every gather is done: the launch allocates no LDS beyond
//     extract_tiled's (at least 96 bytes).
#include "vt_box_common.h"

#include <algorithm>

namespace vt {

// The three sums' terms for one sample, with every rounding the contract names: every product goes through rounded() (vt_box_common.h).
// mask * b and tmpl * b are exact either way (24 + 24 significant bits); (mask * b) * b is the one product whose rounding shows.
__device__ __forceinline__ void dot_add(double& s0, double& s1, double& s2, float mk, float tp, float v)
{
    const double b = (double)v;
    const double mb = rounded((double)mk * b);       // exact
    const double tb = rounded((double)tp * b);       // exact
    const double mbb = rounded(mb * b);              // rounded once
    s0 = s0 + mb;
    s1 = s1 + mbb;
    s2 = s2 + tb;
}

// p.nTd / nTh / nTw = box tiles, p.oD / oH / oW = box shape; part holds [box][tile][3] doubles of this launch.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW>
__global__ __launch_bounds__(256) void extract_dot_tiled(const float* __restrict__ src, double* __restrict__ part,
                                                          const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                          const float* __restrict__ tmpl, const float* __restrict__ mask,
                                                          const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT;
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    constexpr int UNR = CUBIC ? 1 : 4;                   // samples in flight: two cubic ones cost 250 VGPRs, four over 450
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    const int t = xcd_contiguous(blockIdx.x, gridDim.x);
    const int tiles = p.nTd * p.nTh * p.nTw;
    const int box = t / tiles;                           // wave-uniform: the entry is read with scalar loads
    int d0, h0, w0;
    M::tile_origin(t - box * tiles, p, d0, h0, w0);
    const ExtractEntry& e = tab[box];
    const int ostride = p.oH * p.oW;                     // the box has fewer than 2^31 voxels (checked on the host): 32-bit voxel offsets
    const bool has_mask = mask != nullptr;               // uniform

    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int nd = min(DPT, p.oD - d0 - i0);             // planes this thread owns (<= 0: none)

    double s0 = 0.0, s1 = 0.0, s2 = 0.0;

    if (!e.tiled) {
        // footprint beyond the LDS cap: taps from global memory, coordinates by the canonical chain (affine_direct)
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            const int vox = ((d0 + i0) * p.oH + h) * p.oW + w;
            for (int i = 0; i < nd; ++i) {
                const int d = d0 + i0 + i;
                double s[3];
                bool inside = true;
                VT_CANONICAL_INSIDE(inside, s[r_], e, p, d, h, w);
                if (inside) {
                    const double fzd = floor(s[0]), fyd = floor(s[1]), fxd = floor(s[2]);
                    const float val = direct_sample<KIND>(src, p, (int)fzd, (int)fyd, (int)fxd, (float)(s[0] - fzd), (float)(s[1] - fyd), (float)(s[2] - fxd));
                    dot_add(s0, s1, s2, has_mask ? mask[vox + i * ostride] : 1.0f, tmpl[vox + i * ostride], val);
                }
            }
        }
    } else {
        double base[3], lo[3];
        bool any_valid = true, all_valid = true;
        VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0);

        if (any_valid) {                                 // else the whole tile maps outside the valid interval: nothing staged, a zero partial
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
                const int vox = ((d0 + i0) * p.oH + h) * p.oW + w;
                if (whole) {
#pragma unroll UNR
                    for (int i = 0; i < DPT; ++i) {
                        const float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                        dot_add(s0, s1, s2, has_mask ? mask[vox + i * ostride] : 1.0f, tmpl[vox + i * ostride], val);
                        fx_step3(c0, c1, c2, inc);
                    }
                } else {
                    // tiles cut by the valid interval or by the end of the box: the inside test is the canonical chain, the taps still
                    // come from the fixed-point split
                    for (int i = 0; i < nd; ++i) {
                        float val = sample_box<KIND>(lds, Lx, LyLx, c0.hi, c1.hi, c2.hi, fx_frac(c0), fx_frac(c1), fx_frac(c2));
                        int d = d0 + i0 + i;
                        // the float64 chain starts once the sample is complete: scheduled among the cubic taps it costs 40 VGPRs
                        asm volatile("" : "+v"(d), "+v"(val));
                        double s;
                        bool inside = true;
                        VT_CANONICAL_INSIDE(inside, s, e, p, d, h, w);
                        if (inside) dot_add(s0, s1, s2, has_mask ? mask[vox + i * ostride] : 1.0f, tmpl[vox + i * ostride], val);
                        fx_step3(c0, c1, c2, inc);
                    }
                }
            }
        }
    }

    // ---- 256 partial triples -> one, by a tree of fixed shape ----
    s0 = wave_tree_sum(s0);
    s1 = wave_tree_sum(s1);
    s2 = wave_tree_sum(s2);
    __syncthreads();             // every gather of the staged box is done: its first 96 bytes become the cross-wave scratch
    double* red = reinterpret_cast<double*>(lds);
    if ((tid & 63) == 0) {
        const int wv = tid >> 6;
        red[3 * wv] = s0; red[3 * wv + 1] = s1; red[3 * wv + 2] = s2;
    }
    __syncthreads();
    if (tid < 3) part[(int64_t)t * 3 + tid] = (red[tid] + red[3 + tid]) + (red[6 + tid] + red[9 + tid]);
}

// out[i][k] = part[i][0][k] + part[i][1][k] + ... in ascending tile index; one thread per (box, sum)
__global__ __launch_bounds__(256) void extract_dot_reduce(const double* __restrict__ part, double* __restrict__ out, const int tiles, const int64_t n3)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= n3) return;
    const int64_t i = g / 3;
    const int k = (int)(g - i * 3);
    const double* q = part + i * tiles * 3 + k;
    double acc = 0.0;
    for (int u = 0; u < tiles; ++u) acc = acc + q[(int64_t)u * 3];
    out[g] = acc;
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------

VT_BOX_KERNELS(extractdot, extract_dot_tiled<KIND, T::TD, T::TH, T::TW>)

int extract_dot_min_lds() { return 4 * 3 * (int)sizeof(double); }

// grid = box tiles x cnt workgroups, then one thread per output number; `part` holds cnt x tiles x 3 doubles, `out` cnt x 3.
hipError_t launch_extract_dot(int cfg, int interp, const float* src, double* out, double* part, const float* zeros16,
                              const ExtractEntry* d_tab, const float* d_tmpl, const float* d_mask, int cnt, const AffineParams& p,
                              int lds_bytes, hipStream_t stream)
{
    const int64_t tiles = (int64_t)p.nTd * p.nTh * p.nTw;
    const int64_t grid = tiles * cnt;
    if (cnt <= 0 || tiles <= 0 || grid > 0x7fffffffLL || !part || !out || !d_tmpl || lds_bytes < extract_dot_min_lds() || lds_bytes > 160 * 1024)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(extractdot_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, part, zeros16, d_tab, d_tmpl, d_mask, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int64_t n3 = (int64_t)cnt * 3;
    hipLaunchKernelGGL(extract_dot_reduce, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, stream, part, out, (int)tiles, n3);
    return hipGetLastError();
}

}  // namespace vt
