// vt_backproject_common.h -- the back-projection kernel, one text for its two forms: backproject_tiled<.., false> (kind 18, one volume,
// instantiated in vt_kernels_backproject.hip, which describes the kernel) and backproject_tiled<.., true> (kind 19, nb boxes of one
// shape in one launch, instantiated in vt_kernels_backprojectboxes.hip).
//
// BOXES gives the body a box index and nothing else: the workgroup finds its box b and its tile within the box, moves tab, wts and out
// to that box's entries, weights and voxels, and runs the body kind 18 runs.  Every instruction that forms a value is the same text
// compiled with the same flags, which is what makes a box of kind 19 the bits of kind 18's volume for that box's matrices.  The body is
// kept inside the __global__ function: moved into a __device__ function called from two kernels, the same text took up to 29 more
// VGPRs in kind 18's instantiations.
//
// Thread mapping, tile decode and weighted_add are the box family's (vt_box_common.h).  The geometry is not: patch_geo works on rows 1
// and 2 only and returns before anything else is formed when the tile misses the image; the family's three-row form would add a row
// this kernel never reads.
#pragma once
#include "vt_box_common.h"

namespace vt {

// wave-uniform geometry of one entry on one tile: rows 1 and 2 only
struct PatchGeo {
    double base1, base2;       // image coordinate of the tile's first voxel
    int o1, o2;                // integer origin of the staged patch (o2 a multiple of 4)
    bool all_valid;            // the whole tile clears the skirt: no per-voxel test
};

// false: the tile maps outside the valid interval of the image (nothing staged, nothing added)
template <int HALO>
__device__ __forceinline__ bool patch_geo(const ExtractEntry& e, const AffineParams& p, int d0, int h0, int w0, PatchGeo& g)
{
    const double b1 = fma(e.m[4], (double)d0, fma(e.m[5], (double)h0, fma(e.m[6], (double)w0, e.m[7])));
    const double b2 = fma(e.m[8], (double)d0, fma(e.m[9], (double)h0, fma(e.m[10], (double)w0, e.m[11])));
    const double lo1 = b1 + e.neg[1], hi1 = b1 + e.pos[1];
    const double lo2 = b2 + e.neg[2], hi2 = b2 + e.pos[2];
    const bool any_valid = (hi1 >= p.vlo[1] - kTileMargin) && (lo1 < p.vhi[1] + kTileMargin) && (hi2 >= p.vlo[2] - kTileMargin) &&
                           (lo2 < p.vhi[2] + kTileMargin);
    if (!any_valid) return false;
    g.base1 = b1; g.base2 = b2;
    g.all_valid = (lo1 >= p.vlo[1] + kTileMargin) && (hi1 < p.vhi[1] - kTileMargin) && (lo2 >= p.vlo[2] + kTileMargin) &&
                  (hi2 < p.vhi[2] - kTileMargin);
    // finite and small: the tile meets the valid interval, its extent was bounded on the host (vt_device.h: kBoxMargin)
    g.o1 = (int)floor(lo1 - kBoxMargin) - HALO;
    g.o2 = ((int)floor(lo2 - kBoxMargin) - HALO) & ~3;
    return true;
}

// first entry at or after j that stages a patch and reaches the tile; n when there is none
template <int HALO>
__device__ __forceinline__ int next_staged(const ExtractEntry* __restrict__ tab, int n, int j, const AffineParams& p, int d0, int h0, int w0,
                                           PatchGeo& g)
{
    for (; j < n; ++j) {
        const ExtractEntry& e = tab[j];
        if (e.tiled && patch_geo<HALO>(e, p, d0, h0, w0, g)) break;
    }
    return j;
}

// stage_box in two dimensions: the patch [o1, o1 + Ly) x [o2, o2 + Lx) of one image, lane-linear (16-byte vector v lands at buf + 16 v)
__device__ __forceinline__ void stage_patch(float* buf, const float* __restrict__ img, const float* __restrict__ zeros16,
                                            const AffineParams& p, int o1, int o2, int Ly, int Lx, int tid)
{
    const int nvx = Lx >> 2;
    const int total = Ly * nvx;
    const int step_y = 256 / nvx, step_cx = 256 - step_y * nvx;
    int v = tid;
    int y = v / nvx;
    int cx = v - y * nvx;
    const int wave_first = __builtin_amdgcn_readfirstlane(tid & ~63);
    for (int vb = wave_first; vb < total; vb += 256, v += 256) {
        const int gy = o1 + y, gx = o2 + 4 * cx;
        const bool inb = (unsigned)gy < (unsigned)p.sH && (unsigned)gx < (unsigned)p.sP;
        const float* g = inb ? img + ((int64_t)gy * p.sP + gx) : zeros16;
        if (v < total)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                             (__attribute__((address_space(3))) void*)(buf + 4 * vb), 16, 0, 0);
        cx += step_cx; y += step_y;
        if (cx >= nvx) { cx -= nvx; y += 1; }
    }
}

// cubic_gather_b64 cut down to one plane: the four x taps [ix-1, ix+2] of each of the four rows as three 8-byte-aligned ds_read_b64, summed
// per column with the row weights, the x weights meet the four columns of the stencil at the end (selected by the parity, so the one or
// two extra columns of the aligned window never enter the result).  ra: LDS byte address of column e = (ix - 1) & ~1 of tap row 0.
__device__ __forceinline__ float cubic_gather2_b64(unsigned ra, unsigned row_b, int par, const float (&wx)[4], const float (&wy)[4])
{
    const unsigned off3 = par ? 16u : 8u;                          // bytes: third pair, or the second one again
    v2f r[12];
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
        const unsigned a = ra + (unsigned)bb * row_b;
        asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %3 offset:8\n\tds_read_b64 %2, %4"
                     : "=&v"(r[3 * bb]), "=&v"(r[3 * bb + 1]), "=&v"(r[3 * bb + 2]) : "v"(a), "v"(a + off3));
    }
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]), "+v"(r[6]),
                 "+v"(r[7]), "+v"(r[8]), "+v"(r[9]), "+v"(r[10]), "+v"(r[11]));
    v2f S0 = {0.f, 0.f}, S1 = {0.f, 0.f}, S2 = {0.f, 0.f};
#pragma unroll
    for (int bb = 0; bb < 4; ++bb) {
        S0 = __builtin_elementwise_fma(r[3 * bb], (v2f)(wy[bb]), S0);
        S1 = __builtin_elementwise_fma(r[3 * bb + 1], (v2f)(wy[bb]), S1);
        S2 = __builtin_elementwise_fma(r[3 * bb + 2], (v2f)(wy[bb]), S2);     // par = 0: the second pair again, never selected below
    }
    const float t0 = par ? S0.y : S0.x, t1 = par ? S1.x : S0.y, t2 = par ? S1.y : S1.x, t3 = par ? S2.x : S1.y;
    return fmaf(wx[3], t3, fmaf(wx[2], t2, fmaf(wx[1], t1, wx[0] * t0)));
}

// One value from the staged patch.  (iy, ix) = integer tap origin in patch coordinates, fy / fx = fractions.
template <int KIND>
__device__ __forceinline__ float sample_patch(const float* __restrict__ buf, int Lx, int iy, int ix, float fy, float fx)
{
    if constexpr (KIND == 0) {
        const float* q = buf + (__mul24(iy, Lx) + ix);
        const float a00 = q[0], a01 = q[1];
        const float a10 = q[Lx], a11 = q[Lx + 1];
        const float x0 = fmaf(fx, a01 - a00, a00);
        const float x1 = fmaf(fx, a11 - a10, a10);
        return fmaf(fy, x1 - x0, x0);
    } else {
        float wx[4], wy[4];
        cubic_weights<KIND == 2>(fx, wx);
        cubic_weights<KIND == 2>(fy, wy);
        const int x1 = ix - 1, par = x1 & 1, e = x1 - par;
        return cubic_gather2_b64(lds_byte_address(buf + (__mul24(iy - 1, Lx) + e)), 4u * (unsigned)Lx, par, wx, wy);
    }
}

__device__ __forceinline__ float fetch0_2d(const float* __restrict__ img, const AffineParams& p, int y, int x)
{
    if ((unsigned)y < (unsigned)p.sH && (unsigned)x < (unsigned)p.sW) return img[(int64_t)y * p.sP + x];
    return 0.0f;
}

// One value at integer tap origin (iy, ix) and fractions (fy, fx), taps from global memory: direct_sample in two dimensions.
template <int KIND>
__device__ __forceinline__ float direct_sample_2d(const float* __restrict__ img, const AffineParams& p, int iy, int ix, float fy, float fx)
{
    if constexpr (KIND == 0) {
        const float a00 = fetch0_2d(img, p, iy, ix), a01 = fetch0_2d(img, p, iy, ix + 1);
        const float a10 = fetch0_2d(img, p, iy + 1, ix), a11 = fetch0_2d(img, p, iy + 1, ix + 1);
        const float x0 = fmaf(fx, a01 - a00, a00);
        const float x1 = fmaf(fx, a11 - a10, a10);
        return fmaf(fy, x1 - x0, x0);
    } else {
        float wx[4], wy[4];
        cubic_weights<KIND == 2>(fx, wx);
        cubic_weights<KIND == 2>(fy, wy);
        float val = 0.f;
        for (int bb = 0; bb < 4; ++bb) {
            float accx = wx[0] * fetch0_2d(img, p, iy - 1 + bb, ix - 1);
            accx = fmaf(wx[1], fetch0_2d(img, p, iy - 1 + bb, ix), accx);
            accx = fmaf(wx[2], fetch0_2d(img, p, iy - 1 + bb, ix + 1), accx);
            accx = fmaf(wx[3], fetch0_2d(img, p, iy - 1 + bb, ix + 2), accx);
            val = fmaf(wy[bb], accx, val);
        }
        return val;
    }
}

// p.nTd / nTh / nTw = output tiles (BOXES: of one box), p.oD / oH / oW = output shape (BOXES: box shape), p.sD = images in the stack;
// gridDim.x = output tiles (BOXES: nb x tiles, box-major).  buf_floats: floats per LDS buffer (two are allocated), a multiple of 4 that
// holds the largest staged patch (BOXES: of the whole batch; which entries stage was decided per entry on the host).
// BOXES: tab = nb x n entries, wts = nb x n weights, out = nb boxes, each box-major; `tiles` = p.nTd * p.nTh * p.nTw (not read otherwise).
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TD, int TH, int TW, bool BOXES>
__global__ __launch_bounds__(256) void backproject_tiled(const float* __restrict__ src, float* __restrict__ out,
                                                          const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                          const double* __restrict__ wts, const int n, const int buf_floats,
                                                          const int accumulate, const int tiles, const AffineParams p)
{
    using M = BoxTileMap<TD, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP, DPT = M::DPT;
    constexpr bool CUBIC = KIND != 0;
    constexpr int HALO = CUBIC ? 1 : 0;
    constexpr int UNR = CUBIC ? 2 : 4;                   // samples in flight (place_tiled's)
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    int u = xcd_contiguous(blockIdx.x, gridDim.x);
    if constexpr (BOXES) {
        // box-major grid: consecutive u, which xcd_contiguous keeps on one XCD, are the tiles of one box, whose image patches overlap.
        // 64-bit offsets: nb x n and nb x box voxels pass 2^31 long before one box does.
        const int b = u / tiles;                         // workgroup-uniform
        u -= b * tiles;
        tab += (int64_t)b * n;
        wts += (int64_t)b * n;
        out += (int64_t)b * ((int64_t)p.oD * p.oH * p.oW);
    }
    int d0, h0, w0;
    M::tile_origin(u, p, d0, h0, w0);
    const int64_t ostride = (int64_t)p.oH * p.oW;
    const int64_t istride = (int64_t)p.sH * p.sP;        // floats between the images of the stack

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

    // prologue: the first entry that stages a patch for this tile goes into buffer 0
    PatchGeo g;
    int cur = next_staged<HALO>(tab, n, 0, p, d0, h0, w0, g);
    if (cur < n) {
        const ExtractEntry& e = tab[cur];
        stage_patch(lds, src + (int64_t)(int)e.m[3] * istride, zeros16, p, g.o1, g.o2, e.Ly, e.Lx, tid);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the LDS-DMA has landed (and accumulate's pre-load) ...
    __syncthreads();                                     // ... in every wave

    bool touched = cur < n;                              // workgroup-uniform: some entry reaches the tile
    int cur_buf = 0;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const ExtractEntry& e = tab[i];                  // wave-uniform index: scalar loads
        const double wt = wts[i];
        const float* img = src + (int64_t)(int)e.m[3] * istride;

        if (!e.tiled) {
            // patch beyond the LDS buffers: taps from global memory, coordinates by the canonical chain.  No DMA is in flight here.  The
            // plane loop is not unrolled; the accumulators rotate by one per plane instead, DPT steps = identity (place_tiled's).
            PatchGeo gd;
            if (!patch_geo<HALO>(e, p, d0, h0, w0, gd)) continue;
            touched = true;
#pragma unroll
            for (int jj = 0; jj < NJ; ++jj) {
                const int h = h0 + jh0 + jj * RP, w = w0 + kw;
                if (h >= p.oH || w >= p.oW) continue;
#pragma unroll 1
                for (int k = 0; k < DPT; ++k) {
                    double a = acc[jj * DPT];
                    if (k < nd) {
                        const int d = d0 + i0 + k;
                        const double s1 = fma(e.m[4], (double)d, fma(e.m[5], (double)h, fma(e.m[6], (double)w, e.m[7])));
                        const double s2 = fma(e.m[8], (double)d, fma(e.m[9], (double)h, fma(e.m[10], (double)w, e.m[11])));
                        if ((s1 >= p.vlo[1]) && (s1 < p.vhi[1]) && (s2 >= p.vlo[2]) && (s2 < p.vhi[2])) {
                            const double fyd = floor(s1), fxd = floor(s2);
                            a = weighted_add(a, wt, direct_sample_2d<KIND>(img, p, (int)fyd, (int)fxd, (float)(s1 - fyd),
                                                                                       (float)(s2 - fxd)));
                        }
                    }
#pragma unroll
                    for (int q = 0; q + 1 < DPT; ++q) acc[jj * DPT + q] = acc[jj * DPT + q + 1];
                    acc[jj * DPT + DPT - 1] = a;
                }
            }
            continue;
        }
        if (i != cur) continue;                          // the tile maps outside this image's valid interval

        // the next entry's patch sets off into the other buffer: its last reader passed the barrier that ended the previous staged entry
        PatchGeo gn;
        const int nxt = next_staged<HALO>(tab, n, i + 1, p, d0, h0, w0, gn);
        if (nxt < n) {
            const ExtractEntry& en = tab[nxt];
            stage_patch(lds + (cur_buf ^ 1) * buf_floats, src + (int64_t)(int)en.m[3] * istride, zeros16, p, gn.o1, gn.o2, en.Ly, en.Lx, tid);
        }

        // ---- entry i from its own buffer: LDS reads only ----
        const float* buf = lds + cur_buf * buf_floats;
        const int Lx = e.Lx;
        const double b1 = g.base1 - (double)g.o1, b2 = g.base2 - (double)g.o2;
        const int inc_hi1 = e.inc_hi[1], inc_hi2 = e.inc_hi[2];
        const unsigned inc_lo1 = e.inc_lo[1], inc_lo2 = e.inc_lo[2];
        const bool whole = g.all_valid && (p.oD - d0 >= TD);   // wave-uniform

#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int j = jh0 + jj * RP;
            const int h = h0 + j, w = w0 + kw;
            if (h >= p.oH || w >= p.oW) continue;
            const double s1 = fma(e.m[4], (double)i0, fma(e.m[5], (double)j, fma(e.m[6], (double)kw, b1)));
            const double s2 = fma(e.m[8], (double)i0, fma(e.m[9], (double)j, fma(e.m[10], (double)kw, b2)));
            Fx c1 = to_fx(s1), c2 = to_fx(s2);
            // Every plane of the tile is sampled (the staged patch covers the whole tile); planes beyond the output and voxels that fail
            // the inside test are not added.  UNR samples per trip, the accumulators rotate by UNR per trip (place_tiled's).
            static_assert(DPT % UNR == 0, "planes per thread / unroll");
#pragma unroll 1
            for (int ib = 0; ib < DPT; ib += UNR) {
                double a[UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    bool inside = true;
                    if (!whole) {
                        // tiles cut by the valid interval or by the end of the output: the inside test is the canonical float64 chain,
                        // the taps still come from the fixed-point split
                        const int d = d0 + i0 + ib + k;
                        const double t1 = fma(e.m[4], (double)d, fma(e.m[5], (double)h, fma(e.m[6], (double)w, e.m[7])));
                        const double t2 = fma(e.m[8], (double)d, fma(e.m[9], (double)h, fma(e.m[10], (double)w, e.m[11])));
                        inside = (ib + k < nd) && (t1 >= p.vlo[1]) && (t1 < p.vhi[1]) && (t2 >= p.vlo[2]) && (t2 < p.vhi[2]);
                    }
                    const float val = sample_patch<KIND>(buf, Lx, c1.hi, c2.hi, fx_frac(c1), fx_frac(c2));
                    a[k] = inside ? weighted_add(acc[jj * DPT + k], wt, val) : acc[jj * DPT + k];
                    fx_step(c1, inc_hi1, inc_lo1);
                    fx_step(c2, inc_hi2, inc_lo2);
                }
#pragma unroll
                for (int k = 0; k + UNR < DPT; ++k) acc[jj * DPT + k] = acc[jj * DPT + k + UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) acc[jj * DPT + DPT - UNR + k] = a[k];
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the next patch has landed ...
        __syncthreads();                                     // ... in every wave, and every gather from this buffer is done
        cur_buf ^= 1;
        cur = nxt;
        g = gn;
    }

    if (accumulate && !touched) return;                  // the output holds b already
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

}  // namespace vt
