// vt_kernels_stackaffine.hip -- every image of a resident stack resampled under its own 2-D affine map (kind 21), hand-written for gfx950
// (MI355X, CDNA4): tilt alignment before reconstruction, movie frames shifted onto each other, a stack resampled onto another grid.
//
// The handle holds T images of H x W as its planes.  For output pixel (h, w) of output image i
//     y = fma(M_i[1,1], h, fma(M_i[1,2], w, M_i[1,3])),  x = fma(M_i[2,1], h, fma(M_i[2,2], w, M_i[2,3]))          float64
//     out[i, h, w] = float32(weighted_add(+0.0, w_i, B))  where -0.5 <= y < H - 0.5 and -0.5 <= x < W - 0.5, else +0
// with B the handle's interpolation IN TWO DIMENSIONS in image planes[i] at ((int)floor(y), (float)(y - floor(y))), the same for x, taps
// outside the image 0: backproject_tiled's definition (vt_backproject_common.h) for one entry and an output of depth 1.
//
//   * One 256-thread workgroup per (entry, 2-D output tile); the tile is 32 x 32 (four pixels per thread) or 16 x 16, a function of (Ho,
//     Wo, interpolation) only (stack_affine_pick_tile).  Thread <-> pixel mapping: BoxTileMap<1, TH, TW>, lanes along w, so a wave stores
//     whole tile rows of 128 or 64 bytes.
//   * Grid = n x tiles, entry-major through xcd_contiguous: the tiles of one image are consecutive workgroups of one XCD, where their
//     overlapping patches share an L2.
//   * The entry (ExtractEntry: m[3] = the plane, rows 1 and 2 of the matrix, the reach of the tile, the patch dims) and its weight are read
//     by wave-uniform scalar loads.  patch_geo (rows 1 and 2, float64, kTileMargin) classifies the tile: wholly outside -> zeros; cut by
//     the skirt -> every pixel is tested; otherwise no pixel is.  Tiles cut by the end of the output skip the pixels beyond it.
//   * Staging: ONE patch [o1, o1 + Ly) x [o2, o2 + Lx) by stage_patch (16-byte direct-to-LDS loads, vectors outside the image from
//     zeros16), s_waitcnt vmcnt(0), one barrier.  There is no second buffer: a workgroup does not hide its own load, the other workgroups
//     of the CU do, which is why the patch is capped (kStackAffinePatchCap) where five workgroups still fit a CU's LDS.
//   * Coordinates: the canonical chain above for every pixel, not Q32.32 stepping -- there is no depth march to amortise a start over.
//     sample_patch<KIND> at (floor - origin) with the fractions of the chain.  The staged loop is branch-free (stack_affine_rows): the
//     inside test selects, so a thread's gathers are in flight together instead of one LDS round trip per pixel.
//   * Entries with tiled == 0 (patch beyond the cap, VT_FORCE_DIRECT) gather with direct_sample_2d<KIND> at the same (floor, fraction) in
//     the same launch.  Linear: the same taps and arithmetic as the staged route, hence the same bits.  With every entry direct the image
//     is backproject_tiled's direct route for that entry alone and depth 1, bit for bit: its chain starts with fma(m, 0.0, X) == X.
#include "vt_backproject_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace vt {

// One pixel (h, w): the canonical chain, the inside test (WHOLE: none), the sample.  STAGED: every pixel of the tile, inside the skirt or
// not, within the output or not, has its taps in the staged patch (the patch holds the bounding box of the whole tile), so the sample
// is taken without a branch and the test selects.  !STAGED: taps from global memory, only for a pixel of the output that passes the test.
template <int KIND, bool STAGED, bool WHOLE>
__device__ __forceinline__ float stack_affine_pixel(const float* __restrict__ lds, const float* __restrict__ img, const ExtractEntry& e,
                                                    const double wt, const AffineParams& p, const PatchGeo& g, const int h, const int w)
{
    static_assert(STAGED || !WHOLE, "the global-memory route tests every pixel");
    const double y = fma(e.m[5], (double)h, fma(e.m[6], (double)w, e.m[7]));
    const double x = fma(e.m[9], (double)h, fma(e.m[10], (double)w, e.m[11]));
    const bool inside = WHOLE || ((y >= p.vlo[1]) && (y < p.vhi[1]) && (x >= p.vlo[2]) && (x < p.vhi[2]));
    const double fyd = floor(y), fxd = floor(x);
    const float fy = (float)(y - fyd), fx = (float)(x - fxd);
    if constexpr (STAGED) {
        const float val = sample_patch<KIND>(lds, e.Lx, (int)fyd - g.o1, (int)fxd - g.o2, fy, fx);
        return inside ? (float)weighted_add(0.0, wt, val) : 0.0f;
    } else {
        if (!(inside && h < p.oH && w < p.oW)) return 0.0f;
        return (float)weighted_add(0.0, wt, direct_sample_2d<KIND>(img, p, (int)fyd, (int)fxd, fy, fx));
    }
}

// The thread's NJ pixels (h_first + jj * RP, w).  Linear from the patch: unrolled, the NJ gathers in flight together, stores at the end
// (one LDS round trip per thread instead of one per pixel).  Cubic from the patch (a gather holds 12 register pairs and waits for its
// own reads) and the global-memory route: one pixel at a time.
template <int KIND, int NJ, int RP, bool STAGED, bool WHOLE>
__device__ __forceinline__ void stack_affine_rows(const float* __restrict__ lds, const float* __restrict__ img, float* __restrict__ out,
                                                  const ExtractEntry& e, const double wt, const AffineParams& p, const PatchGeo& g,
                                                  const int h_first, const int w)
{
    if constexpr (KIND == 0 && STAGED) {
        float r[NJ];
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) r[jj] = stack_affine_pixel<KIND, STAGED, WHOLE>(lds, img, e, wt, p, g, h_first + jj * RP, w);
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h_first + jj * RP;
            if (WHOLE || (h < p.oH && w < p.oW)) out[(int64_t)h * p.oW + w] = r[jj];
        }
    } else {
#pragma unroll 1
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h_first + jj * RP;
            const float r = stack_affine_pixel<KIND, STAGED, WHOLE>(lds, img, e, wt, p, g, h, w);
            if (WHOLE || (h < p.oH && w < p.oW)) out[(int64_t)h * p.oW + w] = r;
        }
    }
}

// p.nTh / nTw = tiles of one output image (p.nTd = 1), p.oH / oW = the image; gridDim.x = n x tiles, `tiles` = p.nTh * p.nTw.
// Dynamic LDS holds the largest staged patch of the batch; which entries stage was decided per entry on the host.
template <int KIND /*0 linear, 1 cubic (bspline_weights), 2 cubic (bspline fn)*/, int TH, int TW>
__global__ __launch_bounds__(256) void stack_affine_tiled(const float* __restrict__ src, float* __restrict__ out,
                                                           const float* __restrict__ zeros16, const ExtractEntry* __restrict__ tab,
                                                           const double* __restrict__ wts, const int tiles, const AffineParams p)
{
    using M = BoxTileMap<1, TH, TW>;
    constexpr int NJ = M::NJ, RP = M::RP;
    constexpr int HALO = KIND != 0 ? 1 : 0;
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int tid = threadIdx.x;
    int u = xcd_contiguous(blockIdx.x, gridDim.x);
    const int ent = u / tiles;                               // workgroup-uniform
    u -= ent * tiles;
    const ExtractEntry& e = tab[ent];                        // wave-uniform index: scalar loads
    const double wt = wts[ent];
    out += (int64_t)ent * ((int64_t)p.oH * p.oW);            // 64-bit: n images pass 2^31 pixels long before one does
    int d0, h0, w0;
    M::tile_origin(u, p, d0, h0, w0);
    int kw, jh0, i0;
    M::thread_origin(tid, kw, jh0, i0);
    const int w = w0 + kw;

    PatchGeo g;
    if (!patch_geo<HALO>(e, p, 0, h0, w0, g)) {              // the tile maps outside the image
#pragma unroll
        for (int jj = 0; jj < NJ; ++jj) {
            const int h = h0 + jh0 + jj * RP;
            if (h < p.oH && w < p.oW) out[(int64_t)h * p.oW + w] = 0.0f;
        }
        return;
    }
    const float* img = src + (int64_t)(int)e.m[3] * ((int64_t)p.sH * p.sP);
    const bool staged = e.tiled != 0;                        // workgroup-uniform
    if (staged) {
        stage_patch(lds, img, zeros16, p, g.o1, g.o2, e.Ly, e.Lx, tid);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // the LDS-DMA has landed ...
        __syncthreads();                                     // ... in every wave
    }
    const bool whole = g.all_valid && (h0 + TH <= p.oH) && (w0 + TW <= p.oW);
    if (!staged)
        stack_affine_rows<KIND, NJ, RP, false, false>(lds, img, out, e, wt, p, g, h0 + jh0, w);
    else if (whole)
        stack_affine_rows<KIND, NJ, RP, true, true>(lds, img, out, e, wt, p, g, h0 + jh0, w);
    else
        stack_affine_rows<KIND, NJ, RP, true, false>(lds, img, out, e, wt, p, g, h0 + jh0, w);
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
namespace {

constexpr int kStackTiles[2][2] = {{32, 32}, {16, 16}};

// extract_box_dims' formula on rows 1 and 2 for the tile (1, TH, TW): false when the extent is absurd
bool stack_patch_dims(const double m[12], int th, int tw, int halo2, int* Ly, int* Lx)
{
    int L[2];
    for (int r = 1; r <= 2; ++r) {
        const double ext = std::fabs(m[4 * r + 1]) * (th - 1) + std::fabs(m[4 * r + 2]) * (tw - 1);
        if (!(ext < 4096.0)) return false;
        L[r - 1] = (int)std::floor(ext + 2.0 * kBoxMargin) + 3 + halo2;
    }
    *Ly = L[0];
    *Lx = (L[1] + 3 + 3) & ~3;                               // origin aligned down by up to 3, stride multiple of 4
    return true;
}

using StackAffineFn = void (*)(const float*, float*, const float*, const ExtractEntry*, const double*, int, AffineParams);
const StackAffineFn stack_affine_kernels[2][3] = {
    {stack_affine_tiled<0, 32, 32>, stack_affine_tiled<1, 32, 32>, stack_affine_tiled<2, 32, 32>},
    {stack_affine_tiled<0, 16, 16>, stack_affine_tiled<1, 16, 16>, stack_affine_tiled<2, 16, 16>},
};

}  // namespace

void stack_affine_tile(int idx, int* th, int* tw) { *th = kStackTiles[idx][0]; *tw = kStackTiles[idx][1]; }

// The tile of an (output image shape, interpolation) pair -- never of the matrices: staged bytes of the whole image (tiles that hang over
// its end count in full) for the typical rotation, |m[r][k]| = 1/2 (extract_pick_tile's).  The larger tile wins a tie.
int stack_affine_pick_tile(bool cubic, int oh, int ow)
{
    const double typical[12] = {0, 0, 0, 0, 0, 0.5, 0.5, 0, 0, 0.5, 0.5, 0};
    int best = 0;
    double best_cost = 1e300;
    for (int cfg = 0; cfg < 2; ++cfg) {
        const int th = kStackTiles[cfg][0], tw = kStackTiles[cfg][1];
        int Ly, Lx;
        stack_patch_dims(typical, th, tw, cubic ? 2 : 0, &Ly, &Lx);
        const double cost = (double)Ly * Lx * (double)((oh + th - 1) / th) * (double)((ow + tw - 1) / tw);
        if (cost < best_cost) { best_cost = cost; best = cfg; }
    }
    return best;
}

// One table entry: row 0 = (0, 0, 0, plane), rows 1 and 2 = columns 1, 2, 3 of rows 1 and 2 of the caller's matrix (column 0 belongs to
// the depth index, which an image does not have).  `tiled` iff the entry's own patch, cubic halo included, fits kStackAffinePatchCap and
// the terms of its coordinate chain stay below 2^24 over the output: then the six roundings of a pixel's chain and of the tile's base
// together stay below 6 x 2^-29 < kBoxMargin, and every tap of a pixel lies inside the patch that patch_geo places from the base.
void stack_affine_fill_entry(const double rows[8], int plane, int cfg, bool cubic, int oh, int ow, bool force_direct, ExtractEntry* e)
{
    const int th = kStackTiles[cfg][0], tw = kStackTiles[cfg][1];
    std::memset(e, 0, sizeof(*e));
    e->m[3] = (double)plane;
    for (int r = 1; r <= 2; ++r) {
        const double* a = rows + 4 * (r - 1);
        e->m[4 * r + 1] = a[1]; e->m[4 * r + 2] = a[2]; e->m[4 * r + 3] = a[3];
        double neg = 0, pos = 0;                             // set_tile_reach
        const double xs[2] = {a[1] * (th - 1), a[2] * (tw - 1)};
        for (double x : xs) { if (x < 0) neg += x; else pos += x; }
        e->neg[r] = neg; e->pos[r] = pos;
    }
    int Ly, Lx;
    const bool small = std::fabs(e->m[5]) * oh + std::fabs(e->m[6]) * ow + std::fabs(e->m[7]) < 16777216.0 &&
                       std::fabs(e->m[9]) * oh + std::fabs(e->m[10]) * ow + std::fabs(e->m[11]) < 16777216.0;
    if (!force_direct && small && stack_patch_dims(e->m, th, tw, cubic ? 2 : 0, &Ly, &Lx) &&
        (int64_t)Ly * Lx * 4 <= kStackAffinePatchCap) {
        e->Lz = 1; e->Ly = Ly; e->Lx = Lx;
        e->tiled = 1;
    }
}

// grid = n * p.nTh * p.nTw workgroups, entry-major.  d_tab: n entries, d_wts: n weights, out: n images of p.oH x oW.  lds_bytes >= 4 Ly Lx
// of every tiled entry.
hipError_t launch_stack_affine(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                               const double* d_wts, int n, const AffineParams& p, int lds_bytes, hipStream_t stream)
{
    const int64_t tiles = (int64_t)p.nTh * p.nTw;
    if (n <= 0 || tiles <= 0 || p.nTd != 1 || (int64_t)n * tiles > 0x7fffffffLL || lds_bytes < 0 || lds_bytes > kStackAffinePatchCap)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(stack_affine_kernels[cfg][interp_kind(interp)], dim3((unsigned)(n * tiles)), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, (int)tiles, p);
    return hipGetLastError();
}

}  // namespace vt
