// vt_box_common.h -- what the box kernels (kinds 11-19) share, each fragment once: the tile table, the thread <-> voxel mapping of a
// 256-thread workgroup on a tile, the float64 tile geometry, the canonical inside test, the Q32.32 start and step, the rounding helpers
// of the reductions, and the host-side table of a kernel template's instantiations.  A kernel of the family keeps what is its own: the
// decode from workgroup id to (entry, tile index), its reduction, its unroll and fence choices, its stores, its shape plan and its
// launcher's argument checks.
//
// Bit-for-bit equality between these kernels is a contract (box b of kind 19 is kind 18's volume, the columns of kind 15 are kind
// 14's, kind 13 sums kind 11's samples, ...).  It rests on every value below being formed by ONE text compiled with the same flags.
// The device functions here are __forceinline__ fragments without control flow; the two fragments that hold a short-circuit chain (tile
// geometry, inside test) are statement macros, because only text expanded in place compiles as the spelled-out copies did.
#pragma once
#include "vt_internal.h"
#include "vt_device.h"

#include <utility>

namespace vt {

// ---------------------------------------------------------------------------------------------------
// the family's tiles: extract_pick_tile chooses among them, cfg indexes them
// ---------------------------------------------------------------------------------------------------
struct ExtractTile { int td, th, tw; };
constexpr ExtractTile kExtractTiles[] = {
    {16, 16, 16},   // 0: cube -- fewest staged bytes per voxel, one workgroup per CU under a general rotation
    {8, 16, 16},    // 1: half cube
    {8, 8, 16},     // 2: quarter cube -- a general cubic rotation stages under 40 KiB
};
constexpr int kExtractTileCount = (int)(sizeof(kExtractTiles) / sizeof(kExtractTiles[0]));

template <int CFG>
struct ExtractTileAt {
    static constexpr int TD = kExtractTiles[CFG].td, TH = kExtractTiles[CFG].th, TW = kExtractTiles[CFG].tw;
};

// ---------------------------------------------------------------------------------------------------
// 256 threads on a TD x TH x TW tile
// ---------------------------------------------------------------------------------------------------
// lanes run along w, then h; tiles of fewer than 256 in-plane positions split their depth between lane groups
template <int TD, int TH, int TW>
struct BoxTileMap {
    static constexpr int NPOS = TH * TW;
    static_assert(256 % TW == 0 && (NPOS >= 256 ? NPOS % 256 == 0 : 256 % NPOS == 0), "tile/thread mapping");
    static constexpr int DG = NPOS >= 256 ? 1 : 256 / NPOS;     // depth groups
    static constexpr int NJ = NPOS >= 256 ? NPOS / 256 : 1;     // in-plane passes
    static constexpr int RP = NPOS >= 256 ? 256 / TW : TH;      // tile rows covered per pass
    static constexpr int DPT = TD / DG;                         // planes per thread
    static_assert(TD % DG == 0, "tile depth / lane groups");
    static constexpr int NV = NJ * DPT;                         // voxels per thread

    // first voxel of tile u of a p.nTd x nTh x nTw grid of tiles, w fastest
    static __device__ __forceinline__ void tile_origin(int u, const AffineParams& p, int& d0, int& h0, int& w0)
    {
        const int tw_i = u % p.nTw;
        const int u2 = u / p.nTw;
        const int th_i = u2 % p.nTh;
        const int td_i = u2 / p.nTh;
        d0 = td_i * TD; h0 = th_i * TH; w0 = tw_i * TW;
    }

    // the thread's voxels within the tile: column kw, rows jh0 + jj * RP (jj < NJ), planes i0 .. i0 + DPT - 1.  Returns the in-plane
    // position (the thread id within its depth group).
    static __device__ __forceinline__ int thread_origin(int tid, int& kw, int& jh0, int& i0)
    {
        const int pos = DG > 1 ? tid % NPOS : tid;
        kw = pos % TW;
        jh0 = pos / TW;
        i0 = DG > 1 ? (tid / NPOS) * DPT : 0;
        return pos;
    }
};

// ---------------------------------------------------------------------------------------------------
// tile geometry (wave-uniform, float64)
// ---------------------------------------------------------------------------------------------------
// base = source coordinate of the tile's first voxel, lo = lower corner of the tile's bounding box in the source (base plus the
// entry's tile reach).  any_valid (true on entry) stays true iff the box meets the valid interval widened by kTileMargin -- otherwise
// the tile is wholly outside; all_valid (true on entry) iff it lies inside the interval narrowed by kTileMargin -- then no voxel needs
// a test of its own.  A statement macro for VT_CANONICAL_INSIDE's reason (below): as a function it cost kind 13's cubic instantiations
// 4 to 6 SGPR spills where they had none, and one instantiation of kind 16 312 VGPRs for 150.
#define VT_BOX_TILE_GEOMETRY(base, lo, any_valid, all_valid, e, p, d0, h0, w0)                                                             \
    {                                                                                                                                      \
        double hi_[3];                                                                                                                     \
        _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_) {                                                                                 \
            (base)[r_] = fma((e).m[4 * r_], (double)(d0), fma((e).m[4 * r_ + 1], (double)(h0), fma((e).m[4 * r_ + 2], (double)(w0), (e).m[4 * r_ + 3]))); \
            (lo)[r_] = (base)[r_] + (e).neg[r_];                                                                                           \
            hi_[r_] = (base)[r_] + (e).pos[r_];                                                                                            \
            (any_valid) = (any_valid) && (hi_[r_] >= (p).vlo[r_] - kTileMargin) && ((lo)[r_] < (p).vhi[r_] + kTileMargin);                 \
            (all_valid) = (all_valid) && ((lo)[r_] >= (p).vlo[r_] + kTileMargin) && (hi_[r_] < (p).vhi[r_] - kTileMargin);                 \
        }                                                                                                                                  \
    }

// integer origin of the staged box (finite and small: the tile meets the valid interval, its extent was bounded on the host); o[2] is a
// multiple of 4 for the 16-byte loads (vt_device.h: kBoxMargin)
template <int HALO>
__device__ __forceinline__ void box_origin(const double (&lo)[3], int (&o)[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) o[r] = (int)floor(lo[r] - kBoxMargin) - HALO;
    o[2] &= ~3;
}

// ---------------------------------------------------------------------------------------------------
// the canonical float64 chain of output voxel (d, h, w) and its inside test (affine_direct's and the oracle's, vt_device.h: the skirt rule)
// ---------------------------------------------------------------------------------------------------
// Row r_ = 0, 1, 2 of the entry's matrix applied to (d, h, w) is assigned to the lvalue `s`; `inside` (true on entry, or whatever else
// the voxel has to satisfy) stays true iff vlo <= s < vhi on every axis.  The routes that gather from global memory keep the coordinates
// (s names the row: VT_CANONICAL_INSIDE(inside, s[r_], ..)); tiles cut by the valid interval or by the end of the box need the flag only
// and pass a scalar (their taps still come from the fixed-point split).
// A statement macro, not a function: a function is simplified on its own before it is inlined, which turns the short-circuit chain
// into 18 scalar loads live at once -- kind 14's cubic instantiations went from 3 waves per SIMD to 2 (161 -> 172 VGPRs), kinds 12, 13,
// 15 and 16 gained SGPR spills.  Expanded in place the chain compiles as it did when every kernel spelled it out.
#define VT_CANONICAL_INSIDE(inside, s, e, p, d, h, w)                                                                                      \
    _Pragma("unroll") for (int r_ = 0; r_ < 3; ++r_) {                                                                                     \
        s = fma((e).m[4 * r_], (double)(d), fma((e).m[4 * r_ + 1], (double)(h), fma((e).m[4 * r_ + 2], (double)(w), (e).m[4 * r_ + 3])));  \
        (inside) = (inside) && (s >= (p).vlo[r_]) && (s < (p).vhi[r_]);                                                                    \
    }

// ---------------------------------------------------------------------------------------------------
// Q32.32 stepping along the tile's depth (vt_device.h: Fx)
// ---------------------------------------------------------------------------------------------------
struct FxInc3 { int hi[3]; unsigned lo[3]; };

__device__ __forceinline__ FxInc3 fx_inc3(const ExtractEntry& e)
{
    return FxInc3{{e.inc_hi[0], e.inc_hi[1], e.inc_hi[2]}, {e.inc_lo[0], e.inc_lo[1], e.inc_lo[2]}};
}

// the tile's first voxel in the coordinates of the box staged at o
__device__ __forceinline__ void box_base(const double (&base)[3], const int (&o)[3], double (&b)[3])
{
#pragma unroll
    for (int r = 0; r < 3; ++r) b[r] = base[r] - (double)o[r];
}

// box coordinates of the voxel (i0, j, kw) of the tile: where a thread's column restarts, hence what fixes the samples' last bits
__device__ __forceinline__ void fx_start3(const ExtractEntry& e, const double (&b)[3], int i0, int j, int kw, Fx& c0, Fx& c1, Fx& c2)
{
    const double s0 = fma(e.m[0], (double)i0, fma(e.m[1], (double)j, fma(e.m[2], (double)kw, b[0])));
    const double s1 = fma(e.m[4], (double)i0, fma(e.m[5], (double)j, fma(e.m[6], (double)kw, b[1])));
    const double s2 = fma(e.m[8], (double)i0, fma(e.m[9], (double)j, fma(e.m[10], (double)kw, b[2])));
    c0 = to_fx(s0); c1 = to_fx(s1); c2 = to_fx(s2);
}

__device__ __forceinline__ void fx_step3(Fx& c0, Fx& c1, Fx& c2, const FxInc3& inc)
{
    fx_step(c0, inc.hi[0], inc.lo[0]);
    fx_step(c1, inc.hi[1], inc.lo[1]);
    fx_step(c2, inc.hi[2], inc.lo[2]);
}

// ---------------------------------------------------------------------------------------------------
// roundings of the reductions.  The translation units are compiled with -ffp-contract=fast; the contracts below name every rounding,
// so no product may be contracted into the addition that follows it.
// ---------------------------------------------------------------------------------------------------
// acc + w * v in float64 with both roundings: the expression a host loop in float64 evaluates (kinds 13, 16, 17, 18, 19)
__device__ __forceinline__ double weighted_add(double acc, double w, float v)
{
#pragma clang fp contract(off)
    const double t = w * (double)v;
    return acc + t;
}

// A product passed through an empty asm statement is a value of its own (rounded to float64) that no following addition can absorb into a
// fused multiply-add (kinds 14, 15).
__device__ __forceinline__ double rounded(double x)
{
    asm("" : "+v"(x));
    return x;
}

// lane 0 of the wave ends up with the sum over its 64 lanes, always by the same tree
__device__ __forceinline__ double wave_tree_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_down(x, off, 64);
    return x;
}

// ---------------------------------------------------------------------------------------------------
// host side: the instantiations of one kernel template, [tile of kExtractTiles][KIND]
// ---------------------------------------------------------------------------------------------------
// K<KIND, CFG>::fn() returns the kernel for interpolation KIND (interp_kind) on tile CFG.
template <template <int, int> class K>
struct BoxKernelTable {
    using Fn = decltype(K<0, 0>::fn());
    Fn fn[kExtractTileCount][3];

    BoxKernelTable() { fill(std::make_integer_sequence<int, kExtractTileCount>{}); }
    template <int... CFG>
    void fill(std::integer_sequence<int, CFG...>) { ((fn[CFG][0] = K<0, CFG>::fn(), fn[CFG][1] = K<1, CFG>::fn(), fn[CFG][2] = K<2, CFG>::fn()), ...); }

    // every instantiation may allocate the whole 160 KiB of dynamic LDS
    hipError_t raise_lds_limit() const
    {
        for (int cfg = 0; cfg < kExtractTileCount; ++cfg)
            for (int kind = 0; kind < 3; ++kind) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn[cfg][kind]), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   160 * 1024);
                if (e != hipSuccess) return e;
            }
        return hipSuccess;
    }
};

// One declaration per kernel template: the table `name_kernels` and init_name_kernels().  The last argument is the instantiation, written
// with KIND and the tile T::TD, T::TH, T::TW.
#define VT_BOX_KERNELS(name, ...)                                                                                  \
    template <int KIND, int CFG>                                                                                   \
    struct name##_kernel {                                                                                         \
        using T = ExtractTileAt<CFG>;                                                                              \
        static auto fn() { return &__VA_ARGS__; }                                                                  \
    };                                                                                                             \
    static const BoxKernelTable<name##_kernel> name##_kernels;                                                     \
    hipError_t init_##name##_kernels() { return name##_kernels.raise_lds_limit(); }

}  // namespace vt
