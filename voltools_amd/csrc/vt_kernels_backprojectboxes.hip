// vt_kernels_backprojectboxes.hip -- nb boxes of one shape back-projected from one stack of images in ONE launch (kind 19), hand-written
// for gfx950 (MI355X, CDNA4): the per-particle reconstruction of sub-tomogram workflows, n small volumes straight from a resident tilt
// series.
//
// out[b][v] = float32(base[b][v] + sum_i weights[b, i] * B_{b,i}[v]): box b is what backproject_tiled (kind 18, vt_kernels_backproject.hip)
// writes for that box's n matrices and weights, bit for bit.  The kernel IS kind 18's text (vt_backproject_common.h) with a box index:
//
//   * One 256-thread workgroup per (box, box tile); grid = nb x tiles, box-major, blockIdx through xcd_contiguous, so the tiles of a box
//     are consecutive workgroups of one XCD, where their overlapping image patches share an L2.
//   * The workgroup moves tab / wts / out to its box (tab + b n, wts + b n, out + b box voxels; 64-bit offsets) and walks the n entries
//     with kind 18's patch_geo, next_staged, stage_patch into two LDS buffers with the next patch in flight, direct gather for untiled
//     entries, Q32.32 stepping, accumulator rotation and backproject_weighted_add.
//   * buf_floats is the largest staged patch of the whole batch: it places the second buffer and sizes the allocation, nothing else.
//     Whether an entry stages was decided on the host from that entry alone, so a box does not depend on its neighbours.
#include "vt_backproject_common.h"

#include <algorithm>

namespace vt {

typedef void (*backproject_boxes_fn)(const float*, float*, const float*, const ExtractEntry*, const double*, int, int, int, int,
                                     const AffineParams);

template <int TD, int TH, int TW>
static backproject_boxes_fn pick_backproject_boxes(int kind)
{
    switch (kind) {
        case 0: return backproject_tiled<0, TD, TH, TW, true>;
        case 1: return backproject_tiled<1, TD, TH, TW, true>;
        default: return backproject_tiled<2, TD, TH, TW, true>;
    }
}

// The extraction kernel's tile table (extract_tile).  extract_pick_tile never selects configuration 0, (16, 16, 16), for any box shape
// (tests/test_backproject_cases_host.py); it is instantiated because the table is shared and cfg indexes it.
static backproject_boxes_fn backproject_boxes_entry_point(int cfg, int kind)
{
    switch (cfg) {
        case 0: return pick_backproject_boxes<16, 16, 16>(kind);
        case 1: return pick_backproject_boxes<8, 16, 16>(kind);
        default: return pick_backproject_boxes<8, 8, 16>(kind);
    }
}

hipError_t init_backproject_boxes_kernels()
{
    for (int cfg = 0; cfg < extract_tile_count(); ++cfg)
        for (int kind = 0; kind < 3; ++kind) {
            hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(backproject_boxes_entry_point(cfg, kind)),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// grid = nb * p.nTd * nTh * nTw workgroups.  d_tab: nb x n entries, d_wts: nb x n weights, out: nb boxes of p.oD x oH x oW, all box-major.
// lds_bytes >= 2 * buf_floats * 4; every tiled entry's Ly * Lx <= buf_floats.
hipError_t launch_backproject_boxes(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                                    const double* d_wts, int nb, int n, int buf_floats, bool accumulate, const AffineParams& p,
                                    int lds_bytes, hipStream_t stream)
{
    const int64_t tiles = (int64_t)p.nTd * p.nTh * p.nTw;
    if (nb <= 0 || n <= 0 || tiles <= 0 || tiles > 0x7fffffffLL || (int64_t)nb * tiles > 0x7fffffffLL || buf_floats < 0 ||
        (buf_floats & 3) || (int64_t)buf_floats * 8 > lds_bytes)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(backproject_boxes_entry_point(cfg, interp_kind(interp)), dim3((unsigned)(nb * tiles)), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, n, buf_floats, accumulate ? 1 : 0, (int)tiles, p);
    return hipGetLastError();
}

}  // namespace vt
