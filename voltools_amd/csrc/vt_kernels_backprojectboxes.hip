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
//     entries, Q32.32 stepping, accumulator rotation and weighted_add.
//   * buf_floats is the largest staged patch of the whole batch: it places the second buffer and sizes the allocation, nothing else.
//     Whether an entry stages was decided on the host from that entry alone, so a box does not depend on its neighbours.
#include "vt_backproject_common.h"

#include <algorithm>

namespace vt {

// extract_pick_tile never selects configuration 0, (16, 16, 16), for any box shape (tests/test_backproject_cases_host.py); it is
// instantiated because the tile table is shared and cfg indexes it.
VT_BOX_KERNELS(backproject_boxes, backproject_tiled<KIND, T::TD, T::TH, T::TW, true>)

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
    hipLaunchKernelGGL(backproject_boxes_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)(nb * tiles)), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, n, buf_floats, accumulate ? 1 : 0, (int)tiles, p);
    return hipGetLastError();
}

}  // namespace vt
