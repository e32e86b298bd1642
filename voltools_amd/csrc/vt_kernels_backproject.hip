// vt_kernels_backproject.hip -- a stack of images ("tilt series") back-projected into one volume (kind 18), hand-written for gfx950
// (MI355X, CDNA4).
//
// The handle holds T images of H x W as its planes.  out[v] = float32(b[v] + sum_i weights[i] * B_i[v]) with B_i[v] the handle's
// interpolation taken IN TWO DIMENSIONS in plane planes[i] at (y, x) = rows 1 and 2 of pull matrix i applied to the output voxel index,
// 0 outside the skirt, and b = +0 or the output's current value (accumulate).  The transpose of project_tiled (vt_kernels_projbatch.hip):
// there a pixel sums the samples along a ray, here a voxel sums one sample per image.
//
//   * One 256-thread workgroup per output tile (extract_pick_tile's tile, place_tiled's thread <-> voxel mapping, accumulator rotation
//     and UNR), blockIdx through xcd_contiguous.  Every workgroup owns its tile: no memset, no atomics, no lists.
//   * Per entry (ExtractEntry, rows 1 and 2 as given, m[3] = the plane index; entry and weight by wave-uniform scalar loads): float64
//     bounding box of the tile in the image on rows 1 and 2, skip when it clears the valid interval by kTileMargin; the canonical float64
//     inside test per voxel on cut tiles; Q32.32 stepping along the tile's depth with place_tiled's restart points, so the fractions are
//     the ones place_tiled forms for the same rows.
//   * Staging: ONE plane's patch [o1, o1 + Ly) x [o2, o2 + Lx) by 16-byte direct-to-LDS loads, vectors outside the image from zeros16
//     (stage_box in two dimensions).  Half the bytes of the detour through place_tiled (two planes for linear, a quarter of the cubic's
//     four plus halo).
//   * Two LDS buffers.  While entry i is sampled from its buffer (LDS reads only), the patch of the next entry that reaches the tile is
//     already on its way into the other one; one barrier per entry, in front of which the outstanding LDS-DMA is drained (vmcnt(0)).
//     Entries are scalar loads and accumulate's pre-load sits before the loop, so no VGPR-destination global load shares the loop body
//     with a DMA in flight (hipcc would wait for everything at its first use).
//   * Entries whose patch fits no buffer (tiled == 0: strong minification, VT_FORCE_DIRECT) gather their taps from global memory in the
//     same loop, coordinates by the canonical chain.  They touch neither buffer nor the rotation: when one runs, the DMA issued in the
//     previous staged entry's iteration has been drained at that iteration's barrier.
//   * Sampling.  Linear: x0 = fmaf(fx, a01 - a00, a00), x1 likewise, fmaf(fy, x1 - x0, x0): sample_box<0>'s first two levels, so for a
//     matrix whose row 0 is (0, 0, 0, plane) the value is place_tiled's, bit for bit.  Cubic: 4 rows x 4 taps, three ds_read_b64 per
//     row, column sums, parity select: cubic_gather_b64 cut down to one plane.
//
// The kernel's text is in vt_backproject_common.h: backproject_tiled<KIND, TD, TH, TW, BOXES>, shared with kind 19
// (vt_kernels_backprojectboxes.hip, BOXES = true).  This file instantiates BOXES = false: gridDim.x = output tiles, `tiles` is not read.
#include "vt_backproject_common.h"

#include <algorithm>

namespace vt {

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
VT_BOX_KERNELS(backproject, backproject_tiled<KIND, T::TD, T::TH, T::TW, false>)

// grid = p.nTd * nTh * nTw workgroups.  lds_bytes >= 2 * buf_floats * 4; every tiled entry's Ly * Lx <= buf_floats.
hipError_t launch_backproject(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                              const double* d_wts, int n, int buf_floats, bool accumulate, const AffineParams& p, int lds_bytes,
                              hipStream_t stream)
{
    const int64_t grid = (int64_t)p.nTd * p.nTh * p.nTw;
    if (n <= 0 || grid <= 0 || grid > 0x7fffffffLL || buf_floats < 0 || (buf_floats & 3) || (int64_t)buf_floats * 8 > lds_bytes)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(backproject_kernels.fn[cfg][interp_kind(interp)], dim3((unsigned)grid), dim3(256), lds_bytes, stream,
                       src, out, zeros16, d_tab, d_wts, n, buf_floats, accumulate ? 1 : 0, 0, p);
    return hipGetLastError();
}

}  // namespace vt
