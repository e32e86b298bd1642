// vt_kernels_filterstack.hip -- a 1-D filter along axis 1 or 2 of every image of a resident stack (kind 23), hand-written for gfx950
// (MI355X, CDNA4): the ramp filter of weighted back-projection between alignment and reconstruction, per-tilt low-pass, smoothing,
// derivative taps.
//
// The handle holds T images of H x W as its planes.  With L the extent of the filtered axis, r = (k - 1) / 2 and t the tap row of entry i,
// for output pixel (h, w) of output image i (axis 2; axis 1 the same along h)
//     acc = +0.0
//     for j ascending over the NON-ZERO taps:  x = w + r - j;  acc = fma(t[j], (double)S[planes[i], h, pad(x)], acc)
//     out[i, h, w] = float32(w_i * acc)
// pad(x): pad 1 clamps x into [0, L); pad 0 reads 0 outside, which leaves acc as it was (see vt_volume_filter_stack for the one
// exception, a -0 accumulator).  The host compacts each tap row into FilterTap pairs (t, j) of its non-zero taps.
//
//   * One 256-thread workgroup per (entry, strip of kFilterStrip = 64 lines across the unfiltered axis, segment of kFilterSeg = 64 outputs
//     along the filtered axis); grid = n x strips x segments, entry-major, segments fastest.  Lane <-> line, wave <-> 16 consecutive
//     outputs along the filtered axis, held as 16 float64 accumulators per lane: axis 1 and axis 2 are the same loop.
//   * The taps are walked in chunks of at most kFilterChunk = 128 consecutive j.  Per chunk the workgroup stages the kFilterSeg +
//     kFilterChunk - 1 positions its outputs reach, for its 64 lines, as float32 at lds[position * 65 + line]: pad values are written
//     here, so the inner loop has no bounds test.  Reads (lanes along the line index) are consecutive dwords; staging writes of axis 2
//     (lanes along the position) have stride 65 dwords, distinct banks modulo 32.  Global loads are along w for both axes: lanes along
//     the position for axis 2, along the line for axis 1, twelve per thread in flight, on clamped addresses, the pad value selected
//     afterwards.  A chunk wholly outside the image under pad 0 is not staged at all.
//   * Taps are wave-uniform scalar loads.  The FilterTap pairs place the chunks (long runs of zero taps cost nothing); inside a chunk
//     the taps are read from the row itself, zeros included, which the host uploads padded by kFilterChunk zeros.  A chunk is walked in
//     groups of 16 consecutive j: the 31 samples a lane's 16 outputs reach under a group are read from LDS and widened once into a
//     register window, and each non-zero tap of the group is 16 fmas on the window at a static shift (16 unrolled bodies, each behind a
//     wave-uniform test of its tap).  A dense group is 256 fmas per 31 reads and widenings, a Ram-Lak group 128; a group of zero taps
//     is skipped.  The fma chain of an output is the same whatever the grouping.
//   * No image extent and no tap count is refused for LDS: the staged block is (kFilterSeg + kFilterChunk - 1) x 65 floats whatever they are.
#include "vt_internal.h"

#include <cstdint>

namespace vt {

namespace {
constexpr int kFilterU = kFilterSeg / 4;                     // outputs per lane: four waves share a segment
constexpr int kFilterPitch = kFilterStrip + 1;
constexpr int kFilterRows = kFilterSeg + kFilterChunk - 1;   // staged positions along the filtered axis
constexpr int kFilterGroup = 16;                             // consecutive j served by one register window
constexpr int kFilterBatch = 12;                             // staging loads a thread has in flight
static_assert(kFilterStrip == 64, "one lane per line");
static_assert(kFilterChunk % kFilterGroup == 0, "whole groups per chunk");
}  // namespace

// lineStride / posStride: floats between neighbours across / along the filtered axis in the source (axis 2: P, 1; axis 1: 1, P) and in
// the output (axis 2: W, 1; axis 1: 1, W).  lines = extent across, L = extent along.  AXIS2: lanes of the staging loads run along the
// position (the w axis), otherwise along the line (the w axis again).
template <bool AXIS2>
__global__ __launch_bounds__(256) void filter_stack_kernel(const float* __restrict__ src, float* __restrict__ out,
                                                           const FilterEntry* __restrict__ tab, const FilterTap* __restrict__ taps,
                                                           const double* __restrict__ rows,
                                                           const int strips, const int segs, const int lines, const int L, const int r,
                                                           const int pad, const int64_t srcPlane, const int srcPitch, const int outPitch)
{
    __shared__ float lds[kFilterRows * kFilterPitch];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int u = blockIdx.x;
    const int per = strips * segs;
    const int ent = u / per;                                 // workgroup-uniform
    u -= ent * per;
    const int strip = u / segs, seg = u - strip * segs;
    const FilterEntry e = tab[ent];                          // wave-uniform index: scalar loads
    const FilterTap* __restrict__ tp = taps + e.first;
    const double* __restrict__ dense = rows + e.dense;
    const float* __restrict__ img = src + (int64_t)e.plane * srcPlane;
    const int line0 = strip * kFilterStrip, seg0 = seg * kFilterSeg;

    double acc[kFilterU];
#pragma unroll
    for (int o = 0; o < kFilterU; ++o) acc[o] = 0.0;

    int c = 0;
    while (c < e.nnz) {                                      // uniform: every wave walks the same chunks
        const int64_t ja = tp[c].j;
        // the chunk covers taps j in [ja, ja + kFilterChunk); staged row xx holds source position x0 + xx
        const int64_t x0 = (int64_t)seg0 + r - ja - (kFilterChunk - 1);
        int c1 = c;
        while (c1 < e.nnz && tp[c1].j < ja + kFilterChunk) ++c1;
        if (pad == 0 && (x0 + kFilterRows <= 0 || x0 >= L)) { c = c1; continue; }       // every staged sample would be 0

        // Staging in batches of kFilterBatch loads per thread, all issued before the first is used.  Every load has a valid address (the
        // line and the position are clamped); what the block must hold instead -- 0 outside under pad 0 -- is selected afterwards.
        // (positions in 32 bits: x0 clamped into [-kFilterRows, L] classifies every staged position as x0 itself does, and L + kFilterRows
        // fits by the entry point's bound on the extent)
        const int xs = (int)(x0 < -kFilterRows ? (int64_t)-kFilterRows : (x0 > L ? (int64_t)L : x0));
        const auto sample_at = [&](const int line, const int xx, float& s, bool& keep) {
            const int x = xs + xx;
            const int xc = x < 0 ? 0 : (x >= L ? L - 1 : x);
            const int lc = line < lines ? line : lines - 1;
            if constexpr (AXIS2) s = img[(uint64_t)(uint32_t)lc * (uint32_t)srcPitch + (uint32_t)xc];
            else s = img[(uint64_t)(uint32_t)xc * (uint32_t)srcPitch + (uint32_t)lc];
            keep = line < lines && (pad != 0 || (unsigned)x < (unsigned)L);
        };
        // (an empty asm that takes the loaded value keeps the compiler from sinking the load under `keep`, where every load would wait
        // for itself)
        const auto pin = [](float& s) { asm volatile("" : "+v"(s)); };
        if constexpr (AXIS2) {
            constexpr int XT = (kFilterRows + 63) / 64, LQ = kFilterBatch / XT;
            static_assert((kFilterStrip / 4) % LQ == 0, "whole batches of lines per wave");
#pragma unroll 1
            for (int l0 = wave; l0 < kFilterStrip; l0 += 4 * LQ) {
                float s[LQ][XT];
                bool keep[LQ][XT];
#pragma unroll
                for (int q = 0; q < LQ; ++q)
#pragma unroll
                    for (int t = 0; t < XT; ++t) sample_at(line0 + l0 + 4 * q, lane + 64 * t, s[q][t], keep[q][t]);
#pragma unroll
                for (int q = 0; q < LQ; ++q)
#pragma unroll
                    for (int t = 0; t < XT; ++t) pin(s[q][t]);
#pragma unroll
                for (int q = 0; q < LQ; ++q)
#pragma unroll
                    for (int t = 0; t < XT; ++t)
                        if (lane + 64 * t < kFilterRows) lds[(lane + 64 * t) * kFilterPitch + l0 + 4 * q] = keep[q][t] ? s[q][t] : 0.0f;
            }
        } else {
            constexpr int XQ = (kFilterRows + 3) / 4;       // staged positions per wave
            static_assert(XQ % kFilterBatch == 0, "whole batches of positions per wave");
#pragma unroll 1
            for (int i0 = 0; i0 < XQ; i0 += kFilterBatch) {
                float s[kFilterBatch];
                bool keep[kFilterBatch];
#pragma unroll
                for (int q = 0; q < kFilterBatch; ++q) sample_at(line0 + lane, wave + 4 * (i0 + q), s[q], keep[q]);
#pragma unroll
                for (int q = 0; q < kFilterBatch; ++q) pin(s[q]);
#pragma unroll
                for (int q = 0; q < kFilterBatch; ++q) {
                    const int xx = wave + 4 * (i0 + q);
                    if (xx < kFilterRows) lds[xx * kFilterPitch + lane] = keep[q] ? s[q] : 0.0f;
                }
            }
        }
        __syncthreads();

        // The chunk in groups of kFilterGroup consecutive j: the kFilterU + kFilterGroup - 1 samples the lane's outputs reach under
        // the group's taps are read and widened ONCE into a register window, and tap j of the group is kFilterU fmas on the window at
        // the static shift kFilterGroup - 1 - (j - first j of the group), taken or skipped by a wave-uniform branch on the tap's value in the dense row.
        const float* __restrict__ mine = lds + (wave * kFilterU) * kFilterPitch + lane;
        for (int g = 0; g < kFilterChunk / kFilterGroup && c < c1; ++g) {
            const int64_t jb = ja + g * kFilterGroup;
            if (tp[c].j >= jb + kFilterGroup) continue;     // the group holds zero taps only
            const float* __restrict__ at = mine + (kFilterChunk - (g + 1) * kFilterGroup) * kFilterPitch;
            double win[kFilterU + kFilterGroup - 1];
#pragma unroll
            for (int i = 0; i < kFilterU + kFilterGroup - 1; ++i) win[i] = (double)at[i * kFilterPitch];
            const double* __restrict__ row = dense + jb;
            double tg[kFilterGroup];                        // wave-uniform, zeros included: the row is padded by kFilterChunk zeros;
#pragma unroll
            for (int d = 0; d < kFilterGroup; ++d) tg[d] = row[d];      // read together, ahead of the branches, as wide scalar loads
#pragma unroll
            for (int d = 0; d < kFilterGroup; ++d) {
                const double t = tg[d];
                const uint64_t tb = __builtin_bit_cast(uint64_t, t);
                if ((((uint32_t)(tb >> 32) & 0x7fffffffu) | (uint32_t)tb) != 0u) {      // t != 0, either sign, on the scalar unit
#pragma unroll
                    for (int o = 0; o < kFilterU; ++o) acc[o] = fma(t, win[o + kFilterGroup - 1 - d], acc[o]);
                    ++c;
                }
            }
        }
        __syncthreads();                                     // the next chunk overwrites the block
    }

    const int line = line0 + lane;
    if (line >= lines) return;
    const int64_t outLine = AXIS2 ? outPitch : 1, outPos = AXIS2 ? 1 : outPitch;
    float* __restrict__ o_at = out + (int64_t)ent * ((int64_t)lines * L) + (int64_t)line * outLine;
    const int first = seg0 + wave * kFilterU;
#pragma unroll
    for (int o = 0; o < kFilterU; ++o) {
        const int x = first + o;
        if (x < L) o_at[(int64_t)x * outPos] = e.nnz == 0 ? 0.0f : (float)(e.weight * acc[o]);
    }
}

// grid = n x strips x segs workgroups, entry-major.  d_tab: n entries, d_taps: the compacted tap rows they point into, d_rows: the rows
// themselves, each followed by kFilterChunk zeros, out: n images of H x W.  axis: 1 or 2, pad: 0 or 1, k: the odd tap count of the caller's rows.
hipError_t launch_filter_stack(const float* src, float* out, const FilterEntry* d_tab, const FilterTap* d_taps, const double* d_rows, int n,
                               int H, int W, int P, int axis, int pad, int k, hipStream_t stream)
{
    if (n <= 0 || H <= 0 || W <= 0 || P < W || (axis != 1 && axis != 2) || (pad != 0 && pad != 1) || k < 1 || !(k & 1))
        return hipErrorInvalidValue;
    const int L = axis == 2 ? W : H, lines = axis == 2 ? H : W;
    const int64_t strips = filter_stack_strips(lines), segs = filter_stack_segments(L);
    if (strips * segs * n > 0x7fffffffLL) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(strips * segs * n)), block(256);
    const int64_t plane = (int64_t)H * P;
    if (axis == 2)
        hipLaunchKernelGGL(filter_stack_kernel<true>, grid, block, 0, stream, src, out, d_tab, d_taps, d_rows, (int)strips, (int)segs, lines, L,
                           (k - 1) / 2, pad, plane, P, W);
    else
        hipLaunchKernelGGL(filter_stack_kernel<false>, grid, block, 0, stream, src, out, d_tab, d_taps, d_rows, (int)strips, (int)segs, lines, L,
                           (k - 1) / 2, pad, plane, P, W);
    return hipGetLastError();
}

}  // namespace vt
