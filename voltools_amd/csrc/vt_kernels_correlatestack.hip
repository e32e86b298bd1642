// vt_kernels_correlatestack.hip -- shift scores of every image of a resident stack against a reference, per patch of a grid (kind 24),
// hand-written for gfx950 (MI355X, CDNA4): the cross-correlation over a window of integer shifts that coarse tilt alignment, patch
// tracking and local motion correction take their shifts from.
//
// The handle holds T images of H x W as its planes.  For entry i with image p and reference r, patch (a, b) of the grid and shift
// (u, v) of the window (rh, rw)
//     out[i, a, b, u, v] = sum over (y, x) of the patch of  (double) r[y, x] * (double) s(y + u - rh, x + v - rw)
//     s(y', x') = S[p, y', x'] inside the image, +0 outside
// every product exact, every addition rounded by fma, in this order:
//   * a patch is cut from its own first row and column into pieces of 64 x 64 pixels, piece (py, px) row-major, and a piece into four
//     bands of 16 rows;
//   * a band sum starts from +0 and takes its pixels row by row, ascending x within a row: acc = fma(r, s, acc);
//   * a piece sum is ((band 0 + band 1) + band 2) + band 3, a band the piece does not reach being +0;
//   * a score is the piece sums added in ascending piece index, starting from piece 0 itself.
// Nothing in it depends on the window, the grid beyond the patch's own rows and columns, or the batch.
//
//   * One 256-thread workgroup per (unit = (entry, patch), piece, block of shifts): wave <-> band, lane <-> (shift row, run of cv
//     consecutive column shifts), held as cv float64 accumulators, cv = 9 or 11.  A block is rows_blk shift rows x runs * cv shift
//     columns with rows_blk * runs <= 64; windows larger than a block go onto the grid.
//   * The workgroup stages the reference piece (64 x 64 floats, 16 KiB) and the image samples its block reaches for the piece:
//     ph + rows_blk - 1 rows of 63 + runs * cv samples, pitch 64 + runs * cv floats.  Zeros outside the image are written here, so the
//     inner loop has no bounds test.  The lane at (shift row ul, run j) reads lds[(y + ul) * pitch + x + j * cv + ..]: modulo the 32
//     banks of a dword read that is cv * lane + const, and cv is odd, so the 32 lanes of a read group fall on 32 banks.
//   * A band walks its reference rows 8 pixels at a time: the cv + 7 samples a lane's shifts reach under the 8 pixels are read and
//     widened once into a register window, the 8 reference values come as two 16-byte broadcast reads, and pixel d is cv fmas on the
//     window at the static offset d: 8 cv fmas per cv + 9 LDS reads.  A reference pixel past the piece's last column is skipped by a
//     wave-uniform branch, never multiplied: nothing outside the patch reaches a score.
//   * The four band sums meet in LDS and wave 0 adds them in ascending order.  With one piece per patch the scores are stored
//     straight to the output; otherwise to the partials, and correlate_stack_reduce adds them in ascending piece index.  No atomics, no
//     memset: a piece past the end of a patch smaller than the call's largest stores +0.
#include "vt_internal.h"

#include <algorithm>
#include <cstdint>

namespace vt {

CorrPlan correlate_stack_plan(int H, int W, int gh, int gw, int rh, int rw)
{
    CorrPlan c{};
    c.H = H; c.W = W; c.gh = gh; c.gw = gw; c.rh = rh; c.rw = rw;
    c.nu = 2 * rh + 1; c.nv = 2 * rw + 1;
    const int max_ph = (H + gh - 1) / gh, max_pw = (W + gw - 1) / gw;          // the largest patch of the grid
    c.pieces_y = (max_ph + kCorrPiece - 1) / kCorrPiece;
    c.pieces_x = (max_pw + kCorrPiece - 1) / kCorrPiece;
    const int64_t pad9 = ((int64_t)c.nv + 8) / 9 * 9, pad11 = ((int64_t)c.nv + 10) / 11 * 11;
    c.cv = pad11 < pad9 ? 11 : 9;                                              // the run that wastes fewer column shifts
    c.runs = (int)std::min<int64_t>(kCorrMaxRuns, ((int64_t)c.nv + c.cv - 1) / c.cv);
    c.rows_blk = std::min(64 / c.runs, c.nu);
    c.blocks_u = (c.nu + c.rows_blk - 1) / c.rows_blk;
    c.blocks_v = (c.nv + c.runs * c.cv - 1) / (c.runs * c.cv);
    c.lds_rows = kCorrPiece + c.rows_blk - 1;
    c.pitch = kCorrPiece + c.runs * c.cv;
    c.lds_bytes = kCorrRefBytes + c.lds_rows * c.pitch * 4;
    // (counts beyond 2^31 are refused by the entry point: saturated, not wrapped)
    const int64_t pieces = (int64_t)c.pieces_y * c.pieces_x, blocks = (int64_t)c.blocks_u * c.blocks_v, nunv = (int64_t)c.nu * c.nv;
    const bool huge = pieces > 0x7fffffffLL || blocks > 0x7fffffffLL || nunv > 0x7fffffffLL;
    c.unit_wgs = huge ? INT64_MAX : pieces * blocks;
    c.unit_part = pieces > 1 ? (huge ? INT64_MAX : pieces * nunv) : 0;
    return c;
}

namespace {

struct CorrArgs {
    const float* src; int64_t src_plane; int src_pitch;
    const float* refs; int64_t ref_plane; int ref_pitch;
    const CorrEntry* tab;
    double* out; double* part;
    int64_t q0;
    int H, W, gh, gw, rh, rw, nu, nv, pieces_y, pieces_x, runs, rows_blk, blocks_u, blocks_v, lds_rows, pitch;
};

template <int CV>
__global__ __launch_bounds__(256) void correlate_stack_kernel(const CorrArgs a)
{
    extern __shared__ __align__(16) float lds[];
    float* const ref = lds;                                   // [64][64]
    float* const img = lds + kCorrPiece * kCorrPiece;         // [lds_rows][pitch]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup-uniform decode: blocks fastest, then pieces, then units
    uint32_t b = blockIdx.x;
    const int bv = b % (uint32_t)a.blocks_v; b /= (uint32_t)a.blocks_v;
    const int bu = b % (uint32_t)a.blocks_u; b /= (uint32_t)a.blocks_u;
    const int px = b % (uint32_t)a.pieces_x; b /= (uint32_t)a.pieces_x;
    const int py = b % (uint32_t)a.pieces_y; b /= (uint32_t)a.pieces_y;
    const int ql = (int)b;
    const int64_t q = a.q0 + ql;
    const int per = a.gh * a.gw;                              // < 2^31 by the bound on the output
    const int ent = (int)(q / per), patch = (int)(q - (int64_t)ent * per);
    const int pa = patch / a.gw, pb = patch - pa * a.gw;
    const CorrEntry e = a.tab[ent];
    // the patch and the piece
    const int y0 = (int)((int64_t)pa * a.H / a.gh), y1 = (int)((int64_t)(pa + 1) * a.H / a.gh);
    const int x0 = (int)((int64_t)pb * a.W / a.gw), x1 = (int)((int64_t)(pb + 1) * a.W / a.gw);
    const int py0 = y0 + py * kCorrPiece, px0 = x0 + px * kCorrPiece;
    const int ph = std::min(kCorrPiece, y1 - py0), pw = std::min(kCorrPiece, x1 - px0);     // <= 0: the piece is past the patch
    const bool any = ph > 0 && pw > 0;
    const int u0 = bu * a.rows_blk, v0 = bv * a.runs * CV;    // the block's first shift

    if (any) {
        // the reference piece; what lies past its rows and columns is never read by an fma
        const float* __restrict__ rp = a.refs + (int64_t)e.ref * a.ref_plane;
        for (int y = tid >> 6; y < kCorrPiece; y += 4) {
            const int x = lane;
            float r = 0.0f;
            if (y < ph && x < pw) r = rp[(int64_t)(py0 + y) * a.ref_pitch + (px0 + x)];
            ref[y * kCorrPiece + x] = r;
        }
        // the image samples of the block: staged row yy is image row py0 + yy + u0 - rh, staged column xx image column px0 + xx + v0 - rw.
        // Loads are on clamped addresses; +0 is selected outside the image.
        const float* __restrict__ sp = a.src + (int64_t)e.plane * a.src_plane;
        const int rows = ph + a.rows_blk - 1, cols = kCorrPiece - 1 + a.runs * CV;
        const int64_t ys = (int64_t)py0 + u0 - a.rh, xs = (int64_t)px0 + v0 - a.rw;
        for (int xx = tid & 127; xx < cols; xx += 128) {      // cols <= 63 + 7 * 11
            const int64_t x = xs + xx;
            const bool xin = x >= 0 && x < a.W;
            const int xc = (int)(x < 0 ? 0 : (x >= a.W ? a.W - 1 : x));
            for (int yy = tid >> 7; yy < rows; yy += 2) {
                const int64_t y = ys + yy;
                const int yc = (int)(y < 0 ? 0 : (y >= a.H ? a.H - 1 : y));
                const float s = sp[(int64_t)yc * a.src_pitch + xc];
                img[yy * a.pitch + xx] = (xin && y >= 0 && y < a.H) ? s : 0.0f;
            }
        }
    }
    __syncthreads();

    const int ul = lane / a.runs, j = lane - ul * a.runs;
    const bool active = ul < a.rows_blk;                     // runs that do not divide 64 leave the last lanes idle
    double acc[CV];
#pragma unroll
    for (int o = 0; o < CV; ++o) acc[o] = 0.0;

    if (any) {
        const float* __restrict__ mine = img + (active ? ul : 0) * a.pitch + j * CV;
        const int yb = wave * kCorrBand, ye = std::min(yb + kCorrBand, ph);
        for (int y = yb; y < ye; ++y) {
            const float* __restrict__ row = mine + y * a.pitch;
            const float* __restrict__ rr = ref + y * kCorrPiece;
            for (int xg = 0; xg < pw; xg += kCorrGroup) {
                double win[CV + kCorrGroup - 1];
#pragma unroll
                for (int i = 0; i < CV + kCorrGroup - 1; ++i) win[i] = (double)row[xg + i];
                const float4 ra = *reinterpret_cast<const float4*>(rr + xg), rb = *reinterpret_cast<const float4*>(rr + xg + 4);
                const double r[kCorrGroup] = {(double)ra.x, (double)ra.y, (double)ra.z, (double)ra.w,
                                              (double)rb.x, (double)rb.y, (double)rb.z, (double)rb.w};
                if (xg + kCorrGroup <= pw) {
#pragma unroll
                    for (int d = 0; d < kCorrGroup; ++d)
#pragma unroll
                        for (int o = 0; o < CV; ++o) acc[o] = fma(r[d], win[o + d], acc[o]);
                } else {
#pragma unroll
                    for (int d = 0; d < kCorrGroup; ++d)
                        if (xg + d < pw) {                   // wave-uniform
#pragma unroll
                            for (int o = 0; o < CV; ++o) acc[o] = fma(r[d], win[o + d], acc[o]);
                        }
                }
            }
        }
    }
    __syncthreads();                                         // the band sums take the staged blocks' place

    double* const red = reinterpret_cast<double*>(lds);      // [4][CV][64]: 4 * 11 * 64 * 8 bytes at most, inside ref + 64 staged rows
#pragma unroll
    for (int o = 0; o < CV; ++o) red[(wave * CV + o) * 64 + lane] = acc[o];
    __syncthreads();
    if (wave != 0 || !active) return;
    const int u = u0 + ul;
    if (u >= a.nu) return;
    const int pieces = a.pieces_y * a.pieces_x;
    const int64_t nunv = (int64_t)a.nu * a.nv;
    double* __restrict__ dst = pieces == 1 ? a.out + q * nunv : a.part + ((int64_t)ql * pieces + (py * a.pieces_x + px)) * nunv;
    dst += (int64_t)u * a.nv;
#pragma unroll
    for (int o = 0; o < CV; ++o) {
        double t = red[o * 64 + lane];
        t += red[(CV + o) * 64 + lane];
        t += red[(2 * CV + o) * 64 + lane];
        t += red[(3 * CV + o) * 64 + lane];
        const int v = v0 + j * CV + o;
        if (v < a.nv) dst[v] = t;
    }
}

// out[(q0 + l) * nunv + s] = part[(l * pieces + 0) * nunv + s] + part[(l * pieces + 1) * nunv + s] + ..., ascending
__global__ __launch_bounds__(256) void correlate_stack_reduce(const double* __restrict__ part, double* __restrict__ out, const int64_t q0,
                                                              const int64_t total, const int64_t nunv, const int pieces)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= total) return;
    const int64_t l = t / nunv, s = t - l * nunv;
    const double* __restrict__ p = part + l * pieces * nunv + s;
    double sum = p[0];
    for (int k = 1; k < pieces; ++k) sum += p[(int64_t)k * nunv];
    out[(q0 + l) * nunv + s] = sum;
}

}  // namespace

hipError_t launch_correlate_stack(const float* src, int64_t src_plane, int src_pitch, const float* refs, int64_t ref_plane, int ref_pitch,
                                  const CorrEntry* d_tab, double* out, double* part, int64_t q0, int count, const CorrPlan& cp,
                                  hipStream_t stream)
{
    if (count <= 0 || q0 < 0 || !src || !refs || !d_tab || !out || (cp.unit_part > 0 && !part) || (cp.cv != 9 && cp.cv != 11) ||
        cp.runs < 1 || cp.runs > kCorrMaxRuns || cp.rows_blk < 1 || cp.rows_blk * cp.runs > 64 || cp.pitch != kCorrPiece + cp.runs * cp.cv ||
        cp.lds_rows != kCorrPiece + cp.rows_blk - 1 || cp.lds_bytes != kCorrRefBytes + cp.lds_rows * cp.pitch * 4 || cp.lds_bytes > 65536 ||
        cp.unit_wgs * count > 0x7fffffffLL)
        return hipErrorInvalidValue;
    CorrArgs a;
    a.src = src; a.src_plane = src_plane; a.src_pitch = src_pitch;
    a.refs = refs; a.ref_plane = ref_plane; a.ref_pitch = ref_pitch;
    a.tab = d_tab; a.out = out; a.part = part; a.q0 = q0;
    a.H = cp.H; a.W = cp.W; a.gh = cp.gh; a.gw = cp.gw; a.rh = cp.rh; a.rw = cp.rw; a.nu = cp.nu; a.nv = cp.nv;
    a.pieces_y = cp.pieces_y; a.pieces_x = cp.pieces_x; a.runs = cp.runs; a.rows_blk = cp.rows_blk;
    a.blocks_u = cp.blocks_u; a.blocks_v = cp.blocks_v; a.lds_rows = cp.lds_rows; a.pitch = cp.pitch;
    const dim3 grid((unsigned)(cp.unit_wgs * count)), block(256);
    if (cp.cv == 9) hipLaunchKernelGGL(correlate_stack_kernel<9>, grid, block, (size_t)cp.lds_bytes, stream, a);
    else hipLaunchKernelGGL(correlate_stack_kernel<11>, grid, block, (size_t)cp.lds_bytes, stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess || cp.unit_part == 0) return err;
    const int64_t nunv = (int64_t)cp.nu * cp.nv, total = nunv * count;
    hipLaunchKernelGGL(correlate_stack_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, part, out, q0, total, nunv,
                       cp.pieces_y * cp.pieces_x);
    return hipGetLastError();
}

}  // namespace vt
