// vt_kernels_momentsstack.hip -- the sum and the sum of squares of the samples under every patch of a grid at every shift of a window,
// for every image of a resident stack (kind 25), hand-written for gfx950 (MI355X, CDNA4): the two window sums that turn
// vt_volume_correlate_stack's raw scores into correlation coefficients.
//
// The handle holds T images of H x W as its planes.  For entry i with image p, patch (a, b) of the grid and shift (u, v) of the
// window (rh, rw)
//     out[i, a, b, u, v, 0] = sum over (y, x) of the patch of  (double) s(y + u - rh, x + v - rw)
//     out[i, a, b, u, v, 1] = the same sum of                  (double) s(..)^2
//     s(y', x') = S[p, y', x'] inside the image, +0 outside
// every square exact, every addition rounded, in this order:
//   * a row sum R[y', b, dv] belongs to image row y', patch column b and column displacement dv = v - rw.  It starts from +0 and takes
//     the samples s(y', x + dv) of the patch's columns x in ascending order: acc0 = acc0 + s, acc1 = fma(s, s, acc1);
//   * a value starts from +0 and takes the row sums R[y + u - rh, b, v - rw] of the patch's rows y in ascending order; a row outside
//     the image is +0.
// Nothing in it depends on the window, the grid beyond the patch's own rows and columns, or the batch.  The sums are separable, so the
// work is pixels x (2 rw + 1) additions and fmas, not pixels x shifts.
//
//   * moments_rows_kernel: one 256-thread workgroup per (entry, block of rows_wg image rows, patch column, block of runs * cv column
//     shifts): lane <-> (image row, run of cv consecutive column shifts), held as 2 cv float64 accumulators, cv = 9 or 11; a wave holds
//     64 / runs rows of runs runs.  Windows wider than a block go onto the grid.
//   * The workgroup walks its patch column in chunks of 32 pixels.  Per chunk it stages, for each of its rows, the 31 + runs * cv
//     samples the block reaches, at a pitch of 32 + runs * cv floats.  Zeros outside the image are written here, so the inner loop has
//     no bounds test.  The lane at (row rl, run j) of a wave reads lds[(rl) * pitch + x + j * cv + ..]: modulo the 32 banks of a dword
//     read that is cv * lane + const, and cv is odd, so the 32 lanes of a read group fall on 32 banks.
//   * A lane walks the chunk 8 pixels at a time: the cv + 7 samples its shifts reach under the 8 pixels are read and widened once into a
//     register window, and pixel d is cv additions and cv fmas on the window at the static offset d.  A pixel past the patch's last
//     column is skipped by a workgroup-uniform branch: nothing outside the patch reaches a sum.
//   * The row sums go to the partials, [entry of the launch][image row][patch column][column shift][2].  moments_sum_kernel, one thread
//     per output value, adds the rows of its patch in ascending order.  No atomics, no memset: every row sum and every value is stored
//     by exactly one thread.
#include "vt_internal.h"

#include <algorithm>
#include <cstdint>

namespace vt {

MomPlan moments_stack_plan(int H, int W, int gh, int gw, int rh, int rw)
{
    MomPlan m{};
    m.H = H; m.W = W; m.gh = gh; m.gw = gw; m.rh = rh; m.rw = rw;
    m.nu = 2 * rh + 1; m.nv = 2 * rw + 1;
    const int64_t pad9 = ((int64_t)m.nv + 8) / 9 * 9, pad11 = ((int64_t)m.nv + 10) / 11 * 11;
    m.cv = pad11 < pad9 ? 11 : 9;                                              // the run that wastes fewer column shifts
    m.runs = (int)std::min<int64_t>(kMomMaxRuns, ((int64_t)m.nv + m.cv - 1) / m.cv);
    m.rows_wave = 64 / m.runs;
    m.rows_wg = 4 * m.rows_wave;
    m.row_blocks = (H + m.rows_wg - 1) / m.rows_wg;
    m.blocks_v = (m.nv + m.runs * m.cv - 1) / (m.runs * m.cv);
    m.pitch = kMomChunk + m.runs * m.cv;
    m.lds_bytes = m.rows_wg * m.pitch * 4;
    m.unit_wgs = (int64_t)m.row_blocks * gw * m.blocks_v;                      // < 2^31 * 2^31 / 9: the entry point holds it below 2^31
    m.unit_part = (int64_t)H * gw * m.nv * 2;                                  // H gw < 2^31 by the bound on the output, nv < 2^31
    return m;
}

namespace {

constexpr int kMomStage = 8;                   // image rows a thread of the first launch loads before it stores them to LDS
constexpr int kMomSumBlock = 64;               // threads per workgroup of the second launch: small calls still reach every CU
constexpr int kMomRowsInFlight = 16;           // row sums a thread of the second launch loads before it adds them

struct MomArgs {
    const float* src; int64_t src_plane; int src_pitch;
    const MomEntry* tab;
    double* out; double* part;
    int64_t e0;
    int H, W, gh, gw, rh, rw, nu, nv, runs, rows_wave, rows_wg, row_blocks, blocks_v, pitch;
    int64_t unit_part;
};

template <int CV>
__global__ __launch_bounds__(256) void moments_rows_kernel(const MomArgs a)
{
    extern __shared__ __align__(16) float lds[];              // [rows_wg][pitch]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // workgroup-uniform decode: shift blocks fastest, then patch columns, then row blocks, then entries
    uint32_t g = blockIdx.x;
    const int bv = g % (uint32_t)a.blocks_v; g /= (uint32_t)a.blocks_v;
    const int pb = g % (uint32_t)a.gw; g /= (uint32_t)a.gw;
    const int rb = g % (uint32_t)a.row_blocks; g /= (uint32_t)a.row_blocks;
    const int el = (int)g;
    const MomEntry e = a.tab[a.e0 + el];
    const int x0 = (int)((int64_t)pb * a.W / a.gw), x1 = (int)((int64_t)(pb + 1) * a.W / a.gw);
    const int yb = rb * a.rows_wg;                            // the block's first image row
    const int v0 = bv * a.runs * CV;                          // the block's first column shift

    const int rl = lane / a.runs, j = lane - rl * a.runs;
    const bool active = rl < a.rows_wave;                     // runs that do not divide 64 leave the last lanes idle
    const int r = wave * a.rows_wave + (active ? rl : 0);     // the lane's staged row
    const float* __restrict__ mine = lds + r * a.pitch + j * CV;
    const float* __restrict__ sp = a.src + (int64_t)e.plane * a.src_plane;
    const int cols = kMomChunk - 1 + a.runs * CV;             // <= 31 + 7 * 11

    double acc0[CV], acc1[CV];
#pragma unroll
    for (int o = 0; o < CV; ++o) acc0[o] = acc1[o] = 0.0;

    for (int xc = x0; xc < x1; xc += kMomChunk) {
        if (xc != x0) __syncthreads();                        // the chunk before has been read
        // staged row yy is image row yb + yy, staged column xx image column xc + xx + v0 - rw.  Loads are on clamped addresses; +0 is
        // selected outside the image.
        const int64_t xs = (int64_t)xc + v0 - a.rw;
        {
            const int xx = tid & 127;
            if (xx < cols) {
                const int64_t x = xs + xx;
                const bool xin = x >= 0 && x < a.W;
                const int xcl = (int)(x < 0 ? 0 : (x >= a.W ? a.W - 1 : x));
                for (int yy0 = tid >> 7; yy0 < a.rows_wg; yy0 += 2 * kMomStage) {       // kMomStage loads in flight, then their stores
                    float s[kMomStage];
#pragma unroll
                    for (int k = 0; k < kMomStage; ++k) {
                        const int y = yb + yy0 + 2 * k;
                        s[k] = sp[(int64_t)(y >= a.H ? a.H - 1 : y) * a.src_pitch + xcl];
                    }
#pragma unroll
                    for (int k = 0; k < kMomStage; ++k) {
                        const int yy = yy0 + 2 * k;
                        if (yy < a.rows_wg) lds[yy * a.pitch + xx] = (xin && yb + yy < a.H) ? s[k] : 0.0f;
                    }
                }
            }
        }
        __syncthreads();
        const int pw = std::min(kMomChunk, x1 - xc);
        for (int xg = 0; xg < pw; xg += kMomGroup) {
            double win[CV + kMomGroup - 1];
#pragma unroll
            for (int i = 0; i < CV + kMomGroup - 1; ++i) win[i] = (double)mine[xg + i];
            if (xg + kMomGroup <= pw) {
#pragma unroll
                for (int d = 0; d < kMomGroup; ++d)
#pragma unroll
                    for (int o = 0; o < CV; ++o) {
                        acc0[o] = acc0[o] + win[o + d];
                        acc1[o] = fma(win[o + d], win[o + d], acc1[o]);
                    }
            } else {
#pragma unroll
                for (int d = 0; d < kMomGroup; ++d)
                    if (xg + d < pw) {                       // workgroup-uniform
#pragma unroll
                        for (int o = 0; o < CV; ++o) {
                            acc0[o] = acc0[o] + win[o + d];
                            acc1[o] = fma(win[o + d], win[o + d], acc1[o]);
                        }
                    }
            }
        }
    }

    const int y = yb + r;
    if (!active || y >= a.H) return;
    double* __restrict__ dst = a.part + (int64_t)el * a.unit_part + (((int64_t)y * a.gw + pb) * a.nv) * 2;
#pragma unroll
    for (int o = 0; o < CV; ++o) {
        const int v = v0 + j * CV + o;
        if (v < a.nv) *reinterpret_cast<double2*>(dst + (int64_t)v * 2) = make_double2(acc0[o], acc1[o]);
    }
}

// out[e0 + l, a, b, u, v, k] = the rows y + u - rh of R[l, ., b, v, k] over the rows y of patch a that land inside the image, ascending
__global__ __launch_bounds__(kMomSumBlock) void moments_sum_kernel(const MomArgs a, const int64_t total)
{
    const int64_t t = (int64_t)blockIdx.x * kMomSumBlock + threadIdx.x;
    if (t >= total) return;
    const int nv2 = a.nv * 2;                                 // < 2^31: nu * nv * 2 is below it
    int64_t q = t / nv2;
    const int vk = (int)(t - q * nv2);
    const int u = (int)(q % a.nu); q /= a.nu;
    const int pb = (int)(q % a.gw); q /= a.gw;
    const int pa = (int)(q % a.gh);
    const int64_t el = q / a.gh;
    const int y0 = (int)((int64_t)pa * a.H / a.gh), y1 = (int)((int64_t)(pa + 1) * a.H / a.gh);
    // image rows [ya, ye): the patch's rows displaced by u - rh, cut to the image
    const int ya = std::max(y0 + u - a.rh, 0), ye = std::min(y1 + u - a.rh, a.H);
    const int64_t step = (int64_t)a.gw * nv2;
    const double* __restrict__ p = a.part + el * a.unit_part + (int64_t)pb * nv2 + vk + (int64_t)ya * step;
    double sum = 0.0;
    int y = ya;
    for (; y + kMomRowsInFlight <= ye; y += kMomRowsInFlight, p += kMomRowsInFlight * step) {      // the loads first: they do not wait for the chain
        double w[kMomRowsInFlight];
#pragma unroll
        for (int i = 0; i < kMomRowsInFlight; ++i) w[i] = p[i * step];
#pragma unroll
        for (int i = 0; i < kMomRowsInFlight; ++i) sum += w[i];
    }
    for (; y < ye; ++y, p += step) sum += *p;
    a.out[a.e0 * ((int64_t)a.gh * a.gw * a.nu * nv2) + t] = sum;
}

}  // namespace

hipError_t launch_moments_stack(const float* src, int64_t src_plane, int src_pitch, const MomEntry* d_tab, double* out, double* part,
                                int64_t e0, int count, const MomPlan& mp, hipStream_t stream)
{
    const int64_t per_entry = (int64_t)mp.gh * mp.gw * mp.nu * mp.nv * 2;      // < 2^31 by the bound on the output
    if (count <= 0 || e0 < 0 || !src || !d_tab || !out || !part || (mp.cv != 9 && mp.cv != 11) || mp.runs < 1 || mp.runs > kMomMaxRuns ||
        mp.rows_wave != 64 / mp.runs || mp.rows_wg != 4 * mp.rows_wave || mp.pitch != kMomChunk + mp.runs * mp.cv ||
        mp.lds_bytes != mp.rows_wg * mp.pitch * 4 || mp.lds_bytes > 65536 || mp.row_blocks != (mp.H + mp.rows_wg - 1) / mp.rows_wg ||
        mp.unit_wgs != (int64_t)mp.row_blocks * mp.gw * mp.blocks_v || mp.unit_wgs * count > 0x7fffffffLL ||
        mp.unit_part != (int64_t)mp.H * mp.gw * mp.nv * 2 || per_entry * count > 0x7fffffffLL)
        return hipErrorInvalidValue;
    MomArgs a;
    a.src = src; a.src_plane = src_plane; a.src_pitch = src_pitch;
    a.tab = d_tab; a.out = out; a.part = part; a.e0 = e0;
    a.H = mp.H; a.W = mp.W; a.gh = mp.gh; a.gw = mp.gw; a.rh = mp.rh; a.rw = mp.rw; a.nu = mp.nu; a.nv = mp.nv;
    a.runs = mp.runs; a.rows_wave = mp.rows_wave; a.rows_wg = mp.rows_wg; a.row_blocks = mp.row_blocks; a.blocks_v = mp.blocks_v;
    a.pitch = mp.pitch; a.unit_part = mp.unit_part;
    const dim3 grid((unsigned)(mp.unit_wgs * count)), block(256);
    if (mp.cv == 9) hipLaunchKernelGGL(moments_rows_kernel<9>, grid, block, (size_t)mp.lds_bytes, stream, a);
    else hipLaunchKernelGGL(moments_rows_kernel<11>, grid, block, (size_t)mp.lds_bytes, stream, a);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return err;
    const int64_t total = per_entry * count;
    hipLaunchKernelGGL(moments_sum_kernel, dim3((unsigned)((total + kMomSumBlock - 1) / kMomSumBlock)), dim3(kMomSumBlock), 0, stream, a, total);
    return hipGetLastError();
}

}  // namespace vt
