// vt_internal.h -- shared declarations of the HIP library (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "../../include/voltools_hip.h"

namespace vt {

// Prefilter constants in float32, evaluated the way the reference's device code does
// (helper_math.h:1468 `Pole = sqrt(3.0f)-2.0f`; bspline.h:36 Lambda; bspline.h:27 anticausal gain).
constexpr float kPole   = -0x1.126148p-2f;   // -0.26794922
constexpr float kLambda =  0x1.7ffffep+2f;   //  5.9999995 = (1-Pole)*(1-1/Pole)
constexpr float kAntiInit = 0x1.b0cb1ap-3f;  //  0.21132489 = Pole/(Pole-1)

// Kernel argument block of the transform kernels.  Lives in the kernarg segment, i.e. it is read with
// scalar loads into SGPRs once per wave ("matrix broadcast from constant memory").
struct AffineParams {
    double m[12];      // 3x4 pull matrix in array-axis order; output-plane and slab offsets folded into m[r][3]
    double neg[3];     // sum_c min(0, m[r][c]*(T_c-1)): lowest source coordinate of a tile relative to its base
    double pos[3];     // sum_c max(0, m[r][c]*(T_c-1))
    double vlo[3];     // valid source interval [vlo, vhi) per axis: the skirt rule src+0.5 in [0, dim)
    double vhi[3];
    int32_t inc_hi[3];         // Q32.32 split of m[r][0]: per-step increment along the tile's depth axis
    uint32_t inc_lo[3];
    int32_t sD, sH, sW;        // resident source dims
    int32_t sP;                // row pitch of the resident source in floats (multiple of 4, pad columns are 0)
    int32_t oD, oH, oW;        // output dims
    int32_t nTd, nTh, nTw;     // output tile counts
    int32_t Lz, Ly, Lx;        // staged source box (floats); Lx is the LDS row stride
    int32_t flags;             // VT_KEEP_OUTSIDE
    int32_t zoff;              // axis-0-separable launches: src_z = d + zoff + fz
    float fz;
    int32_t dch;               // marching kernel: output planes per workgroup
    int32_t zero_off;          // byte offset, inside any source plane, of a 16-byte vector of zeros (row pad)
    int32_t slot_floats;       // marching kernel: floats per LDS plane slot (packed footprint, multiple of 4)
    int32_t sP2;               // plane-pair layout: floats per pair-row (2 * (roundup4(W) + 4))
    int32_t zero_off2;         // plane-pair layout: byte offset of a zero vector inside any pair-plane
    double ia1, ib1;           // marching kernels: march_recip(m[1][1]), march_recip(m[1][2])
    int32_t Lx_used;           // marching kernels, box mode: columns of a staged row that hold data (the rest of Lx is padding)
    int32_t ord[3];            // column order of the skirt test's fma chain (0,1,2; permuted when the launch runs on an axis-exchanged copy,
                               // so that the chain is the original problem's and boundary voxels classify as in affine_direct)
    int64_t ostride, orow;     // marching kernels: element stride between output planes / rows (oH*oW, oW unless axes are swapped)
    int blk_h, blk_w;          // marching kernels: blocked tile order inside a chunk layer (tiles per block; 0 = plain order)
    int32_t sPq;               // plane-quad layout: floats per quad-row (4 * positions per row)
    int32_t zero_off_q;        // plane-quad layout: byte offset of a zero vector inside any quad-plane
    uint32_t nTw_magic, nTh_magic;   // plane-quad kernel, 2-D grid: floor(2^32 / n) + 1 -- (u * magic) >> 32 == u / n for u * n < 2^32
    int32_t row_s;             // plane-quad kernel: bank-aware row starts, slot = column + row * row_s (mod 16); -1 = rows packed back to back
    int32_t dshift;            // plane-quad kernel: chunk c > 0 starts at output plane c*dch + dshift (0..3), chosen so that a chunk's first
                               // tap plane is the first plane of a quad (one quad step per chunk beyond its own planes instead of two)
    int32_t Lps;               // block kernel: LDS plane stride in floats (Ly * row stride + bank padding, multiple of 4)
    uint32_t psv_magic;        // block kernel: floor(2^32 / (Lps / 4)) + 1
    int32_t lds_cap;           // block kernel: bytes of LDS the box may take (the tile-queue word follows)
    int32_t binc_hi[5][3];     // block kernel: Q32.32 increments of the steps between a thread's eight voxels (+8 w, +8 h, -8 w, +4 d, -8 h),
    uint32_t binc_lo[5][3];    // [step kind][source axis]
    void* tplan;               // plane-quad kernel, KIND 4: per-tile staging plans shared by the chunk layers of a launch (nullptr = off)
    uint32_t tplan_epoch;      // ... and the launch's epoch: a plan granule counts only if it carries this value
};


// Columns [*mn, *mx] (box-relative) that the pixels of a TH x TW in-plane tile tap in box row Y, for the in-plane map
// sy = by + a1*j + b1*k, sx = bx + a2*j + b2*k.  A pixel taps the row iff sy lies in [Y-1-halo, Y+halo+1); over the
// continuous pixel rectangle that is a convex polygon and the extreme sx over it is attained at a vertex: a rectangle
// corner inside the strip, or a point where a strip line crosses a rectangle edge.  The result is a superset of the
// taps of the discrete pixels (widened by 1e-6).  Shared by the marching kernel (per workgroup) and the host planner
// (slot sizing), so both see the same spans.  Returns false when no pixel taps the row.
// ia1 / ib1: reciprocals of a1 / b1, 0 where the coefficient vanishes (march_recip; wave-uniform, computed on the host).
__host__ __device__ inline double march_recip(double a) { return (a > 1e-12 || a < -1e-12) ? 1.0 / a : 0.0; }

__host__ __device__ inline bool march_row_span(double a1, double b1, double a2, double b2, double ia1, double ib1,
                                               double by, double bx, int Y, int TH, int TW, int halo, int* mn, int* mx)
{
    const double ylo = (double)(Y - 1 - halo), yhi = (double)(Y + halo + 1);
    const double jm = (double)(TH - 1), km = (double)(TW - 1);
    double smin = 1e30, smax = -1e30;
    for (int cj = 0; cj < 2; ++cj)
        for (int ck = 0; ck < 2; ++ck) {
            const double j = cj ? jm : 0.0, k = ck ? km : 0.0;
            const double sy = by + a1 * j + b1 * k;
            if (sy >= ylo - 1e-6 && sy <= yhi + 1e-6) {
                const double sx = bx + a2 * j + b2 * k;
                smin = sx < smin ? sx : smin;
                smax = sx > smax ? sx : smax;
            }
        }
    for (int e = 0; e < 2; ++e) {
        const double L = e ? yhi : ylo;
        for (int c = 0; c < 2; ++c) {
            if (ib1 != 0.0) {                 // edges j = 0 and j = TH-1: solve for k
                const double j = c ? jm : 0.0;
                const double k = (L - by - a1 * j) * ib1;
                if (k >= 0.0 && k <= km) {
                    const double sx = bx + a2 * j + b2 * k;
                    smin = sx < smin ? sx : smin;
                    smax = sx > smax ? sx : smax;
                }
            }
            if (ia1 != 0.0) {                 // edges k = 0 and k = TW-1: solve for j
                const double k = c ? km : 0.0;
                const double j = (L - by - b1 * k) * ia1;
                if (j >= 0.0 && j <= jm) {
                    const double sx = bx + a2 * j + b2 * k;
                    smin = sx < smin ? sx : smin;
                    smax = sx > smax ? sx : smax;
                }
            }
        }
    }
    if (!(smin <= smax)) { *mn = 0; *mx = -1; return false; }
    *mn = (int)floor(smin - 1e-6) - halo;
    *mx = (int)floor(smax + 1e-6) + 1 + halo;
    return true;
}

// Geometry of a tile's source footprint for the packed general-matrix kernel: u' = A.p - neg is the position of tile
// voxel p inside the footprint's bounding box (before the sub-voxel offset of the tile is added).
struct PackGeom {
    double inv[9];     // A^-1 (rows: tile axes d,h,w; columns: source axes z,y,x)
    double cst[3];     // A^-1 . neg
    double ext[3];     // bounding-box extent of A.[0,T-1]^3 per source axis
    int32_t T[3];      // tile dims
    int32_t halo;      // 0 linear, 1 cubic
    int32_t Lxbox;     // bounding-box row length (floats) incl. alignment slack
    int32_t Lybox;
};

struct TilePlan {
    int kind;            // 1 direct, 2 tiled, 3 tiled axis-0-separable, 4 marching, 5 marching on plane pairs, 6 tiled with packed footprints,
                         // 7 reserved (vt_volume_info: fused projection), 8 marching on plane quads, 9 lane-block tiles (cfg = row-stride index),
                         // 10 source rows along w (maps that leave axis 2 alone); vt_volume_info also reports 11 (batched box extraction),
                         // 12 (batched projection), 13 (weighted sum of boxes) and 14 (per-box template scores), which are planned by their own entry points
    int cfg;             // index into the tile table
    int td, th, tw;
    int lds_bytes;
    int grid;
    int blocks_per_cu;
    PackGeom geo;       // kind 6 only
};

// Columns [*mn, *mx] (box-relative) that tile voxels can tap in box row (Z, Y), for EVERY sub-voxel position of a tile:
// box coordinate = b + u' with b_z, b_y in [halo, halo+1), b_x in [halo, halo+4) (16-byte alignment of the box origin).
// Row Z is tapped iff u'_z in (Z-2-2*halo, Z+1), same for Y.  Each pair of opposite faces of the tile bounds u'_x by an
// interval that is linear in (u'_z, u'_y); over the rectangle of admissible (u'_z, u'_y) the lower end of the feasible u'_x
// is >= max over faces of (min over the 4 corners), the upper end <= min over faces of (max over corners).
// Conservative (a superset of the taps), cheap (3 x 4 corner evaluations), identical on host and device.
__host__ __device__ inline bool packed_row_span(const PackGeom& g, int Z, int Y, int* mn, int* mx)
{
    const double zlo = (double)(Z - 2 - 2 * g.halo) - 1e-6, zhi = (double)(Z + 1) + 1e-6;
    const double ylo = (double)(Y - 2 - 2 * g.halo) - 1e-6, yhi = (double)(Y + 1) + 1e-6;
    // rows the footprint cannot reach at all
    if (zhi < 0.0 || zlo > g.ext[0] || yhi < 0.0 || ylo > g.ext[1]) { *mn = 0; *mx = -1; return false; }
    double LB = 0.0, UB = g.ext[2];
    for (int c = 0; c < 3; ++c) {
        const double gz = g.inv[3 * c], gy = g.inv[3 * c + 1], gx = g.inv[3 * c + 2];
        if (gx > -1e-9 && gx < 1e-9) continue;                  // this pair of faces does not bound x
        const double inv_gx = 1.0 / gx;
        const double top = (double)(g.T[c] - 1);
        double lo_min = 1e30, hi_max = -1e30;
        for (int k = 0; k < 4; ++k) {
            const double uz = (k & 1) ? zhi : zlo, uy = (k & 2) ? yhi : ylo;
            const double s = gz * uz + gy * uy + g.cst[c];
            const double xa = (0.0 - s) * inv_gx, xb = (top - s) * inv_gx;
            const double lo = xa < xb ? xa : xb, hi = xa < xb ? xb : xa;
            lo_min = lo < lo_min ? lo : lo_min;
            hi_max = hi > hi_max ? hi : hi_max;
        }
        LB = lo_min > LB ? lo_min : LB;
        UB = hi_max < UB ? hi_max : UB;
    }
    if (LB > UB + 1e-6) { *mn = 0; *mx = -1; return false; }
    int a = (int)floor(LB - 1e-6);                               // + b_x (>= halo) - halo taps
    int b = (int)floor(UB + 1e-6 + (double)g.halo + 4.0) + 1 + g.halo;
    if (a < 0) a = 0;
    if (b > g.Lxbox - 1) b = g.Lxbox - 1;
    *mn = a;
    *mx = b;
    return a <= b;
}

// Axis-0 projection (vt_kernels_project.hip): dst[y, x] = sum_z c_z * src[z, y, x]
struct ProjectParams {
    int32_t D, H;              // planes to sum, rows per plane
    int32_t nxv;               // column groups per row (VEC floats each)
    int32_t vec;               // 4: float4 per lane (pitches multiples of 4), 1: scalar
    int32_t src_pitch;         // floats per source row
    int32_t dst_pitch;         // floats per destination row
    int64_t dst_plane;         // floats between the `copies` destination planes
    int32_t copies;            // the sum is written `copies` times (3 planes of the helper volume)
    int32_t uniform;           // 1: c_z = 1
    int32_t zoff, halo, ntap;  // output plane d taps source planes d + zoff - halo + k, k < ntap, with weight wz[k]
    int32_t dlo, dhi;          // valid output planes (inclusive)
    float wz[4];
};
hipError_t launch_plane_sum(const float* src, float* dst, const ProjectParams& q, hipStream_t stream);

// launchers (vt_kernels_affine.hip)
int tile_config_count();
void tile_config(int idx, int* td, int* th, int* tw);
hipError_t launch_affine_tiled(int cfg, int interp, bool zsep, const float* src, float* out, const float* zeros16,
                               const AffineParams& p, int grid, int lds_bytes, hipStream_t stream);
hipError_t launch_affine_direct_batch(int interp, const float* src, float* out, const double* d_ms, int n,
                                      const AffineParams& p, hipStream_t stream);
int march_table_bytes();   // LDS bytes the packed-span set-up table needs (overlays the ring)
int march_config_count();
void march_config(int idx, int* th, int* tw, int* g, int* la, int* nt);
int zpair_config_count();
void zpair_config(int idx, int* th, int* tw, int* la, int* nt);
int march_blocks_per_cu(bool pair, int cfg, int interp, int lds_bytes);   // resident workgroups per CU (occupancy calculator, cached)
hipError_t launch_affine_zpair(int cfg, int interp, const float* src2, float* out, const AffineParams& p,
                               int grid, int lds_bytes, hipStream_t stream);
hipError_t launch_relayout_zpair(const float* src, float* dst, int D, int H, int W, int P, int P2, hipStream_t stream);
// dst[k][j][i] = src[i][j][k]; element strides: src i*ss0 + j*ss1 + k, dst k*ds0 + j*ds1 + i (vt_kernels_layout.hip)
hipError_t launch_transpose02(const float* src, float* dst, int n0, int n1, int n2, int64_t ss0, int64_t ss1,
                              int64_t ds0, int64_t ds1, hipStream_t stream);
hipError_t launch_mirror_pad(const float* src, float* dst, int D, int H, int W, int R, int P, hipStream_t stream);
hipError_t launch_relayout_swap01(const float* src, float* dst, int D, int H, int P, hipStream_t stream);
// plane-quad marching kernel (vt_kernels_quad.hip)
int quad_max_it();
int quad_config_count();
void quad_config(int idx, int* th, int* tw, int* nt);
int quad_tile_plan_granules(int cfg);   // 16-byte granules of one tile's shared staging plan (KIND 4)
int quad_tile_plan_lds(int cfg);        // LDS bytes a launch that shares plans needs at least
int quad_blocks_per_cu(int cfg, int interp, int lds_bytes, bool zid = false);
hipError_t init_quad_kernels();
hipError_t launch_relayout_zquad(const float* src, float* dst, int D, int H, int W, int P, int Pq, hipStream_t stream);
// vt_kernels_rows.hip (kind 10: maps that leave axis 2 alone)
hipError_t launch_relayout_xfir(const float* src, float* dst, int D, int H, int W, int P, bool simple, hipStream_t stream);
hipError_t init_rows_kernels();
void rows_tile(int* ph, int* run);
hipError_t launch_affine_rows(int interp, int pd, const float* src, float* out, const float* zeros16, const AffineParams& p, int lds_bytes, hipStream_t stream);
hipError_t launch_relayout_zquad_fir(const float* src, float* dst, int D, int H, int W, int P, int Pq, bool simple, hipStream_t stream);
// the same two forms of the in-plane transposed orientation, straight from the plain copy (no exchanged plain copy in between)
hipError_t launch_relayout_zquad_swap12(const float* src, float* dst, int D, int H, int W, int P, int Pq, bool fir, bool simple, hipStream_t stream);
hipError_t launch_affine_quad(int cfg, int interp, const float* srcq, float* out, const AffineParams& p,
                              int grid, int lds_bytes, hipStream_t stream);
// lane-block kernel for general matrices (vt_kernels_block.hip)
int block_rs_count();
int block_rs(int idx);
int block_rs_order(int th, const int** order);   // row-stride indices in the planner's order of preference for tile height th (16 or 8)
int block_max_vectors(int th);
void block_tile(int th, int* td, int* tw);
hipError_t init_block_kernels();
hipError_t launch_affine_block(int rs_idx, int th, int interp, const float* src, float* out, const float* zeros16, int* queue,
                               const AffineParams& p, const PackGeom& geo, int grid, int lds_bytes, hipStream_t stream);
int packed_config_count();
void packed_config(int idx, int* td, int* th, int* tw);
int packed_rows_max();
int packed_vectors_max();
hipError_t init_packed_kernels();
hipError_t launch_affine_packed(int cfg, int interp, const float* src, float* out, const float* zeros16, int* queue,
                                const AffineParams& p, const PackGeom& geo, int grid, int lds_bytes, hipStream_t stream);
// trilinear packed-span kernel of round 5 (vt_kernels_span.hip)
int span_config_count();
void span_config(int idx, int* td, int* th, int* tw);
int span_rows_max();
bool span_config_pipelined(int idx);      // two footprint buffers: LDS = table + 2 x capacity
int span_vectors_max();
hipError_t init_span_kernels();
hipError_t launch_affine_span(int cfg, const float* src, float* out, const float* zeros16, int* queue,
                              const AffineParams& p, const PackGeom& geo, int grid, int lds_bytes, hipStream_t stream);
int march_rows_max();
int march_max_it();
int interp_kind(int interp);
hipError_t init_march_kernels();
hipError_t launch_affine_march(int cfg, int interp, const float* src, float* out, const AffineParams& p,
                               int grid, int lds_bytes, hipStream_t stream);
hipError_t launch_affine_direct(int interp, const float* src, float* out, const AffineParams& p,
                                hipStream_t stream);
hipError_t init_affine_kernels();   // raises the dynamic-LDS limit of every tiled instantiation

// batched box extraction (vt_kernels_extract.hip, kind 11): one table entry per matrix, read by its workgroups with scalar loads
struct ExtractEntry {
    double m[12];              // 3x4 pull matrix, resident-window and edge offsets folded into m[r][3]
    double neg[3], pos[3];     // tile reach (set_tile_reach) for the launch's tile
    int32_t inc_hi[3];         // Q32.32 split of m[r][0]
    uint32_t inc_lo[3];
    int32_t Lz, Ly, Lx;        // this entry's staged box (floats); Lx is its LDS row stride
    int32_t tiled;             // 1: stage into LDS; 0: the footprint fits no LDS box, gather from global memory
    int32_t pad_[2];
};
static_assert(sizeof(ExtractEntry) == 192, "table entries are read with 16-byte scalar loads");
int extract_tile_count();
void extract_tile(int idx, int* td, int* th, int* tw);
int extract_pick_tile(bool cubic, const int box[3], int* wg_per_cu);     // a function of (box shape, interpolation) only
void extract_fill_entry(const double m[12], int cfg, bool cubic, int lds_cap, bool force_direct, ExtractEntry* e);
hipError_t init_extract_kernels();
hipError_t launch_extract(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                          const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream);

// a stack of axis-0 projections (vt_kernels_projbatch.hip, kind 12): extract_tiled's tiles and table entries, the samples of a pixel
// summed in float64 along the output depth instead of stored.  AffineParams: nTd = depth segments per image, dch = depth tiles per segment.
void project_batch_shape_plan(bool cubic, int depth, int height, int width, int* cfg, int* nseg, int* tiles_per_seg);   // (shape, interpolation) only
hipError_t init_projbatch_kernels();
hipError_t launch_project_tiled(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                                const ExtractEntry* d_tab, const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream);
hipError_t launch_project_reduce(const double* part, float* out, int nseg, int64_t plane, int images, hipStream_t stream);

// weighted sum of n extracted boxes (vt_kernels_extractsum.hip, kind 13): extract_tiled's tiles and table entries plus a table of n float64
// weights; a workgroup owns one box tile and one segment of consecutive matrices.  AffineParams: nTd / nTh / nTw = box tiles.  With nseg > 1
// the partials [segment][d][h][w] go through launch_project_reduce(part, out, nseg, box voxels, 1, stream).
void extract_sum_shape_plan(bool cubic, const int box[3], int n, int* cfg, int* nseg, int* per_seg);   // (n, box shape, interpolation) only
hipError_t init_extractsum_kernels();
hipError_t launch_extract_sum(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                              const ExtractEntry* d_tab, const double* d_wts, int n, int per_seg, int nseg, const AffineParams& p,
                              int lds_bytes, hipStream_t stream);

// per-box template scores (vt_kernels_extractdot.hip, kind 14): extract_tiled's tiles and table entries; a workgroup reduces the three sums
// of its (matrix, box tile) pair to one float64 triple in part[matrix][tile][3], a second kernel adds a box's tiles in ascending order
// into out[matrix][3].  d_mask == nullptr: a mask of ones.  lds_bytes >= extract_dot_min_lds() (the cross-wave scratch overlays the box).
int extract_dot_min_lds();
hipError_t init_extractdot_kernels();
hipError_t launch_extract_dot(int cfg, int interp, const float* src, double* out, double* part, const float* zeros16,
                              const ExtractEntry* d_tab, const float* d_tmpl, const float* d_mask, int cnt, const AffineParams& p,
                              int lds_bytes, hipStream_t stream);

// per-box scores against k templates (vt_kernels_extractdotmulti.hip, kind 15): launch_extract_dot's tiles, entries and LDS; d_tmpls holds k
// boxes back to back; part[matrix][tile][2 + k], out[matrix][2 + k].  Column 2 + j holds launch_extract_dot's bits for template j.
hipError_t init_extractdotmulti_kernels();
hipError_t launch_extract_dot_multi(int cfg, int interp, const float* src, double* out, double* part, const float* zeros16,
                                    const ExtractEntry* d_tab, const float* d_tmpls, const float* d_mask, int k, int cnt,
                                    const AffineParams& p, int lds_bytes, hipStream_t stream);

// g weighted sums of the same n extracted boxes (vt_kernels_extractsummulti.hip, kind 16): launch_extract_sum's tile, entries, segments and
// LDS; d_wts[i * g + j] for the gc columns of this launch (d_wts, out and part point at its first column); a workgroup owns a (segment,
// chunk of extract_sum_multi_chunk(cfg) columns, box tile) triple.  With nseg > 1 the partials [column][segment][d][h][w] go through
// launch_project_reduce(part, out, nseg, box voxels, gc, stream).  Box j holds launch_extract_sum's bits for column j.
int extract_sum_multi_chunk(int cfg);
hipError_t init_extractsummulti_kernels();
hipError_t launch_extract_sum_multi(int cfg, int interp, const float* src, float* out, double* part, const float* zeros16,
                                    const ExtractEntry* d_tab, const double* d_wts, int n, int per_seg, int nseg, int g, int gc,
                                    const AffineParams& p, int lds_bytes, hipStream_t stream);

// n posed, weighted copies of the resident map summed into one output (vt_kernels_place.hip, kind 17): launch_extract_sum's tile, entries and
// LDS with the output as "the box", one workgroup per NON-EMPTY output tile.  d_tile_ids: the n_tiles (> 0) tile ids that have a list;
// d_offs: n_tiles + 1 ascending offsets into d_idx; d_idx: entry indices, ascending per tile.  accumulate: sums start from `out` as found.
// Tiles without a list are not touched: the caller zeroes `out` first unless it accumulates.
hipError_t init_place_kernels();
hipError_t launch_place(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                        const double* d_wts, const int* d_tile_ids, const int* d_offs, const int* d_idx, int n_tiles, bool accumulate,
                        const AffineParams& p, int lds_bytes, hipStream_t stream);

// a stack of images back-projected into one volume (vt_kernels_backproject.hip, kind 18): launch_place's tile and entries, rows 1 and 2 of
// an entry's matrix map an output voxel into image (int)m[3] of the stack; one workgroup per output tile walks all n entries.  Two LDS
// buffers of buf_floats floats each (lds_bytes >= 8 * buf_floats, every tiled entry's Ly * Lx <= buf_floats); Lz is not read.
// accumulate: sums start from `out` as found, tiles no entry reaches are not written; otherwise every voxel is written.
hipError_t init_backproject_kernels();
hipError_t launch_backproject(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                              const double* d_wts, int n, int buf_floats, bool accumulate, const AffineParams& p, int lds_bytes,
                              hipStream_t stream);

// nb boxes of one shape back-projected from one stack in one launch (vt_kernels_backprojectboxes.hip, kind 19): kind 18's kernel with a box
// index, one workgroup per (box, box tile), grid = nb * tiles box-major.  d_tab: nb x n entries, d_wts: nb x n weights, out: nb boxes of
// p.oD x oH x oW, p.nTd / nTh / nTw the tiles of one box.  buf_floats: the largest staged patch of the batch (lds_bytes >= 8 * buf_floats).
hipError_t init_backproject_boxes_kernels();
hipError_t launch_backproject_boxes(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                                    const double* d_wts, int nb, int n, int buf_floats, bool accumulate, const AffineParams& p,
                                    int lds_bytes, hipStream_t stream);

// resampling through a displacement grid (vt_kernels_warp.hip, kind 20): s(v) = M.v + u(v), u the float64 trilinear interpolation of a
// (gD, gH, gW, 3) float32 control grid whose nodes span the output corner to corner.  One workgroup per output tile loads its nodes into
// LDS, bounds its source box by their range and stages that box, or gathers from global memory when its own box exceeds kWarpBoxCap.
constexpr int kWarpScratchFloats = 32;           // LDS in front of the node block: the cross-wave reduction of the node range
// Bytes of LDS a tile's staged box may take.  With the largest node block (17^3 nodes, 58956 bytes) and the scratch the launch stays
// below the 160 KiB a workgroup can have; boxes of ordinary fields (<= 48 KiB) leave room for three workgroups per CU.
constexpr int kWarpBoxCap = 96 * 1024;
// A tile bounds its source box by the hull of its nodes only while (largest |node component|) x (max_k g_k - 1) <= this (the header of
// vt_kernels_warp.hip derives the bound on what trilinear extrapolation by an ulp of f can add).
constexpr double kWarpHullLimit = 1048576.0;
struct WarpTable {
    ExtractEntry e;            // folded matrix and tile reach of the launch's tile; tiled = 0: every tile gathers from global memory
    double r[3];               // (g_k - 1) / (o_k - 1); 0 where g_k == 1
    double ext[3];             // affine extent of a tile per source axis: sum_k |m[r][k]| (T_k - 1)
    int32_t g[3];              // nodes per axis
    int32_t node_floats;       // floats of LDS between the scratch and the staged box (the largest node block, a multiple of 4)
    int32_t pad_[4];
};
static_assert(sizeof(WarpTable) == 272, "the grid follows the table 16-byte aligned");
// fills *wt and reports the dims of the largest staged box ((0, 0, 0): no tile stages) and the launch's dynamic LDS
void warp_plan(const double m[12], const float* grid, const int g[3], const int out_shape[3], int cfg, bool cubic, bool force_direct,
               WarpTable* wt, int L_max[3], int* lds_bytes);
hipError_t init_warp_kernels();
hipError_t launch_warp(int cfg, int interp, const float* src, float* out, const float* zeros16, const WarpTable* d_tab, const float* d_grid,
                       const AffineParams& p, int64_t grid, int lds_bytes, hipStream_t stream);

// every image of the stack under its own 2-D affine map (vt_kernels_stackaffine.hip, kind 21): one workgroup per (entry, 2-D output tile),
// grid = n x tiles entry-major; an entry's rows 1 and 2 map pixel (h, w) of output image i into image (int)m[3].  An entry stages ONE
// patch of Ly x Lx floats, or gathers from global memory when that patch exceeds kStackAffinePatchCap.
// Bytes of LDS a staged patch may take: five workgroups (20 waves) per CU by LDS at the cap.  The kernel has one buffer, so a workgroup
// waits for its own patch and the other workgroups of the CU are the overlap.
constexpr int kStackAffinePatchCap = 32 * 1024;
void stack_affine_tile(int idx, int* th, int* tw);
int stack_affine_pick_tile(bool cubic, int oh, int ow);                  // a function of (output image shape, interpolation) only
// rows: columns 0..3 of rows 1 and 2 of the caller's matrix (column 0 is not read)
void stack_affine_fill_entry(const double rows[8], int plane, int cfg, bool cubic, int oh, int ow, bool force_direct, ExtractEntry* e);
hipError_t launch_stack_affine(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                               const double* d_wts, int n, const AffineParams& p, int lds_bytes, hipStream_t stream);

// every image of the stack through its own 2-D displacement grid (vt_kernels_warpstack.hip, kind 22): kind 21's workgroups, tile and
// entries plus kind 20's grid rule on axes 1 and 2.  A workgroup loads the nodes its tile touches into LDS (behind kWarpScratchFloats),
// bounds its patch by their range and stages it, or gathers from global memory when the entry's flag is off, the hull is not granted
// (kWarpHullLimit) or its own patch exceeds kStackAffinePatchCap.
struct WarpStackHeader {
    double r[2];               // (g_k - 1) / (o_k - 1) on axes 1 and 2; 0 where g_k == 1
    int32_t g[2];              // nodes per axis
    int32_t n_grids;           // 1: one grid shared by every entry, else one per entry
    int32_t gm1_max;           // max(g) - 1
    int32_t node_floats;       // floats of LDS between the scratch and the patch (the largest node block, a multiple of 4)
    int32_t pad_[3];
};
static_assert(sizeof(WarpStackHeader) == 48, "the grids follow the header 16-byte aligned");
// what last_lds_dims reports when an entry's bound exceeds the cap and the allocation is the cap itself: 64 x 128 floats
constexpr int kWarpStackCapLy = 64, kWarpStackCapLx = 128;
static_assert(kWarpStackCapLy * kWarpStackCapLx * 4 == kStackAffinePatchCap, "the cap as a patch");
// the entry's flag (ExtractEntry::tiled) says only that its tiles MAY stage; rows as for stack_affine_fill_entry
void warp_stack_fill_entry(const double rows[8], int plane, int cfg, bool cubic, int oh, int ow, bool force_direct, ExtractEntry* e);
// folds the range of `nodes` nodes into r = (min y, max y, min x, max x); false: a component is not finite
bool warp_stack_grid_range(const float* q, size_t nodes, float r[4]);
// fills *hd and sizes the patch allocation from the grids' ranges (four floats per grid): L_alloc = (Ly, Lx), (0, 0) when no entry
// carries the flag
void warp_stack_plan(const ExtractEntry* e, int n, const float* ranges, int n_grids, const int g[2], int cfg, bool cubic, int oh, int ow,
                     WarpStackHeader* hd, int L_alloc[2], int* patch_bytes);
hipError_t launch_warp_stack(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                             const double* d_wts, const WarpStackHeader* d_hdr, const float* d_grids, int n, const AffineParams& p,
                             int lds_bytes, hipStream_t stream);

// kind 22's images summed under g weight columns without being written (vt_kernels_warpstacksum.hip, kind 26): one workgroup per (chunk of
// kWarpStackSumChunk consecutive columns, 2-D output tile) walks the n entries in ascending order with float64 accumulators in registers;
// tile, entries, header, node block and patch allocation are kind 22's (warp_stack_fill_entry, warp_stack_plan).  d_wts: n x g, C order.
// Dynamic LDS: one node block (shared grid) or three, then two patch allocations -- warp_stack_sum_lds_bytes.
// accumulate: sums start from `out` as found, tiles no entry reaches are not written; otherwise every pixel is written.
constexpr int kWarpStackSumChunk = 4;
hipError_t init_warp_stack_sum_kernels();
int warp_stack_sum_lds_bytes(const WarpStackHeader& hd, int patch_bytes);
hipError_t launch_warp_stack_sum(int cfg, int interp, const float* src, float* out, const float* zeros16, const ExtractEntry* d_tab,
                                 const double* d_wts, const WarpStackHeader* d_hdr, const float* d_grids, int n, int g, int patch_bytes,
                                 bool accumulate, const AffineParams& p, int lds_bytes, hipStream_t stream);

// a 1-D filter along axis 1 or 2 of every image of the stack (vt_kernels_filterstack.hip, kind 23): one workgroup per (entry, strip of
// kFilterStrip lines across the unfiltered axis, segment of kFilterSeg outputs along the filtered axis), grid = n x strips x segments
// entry-major.  The taps are walked kFilterChunk consecutive j at a time; per chunk the workgroup stages kFilterSeg + kFilterChunk - 1
// positions of its lines, (kFilterStrip + 1) floats apart.
constexpr int kFilterStrip = 64, kFilterSeg = 64, kFilterChunk = 128;
constexpr int64_t kFilterStackMaxTaps = (int64_t)1 << 26;    // n_taps x k of one call: at most 1.5 GiB of pairs and rows in the table buffer
constexpr int kFilterStackMaxExtent = 0x7fffffff - 256;       // the kernel's staged positions, extent + block, are 32-bit
constexpr int kFilterLdsBytes =(kFilterSeg + kFilterChunk - 1) * (kFilterStrip + 1) * 4;
struct FilterEntry {
    double weight;
    int64_t first;             // index of the entry's first FilterTap
    int64_t dense;             // index of tap 0 of the entry's row among the uploaded rows (k taps, then kFilterChunk zeros)
    int32_t plane;
    int32_t nnz;               // its non-zero taps
};
struct FilterTap {
    double t;
    int32_t j;                 // the tap's index in the caller's row, ascending within a row
    int32_t pad_;
};
static_assert(sizeof(FilterEntry) == 32 && sizeof(FilterTap) == 16, "tables of whole doubles, a tap per 16-byte scalar load");
inline int64_t filter_stack_strips(int lines) { return ((int64_t)lines + kFilterStrip - 1) / kFilterStrip; }
inline int64_t filter_stack_segments(int L) { return ((int64_t)L + kFilterSeg - 1) / kFilterSeg; }
hipError_t launch_filter_stack(const float* src, float* out, const FilterEntry* d_tab, const FilterTap* d_taps, const double* d_rows, int n,
                               int H, int W, int P, int axis, int pad, int k, hipStream_t stream);

// shift scores of every image of the stack against a reference, per patch of a grid (vt_kernels_correlatestack.hip, kind 24).  A patch
// is cut from its own origin into pieces of kCorrPiece x kCorrPiece pixels, the shift window into blocks of rows_blk shift rows x
// runs * cv shift columns; one workgroup per (entry, patch, piece, block), entry-major, blocks fastest.  Every patch of a call gets
// the piece grid of the largest patch; a piece past a smaller patch's end adds +0.
constexpr int kCorrPiece = 64;                 // piece edge: 4 bands of kCorrBand rows, one per wave
constexpr int kCorrBand = 16;
constexpr int kCorrGroup = 8;                  // reference pixels served by one register window
constexpr int kCorrMaxRuns = 7;                // runs of cv column shifts side by side in a wave
constexpr int kCorrRefBytes = kCorrPiece * kCorrPiece * 4;
struct CorrEntry {
    int32_t plane;             // the image
    int32_t ref;               // the reference: index among the uploaded references, or the resident image
};
static_assert(sizeof(CorrEntry) == 8, "one entry per double of the staging vector");
struct CorrPlan {
    int H, W, gh, gw, rh, rw, nu, nv;          // image, grid, window, shifts per axis (2 rh + 1, 2 rw + 1)
    int pieces_y, pieces_x;                    // pieces per patch
    int cv, runs, rows_blk;                    // a lane's run of column shifts (9 or 11), runs per shift row, shift rows per block
    int blocks_u, blocks_v;                    // blocks of the window
    int lds_rows, pitch;                       // staged image rows (kCorrPiece + rows_blk - 1) and the floats between them
    int lds_bytes;                             // kCorrRefBytes + lds_rows * pitch * 4
    int64_t unit_wgs;                          // workgroups per (entry, patch)
    int64_t unit_part;                         // float64 partials per (entry, patch): pieces * nu * nv, 0 with one piece
};
CorrPlan correlate_stack_plan(int H, int W, int gh, int gw, int rh, int rw);
// units [q0, q0 + count) of the call, unit q = entry q / (gh gw), patch q % (gh gw).  With one piece per patch the scores go to `out`,
// otherwise the partials of piece k of local unit l go to part[(l * pieces + k) * nu * nv ...] and a second launch adds them in
// ascending k into `out`.
hipError_t launch_correlate_stack(const float* src, int64_t src_plane, int src_pitch, const float* refs, int64_t ref_plane, int ref_pitch,
                                  const CorrEntry* d_tab, double* out, double* part, int64_t q0, int count, const CorrPlan& cp,
                                  hipStream_t stream);

// window sums of every image of the stack, per patch of a grid: the sum and the sum of squares of the samples under the patch at every
// shift (vt_kernels_momentsstack.hip, kind 25).  Two launches per run of entries: row sums R[entry, image row, patch column, column
// shift, 2] into the handle's partials, then every output as the ascending sum of its patch's rows of R.  The first launch has one
// workgroup per (entry, block of rows_wg image rows, patch column, block of runs * cv column shifts), entry-major, blocks fastest; a
// workgroup walks its patch column in chunks of kMomChunk pixels.
constexpr int kMomChunk = 32;                  // patch columns staged at a time
constexpr int kMomGroup = 8;                   // pixels served by one register window
constexpr int kMomMaxRuns = 7;                 // runs of cv column shifts side by side in a wave
struct MomEntry {
    int32_t plane;             // the image
    int32_t pad;
};
static_assert(sizeof(MomEntry) == 8, "one entry per double of the staging vector");
struct MomPlan {
    int H, W, gh, gw, rh, rw, nu, nv;          // image, grid, window, shifts per axis (2 rh + 1, 2 rw + 1)
    int cv, runs;                              // a lane's run of column shifts (9 or 11), runs per image row
    int rows_wave, rows_wg;                    // image rows per wave (64 / runs) and per workgroup (4 waves)
    int row_blocks, blocks_v;                  // blocks of image rows, blocks of column shifts
    int pitch;                                 // floats between staged rows: kMomChunk + runs * cv
    int lds_bytes;                             // rows_wg * pitch * 4
    int64_t unit_wgs;                          // workgroups of the first launch per entry: row_blocks * gw * blocks_v
    int64_t unit_part;                         // float64 row sums per entry: H * gw * nv * 2
};
MomPlan moments_stack_plan(int H, int W, int gh, int gw, int rh, int rw);
// entries [e0, e0 + count) of the call: the row sums of local entry l go to part[l * unit_part ...], the sums of entry e0 + l to
// out[(e0 + l) * gh * gw * nu * nv * 2 ...].
hipError_t launch_moments_stack(const float* src, int64_t src_plane, int src_pitch, const MomEntry* d_tab, double* out, double* part,
                                int64_t e0, int count, const MomPlan& mp, hipStream_t stream);

// prefilter (vt_kernels_prefilter.hip).  src -> dst; `*in_place_ok` tells whether src == dst is legal.
// axis: 0 (Z, stride H*W), 1 (Y, stride W), 2 (X, contiguous).
hipError_t launch_prefilter_axis(int axis, const float* src, float* dst, int D, int H, int W, int pitch,
                                 bool lo_interior, hipStream_t stream);
int prefilter_chunk_size(int N);                  // samples per chunk of the strided passes on lines of N samples
int prefilter_warmup();                           // samples of warm-up on each side of a chunk
hipError_t launch_prefilter_axis0_chunks(const float* src, float* dst, int D, int H, int W, int pitch, int c0, int c1, hipStream_t stream);
bool prefilter_axis_in_place_ok(int axis, int D, int H, int W);
bool prefilter_xy_ok(int D, int H, int W, int pitch, const void* src, const void* dst);
hipError_t launch_prefilter_xy(const float* src, float* dst, int D, int H, int W, int pitch, hipStream_t stream);

}  // namespace vt
