/*
 * voltools_hip.h -- C ABI of the MI355X (gfx950) 3-D affine-resampling engine.
 *
 * This is the drop-in boundary for the reference's Python -> device launch interface
 * (the-lay/voltools v0.6.0).  The reference has no FFI layer of its own: its host code reaches
 * the GPU through cupy (RawKernel launches, texture objects, cp.asarray / cp.zeros / .get()).
 * Every entry point below names the reference call site it stands in for (file:line into
 * /root/reference).  The library behind it is hand-written HIP; it links against libamdhip64 only
 * (no torch, no cupy), takes plain pointers and sizes, and never throws across the boundary:
 * every function returns 0 on success, otherwise a non-zero code (a hipError_t value, or one of
 * the VT_E* codes below) and leaves a message retrievable with vt_last_error().
 *
 * Conventions
 *   - Volumes are float32, C order, shape (D, H, W); axis 0 is slowest ("depth"), axis 2 fastest.
 *   - A transform is the reference's 4x4 float32 *pull* matrix in array-axis order
 *     (transforms.py:147-152, :265-274): src[d',h',w'] = M[:3,:3] . (d,h,w) + M[:3,3].  Only the
 *     first three rows are read.  The coordinate arithmetic is carried out in float64 from those
 *     float32 (or float64, *_f64 variants) entries.
 *   - Sampling semantics are the reference GPU path's: zero border, and an output voxel is
 *     "outside" when any src+0.5 < 0 or src+0.5 >= dim (transforms.py:276-278).  Outside voxels are
 *     written as 0 unless VT_KEEP_OUTSIDE is set (then they are left untouched, as the reference's
 *     kernel does; its callers pre-zero the buffer, transforms.py:208, volume.py:73).
 *   - Handles are opaque, owned by the library, and bound to one device and one HIP stream; calls
 *     on one handle are serialised on that stream.  Output buffers are owned by the caller.
 */
#ifndef VOLTOOLS_HIP_H
#define VOLTOOLS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* interpolation= strings of the reference (transforms.py:11-17), in that order */
enum vt_interp {
    VT_LINEAR = 0,               /* 'linear'              -> linearTex3D       (helper_interpolation.h:3-6)   */
    VT_BSPLINE = 1,              /* 'bspline'             -> cubicTex3D        (helper_interpolation.h:8-40)  */
    VT_BSPLINE_SIMPLE = 2,       /* 'bspline_simple'      -> cubicTex3DSimple  (helper_interpolation.h:42-68) */
    VT_FILT_BSPLINE = 3,         /* 'filt_bspline'        -> prefilter + cubicTex3D       (transforms.py:195-197) */
    VT_FILT_BSPLINE_SIMPLE = 4   /* 'filt_bspline_simple' -> prefilter + cubicTex3DSimple                        */
};

/* flags for the *_affine calls */
enum vt_flags {
    VT_OUT_DEVICE = 1,     /* `out` is a device pointer on the handle's device (else host memory)          */
    VT_KEEP_OUTSIDE = 2,   /* leave outside voxels untouched (reference kernel: `continue`, transforms.py:278) */
    VT_FORCE_DIRECT = 4,   /* diagnostic: use the untiled global-gather kernel                              */
    VT_FORCE_TILED = 8,    /* diagnostic: use the LDS-tiled kernel even for tiny volumes                    */
    VT_NO_ZSEP = 16,       /* diagnostic: disable the axis-0-separable kernels (use the general tiled kernel) */
    VT_NO_MARCH = 32,      /* diagnostic: axis-0-separable matrices use the 3-D tiled kernel, not the marching one */
    VT_NO_ZPAIR = 64,      /* diagnostic: cubic marching on the plain layout instead of the plane-pair copy          */
    VT_NO_PACKED = 128,    /* diagnostic: general matrices use bounding-box tiles, not packed footprints             */
    VT_FORCE_PACKED = 256, /* diagnostic: packed footprints whenever they fit, even where boxes are cheaper          */
    VT_FORCE_XSWAP = 512,  /* diagnostic: rotations about axis 2 take the axis-exchange path for every interpolation  */
    VT_NO_RSWAP = 1024,    /* diagnostic: in-plane maps near a quarter turn sample the plain copy, not the transposed */
    VT_ONESHOT_EDGE_SCIPY = 4096, /* vt_affine_oneshot only: build the temporary handle with VT_EDGE_SCIPY */
    VT_NO_QUAD = 2048,     /* diagnostic: no plane-quad marching kernel (the plain / plane-pair marching kernels serve instead);
                              VT_NO_ZPAIR disables both interleaved layouts */
    VT_NO_BLOCK = 8192,    /* diagnostic: general matrices use the bounding-box / packed-footprint kernels, not the lane-block
                              kernel (VT_NO_PACKED and VT_FORCE_PACKED imply it) */
    VT_NO_ZFIR = 16384,    /* diagnostic: cubic plane-quad launches with an integer axis-0 offset keep the four-tap-plane kernel
                              instead of sampling the z-convolved copy (also what a call falls back to when that copy does not fit) */
    VT_NO_REORIENT = 32768,/* diagnostic: general matrices always sample the plain resident copy, never an axis-permuted one */
    VT_NO_ROWS = 65536,    /* diagnostic: maps that leave axis 2 alone take the axis-exchange path, not the row kernel (kind 10) */
    VT_NO_PLANSHARE = 131072,/* diagnostic: the chunk layers of a cubic plane-quad launch on the z-convolved copy each build their
                              tile's staging plan instead of sharing one per tile (same results) */
    VT_ACCUMULATE = 262144,/* vt_volume_place and vt_volume_backproject only (vt_volume_backproject_boxes: per box): the sums start from
                              `out` as found instead of +0; voxels of tiles no copy (no image) can reach are neither read nor written */
    VT_PLACE_DENSE = 524288/* vt_volume_place only, diagnostic: every matrix is listed for every output tile (same results) */
};

/* flags for vt_volume_create* */
enum vt_create_flags {
    VT_SRC_DEVICE = 1,       /* `data` is a device pointer on `dev` (else host memory)                    */
    VT_SLAB_LO_INTERIOR = 2, /* slab volumes: plane 0 of `data` is NOT the global volume's first plane     */
    VT_SLAB_HI_INTERIOR = 4, /* slab volumes: the last plane of `data` is NOT the global volume's last     */
    VT_EDGE_SCIPY = 16,      /* boundary contract of the reference's CPU path (scipy.ndimage.affine_transform, mode='constant', cval=0,
                                transforms.py:147-152) instead of the GPU path's texture contract: hard cut-off outside [0, dim-1],
                                mirrored taps inside, mirror-boundary prefilter.  Whole-volume handles only.                 */
    VT_SRC_DEFERRED = 8,     /* `data` may be NULL: the resident window starts zero-filled, is filled plane range by plane
                                range with vt_volume_upload_planes and becomes usable with vt_volume_finalize              */
    VT_STACK = 32            /* the planes are independent images (a tilt series) for vt_volume_backproject: filt_* interpolations prefilter
                                along axes 2 and 1 only, and such a handle (in-plane coefficients) refuses every sampling entry
                                point but the back-projections, vt_volume_affine_stack and vt_volume_warp_stack with VT_EUNSUPPORTED.  With the other interpolations the flag changes nothing.  Not together with
                                VT_EDGE_SCIPY, a slab window or VT_SRC_DEFERRED (VT_EUNSUPPORTED).                          */
};

enum vt_error {
    VT_OK = 0,
    VT_EINVAL = 10001,       /* bad argument (NULL pointer, non-positive dims, unknown interpolation ...)  */
    VT_ENODEV = 10002,       /* device index out of range / no HIP device                                   */
    VT_ENOMEM = 10003,       /* host allocation failed                                                      */
    VT_EUNSUPPORTED = 10004  /* shape too large for this build's index arithmetic                           */
};

typedef struct vt_volume vt_volume_t;

typedef struct vt_volume_info {
    int32_t device;
    int32_t interp;
    int32_t depth, height, width;      /* source dims as passed to create (including any slab halo planes; the mirror padding of VT_EDGE_SCIPY handles is not counted) */
    int32_t out_depth, out_height, out_width;
    int32_t last_kernel;               /* 0 none, 1 direct, 2 tiled (boxes), 3 tiled axis-0-separable, 4 marching, 5 marching on plane pairs, 6 tiled (packed footprints), 7 fused projection (vt_volume_project), 8 marching on plane quads, 9 lane-block tiles (general matrices), 10 source rows along w (maps that leave axis 2 alone), 11 batched box extraction (LDS tiles; vt_volume_extract), 12 batched projection (LDS tiles summed along the output depth; vt_volume_project_batch), 13 weighted sum of extracted boxes (LDS tiles summed over the matrices; vt_volume_extract_sum), 14 per-box template scores (LDS tiles reduced within each box; vt_volume_extract_dot), 15 per-box scores against k templates (each box staged and sampled once; vt_volume_extract_dot_multi), 16 g weighted sums of the same extracted boxes (each box staged and sampled once per chunk of columns; vt_volume_extract_sum_multi), 17 posed weighted copies summed into one map (LDS tiles summed over each output tile's list of matrices; vt_volume_place), 18 a stack of images back-projected into one volume (2-D LDS patches, two buffers, summed over the images per output tile; vt_volume_backproject), 19 nb boxes of one shape back-projected from one stack (kernel 18 with a box index, one workgroup per (box, box tile); vt_volume_backproject_boxes), 20 resampling through a displacement grid (per output tile: its nodes in LDS, a staged box bounded by their range or a gather from global memory; vt_volume_warp), 21 per-image 2-D transforms of a stack (one workgroup per (entry, 2-D output tile), one LDS patch, one sample per pixel; vt_volume_affine_stack), 22 per-image displacement grids of a stack (kernel 21's workgroups; per tile its nodes in LDS, a patch bounded by their range or a gather from global memory; vt_volume_warp_stack), 23 a 1-D filter along axis 1 or 2 of every image of a stack (one workgroup per (entry, strip of lines, segment of the filtered axis), float64 sums over the non-zero taps; vt_volume_filter_stack), 24 shift scores of every image of a stack against a reference per patch of a grid (one workgroup per (entry, patch, piece of 64 x 64 pixels, block of shifts), float64 sums, pieces added by a second launch; vt_volume_correlate_stack), 25 the sum and the sum of squares of the samples under every patch of a grid at every shift, for every image of a stack (row sums per (entry, block of image rows, patch column, block of column shifts), then one thread per value adds its patch's rows; vt_volume_moments_stack), 26 the images of kind 22 summed under weight columns without being written (one workgroup per (chunk of columns, 2-D output tile) walks the entries with float64 accumulators; vt_volume_warp_stack_sum) */
    int32_t last_tile[3];              /* output tile (TD, TH, TW) of the last tiled launch (marching: G, TH, TW) */
    int32_t last_lds_dims[3];          /* staged source box (Lz, Ly, Lx) (marching: ring slots, Ly, Lx)    */
    int32_t last_lds_bytes;
    int32_t last_grid;
    float   prefilter_ms;              /* one-time prefilter time measured at create (filt_*), else 0      */
    uint64_t resident_bytes;           /* what the budget counts: the plain resident copy, the projection helper, every lazily built
                                          copy at the size of its allocation and the spare buffer kept for the next build */
    float   copies_ms;                 /* GPU time spent so far building lazy copies (relayouts; hip events on the handle's stream) */
    int32_t copies_built;              /* lazy copies built so far (rebuilt ones count again) */
    int32_t copies_evicted;            /* ... and released to stay inside the budget */
    uint64_t max_resident_bytes;       /* the handle's budget (vt_volume_set_max_resident), 0 = none */
} vt_volume_info_t;

/* ---- devices: replaces general.py:61-88 (cupy.cuda.runtime.getDeviceCount, Device(i).use()) ---- */
int vt_device_count(int* count);                         /* 0 devices is not an error                    */
int vt_device_name(int dev, char* buf, int buflen);
int vt_device_props(int dev, int* cu_count, int* lds_bytes_per_block, uint64_t* hbm_bytes);
int vt_device_synchronize(int dev);

/* ---- raw device memory: replaces cp.asarray / cp.zeros / ndarray.get (transforms.py:180,223; volume.py:30,73,89) ---- */
int vt_malloc(int dev, size_t bytes, void** dptr);
int vt_free(int dev, void* dptr);
int vt_memset_zero(int dev, void* dptr, size_t bytes);
int vt_memcpy_h2d(int dev, void* dptr, const void* hptr, size_t bytes);
int vt_memcpy_d2h(int dev, void* hptr, const void* dptr, size_t bytes);
int vt_memcpy_d2d(int dev, void* dst, const void* src, size_t bytes);
/* Pin a caller-owned host range for DMA at PCIe rate (the result-buffer pool of the Python layer keeps its buffers
 * registered; the reference's `.get()`, transforms.py:223, lands in freshly allocated pageable memory). */
int vt_host_register(int dev, void* ptr, size_t bytes);
int vt_host_unregister(int dev, void* ptr);
/* Release the device buffers the library keeps for recycling (resident sources and result staging of destroyed handles
 * and one-shot calls, at most 16 GiB per device; cupy's memory pool plays this role for the reference:
 * `cp.get_default_memory_pool().free_all_blocks()`). */
int vt_device_trim(int dev);

/* ---- StaticVolume: replaces volume.py:17-59 (upload, optional prefilter, texture build; done once) ----
 * `data` holds depth*height*width float32.  For filt_* interpolations the three-pass prefilter
 * (bspline.h:30-99, launched by transforms.py:290-309) runs here, once. */
int vt_volume_create(int dev, int depth, int height, int width, int interp,
                     const float* data, int create_flags, vt_volume_t** out);

/* Slab-partitioned volume (no reference counterpart: the reference is single-GPU).  `data` holds
 * local_depth planes that are planes [plane0, plane0+local_depth) of a global volume with
 * global_depth planes; output voxels are planes [out_plane0, out_plane0+out_depth) of the global
 * output.  Source planes outside the local window read as zero. */
int vt_volume_create_slab(int dev, int local_depth, int height, int width, int interp,
                          const float* data, int create_flags,
                          int64_t plane0, int64_t global_depth, int64_t out_plane0, int out_depth,
                          vt_volume_t** out);

/* Deferred construction (multi-GPU slabs: a rank's own planes and the halo planes it receives from its neighbours land in
 * the resident buffer directly, without assembling the window in a second device buffer first).  No reference counterpart.
 * `data`: nplanes * height * width float32 (host, or device with VT_SRC_DEVICE in `flags`) for resident planes
 * [first_plane, first_plane + nplanes).  vt_volume_finalize runs the one-time prefilter (filt_*) and enables the handle. */
int vt_volume_upload_planes(vt_volume_t* vol, int first_plane, int nplanes, const float* data, int flags);
int vt_volume_finalize(vt_volume_t* vol);

/* 1 when the library is the test build that also carries round 1's kernel families (plain / plane-pair marching, kernels 4 / 5, and
 * the axis-0-separable box kernel, 3): `make LEGACY=1`.  The product build returns 0; VT_NO_QUAD / VT_NO_ZPAIR / VT_NO_MARCH then
 * send an axis-0-separable matrix to the general-matrix kernels.  (No reference counterpart: diagnostic.) */
int vt_has_legacy_kernels(void);

/* Free the resident copies the handle built lazily besides its plain one -- per orientation used: the axis-exchanged plain copy, its
 * plane-quad form and the z-convolved plane-quad form, up to 4x the volume each way round (vt_volume_info.resident_bytes) -- e.g. between
 * the phases of a job that rotate about different axes, or before another handle needs the memory.  The next call that needs a copy
 * rebuilds it; results are unchanged.  freed_bytes may be NULL.  (No reference counterpart: the reference keeps one CUDA array per
 * StaticVolume, volume.py:37-45; cupy's pool serves `free_all_blocks()` for its temporaries.) */
int vt_volume_release_copies(vt_volume_t* vol, uint64_t* freed_bytes);
/* Resident-memory budget of the handle in bytes, the plain copy included (0 = none; default: VT_MAX_RESIDENT_GB or none).  Before a lazy
 * copy is built the least recently used ones are released until it fits; a copy that cannot fit is not built and the call runs on the
 * kernel family that samples the plain layout.  Results do not depend on the budget.  (No reference counterpart: the reference keeps
 * exactly one CUDA array per StaticVolume, volume.py:37-45.) */
int vt_volume_set_max_resident(vt_volume_t* vol, uint64_t bytes);
int vt_volume_destroy(vt_volume_t* vol);
int vt_volume_info(const vt_volume_t* vol, vt_volume_info_t* info);
int vt_volume_stream(const vt_volume_t* vol, void** hip_stream);   /* the hipStream_t launches go to */
int vt_volume_sync(vt_volume_t* vol);

/* Output shape other than the source shape (scipy's output_shape, transforms.py:136-150; reshape=True). */
int vt_volume_set_output_shape(vt_volume_t* vol, int out_depth, int out_height, int out_width);

/* ---- StaticVolume.affine: replaces volume.py:61-91 (matrix upload + one kernel launch) ----
 * m4x4: 16 float32, row-major (the reference's `xform`, transforms.py:204,255).  out: out_depth *
 * out_height * out_width float32.  With VT_OUT_DEVICE the call is asynchronous on the handle's
 * stream; with a host `out` it returns after the copy back (volume.py:89). */
int vt_volume_affine(vt_volume_t* vol, const float* m4x4, float* out, int flags);
int vt_volume_affine_f64(vt_volume_t* vol, const double* m4x4, float* out, int flags);

/* ---- a batch of matrices against one resident volume (the loop of README.md:25-27 / benchmark.py:52-54 in one call)
 * m4x4s: n x 16 float32; out: n consecutive output volumes.  Volumes up to 96^3 are served by ONE kernel launch
 * (launch latency, README.md:74, is paid once); larger ones are queued back to back on the handle's stream.
 * With a host `out` the call returns after the copy back; with VT_OUT_DEVICE it returns after the launch. */
int vt_volume_affine_batch(vt_volume_t* vol, int n, const float* m4x4s, float* out, int flags);

/* ---- batched sub-volume extraction: n boxes of one shape cut out of the resident volume, each at its own position and
 * orientation (sub-tomogram extraction, particle re-extraction, local template-matching windows).  Extends the reference's
 * CPU call site transforms.py:136-150 (scipy's `output_shape` argument of affine_transform) to the GPU and to a batch; the
 * reference's GPU path has no output shape other than the source's.
 * m4x4s: n x 16 pull matrices; box i is what vt_volume_affine would write for matrix i if the handle's output shape were
 * (box_d, box_h, box_w): src = M_i[:3,:3] . (d,h,w) + M_i[:3,3] with (d,h,w) the voxel index inside the box, the handle's
 * interpolation and boundary contract (VT_EDGE_SCIPY handles included).  out: n consecutive boxes; voxels outside the valid
 * interval are written as 0 (VT_KEEP_OUTSIDE is ignored).  Box i depends on M_i, the source and the box shape only, bit for
 * bit -- not on n, the other matrices or its place in the batch.  The handle's own output shape is neither read nor changed.
 * One launch serves every (matrix, box tile) pair (last_kernel 11); matrices whose tile footprint fits no LDS box gather
 * from global memory inside the same launch.  VT_FORCE_TILED / VT_FORCE_DIRECT select kernel 11 / the batched direct
 * kernel (last_kernel 1) whatever the box shape.  Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on
 * the handle's stream.  Slab handles and handles not yet finalized: VT_EINVAL; non-finite matrix entries: VT_EINVAL. */
int vt_volume_extract(vt_volume_t* vol, int n, const float* m4x4s,
                      int box_d, int box_h, int box_w, float* out, int flags);
int vt_volume_extract_f64(vt_volume_t* vol, int n, const double* m4x4s,
                          int box_d, int box_h, int box_w, float* out, int flags);

/* ---- weighted sum of n extracted boxes (sub-tomogram averaging; symmetrisation with the whole volume as the box) without writing them.
 * out: ONE box of box_d * box_h * box_w float32 (host, or device with VT_OUT_DEVICE):
 *     out[d, h, w] = float32(sum_i weights[i] * B_i[d, h, w])
 * with B_i the float32 box vt_volume_extract writes for matrix i (the handle's interpolation and boundary contract, VT_EDGE_SCIPY handles
 * included; voxels that map outside are 0).  weights: n float64, or NULL for all 1.  Each sample is widened to float64, multiplied by its
 * weight (rounded) and added (rounded) to a float64 accumulator, in ascending i within a segment of consecutive matrices; the segments'
 * sums are added in ascending order and the result is rounded to float32 once.  A voxel no box reaches is +0.
 * The fused kernel (last_kernel 13) gives one workgroup a box tile and a segment and loops over the segment's matrices; last_grid = box
 * tiles x segments, last_tile / last_lds_dims / last_lds_bytes as for vt_volume_extract.  The segmentation follows from (n, box shape,
 * interpolation) alone and the tile is vt_volume_extract's, so the result is a fixed expression of (matrices in their order, weights,
 * source, box shape, interpolation, route): repeated calls, host and device output and whatever the handle did before give identical bits,
 * and for n = 1 with weight 1 the result is vt_volume_extract's box bit for bit (up to the sign of a zero) on its default and
 * VT_FORCE_TILED routes.  Matrices whose tile footprint fits no LDS box gather from global memory inside the same launch; VT_FORCE_DIRECT
 * makes every matrix do so; VT_FORCE_TILED selects the same kernel as the default; VT_KEEP_OUTSIDE is ignored.  Device memory beyond the
 * source: n x 200 bytes of tables and, with more than one segment, float64 partials of segments x box voxels (tiles x segments < 2048:
 * under 64 MiB), in a buffer the handle recycles.  The handle's own output shape is neither read nor changed.
 * Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  Slab handles and handles not yet
 * finalized: VT_EINVAL; n <= 0, non-positive box dims, non-finite matrix entries or weights: VT_EINVAL. */
int vt_volume_extract_sum(vt_volume_t* vol, int n, const float* m4x4s, const double* weights /* n, or NULL = all 1 */,
                          int box_d, int box_h, int box_w, float* out, int flags);
int vt_volume_extract_sum_f64(vt_volume_t* vol, int n, const double* m4x4s, const double* weights /* n, or NULL = all 1 */,
                              int box_d, int box_h, int box_w, float* out, int flags);

/* ---- per-box template scores: three float64 sums over each of n boxes, without writing the boxes ----
 * out[i] = (sum_v mask[v] * B_i[v], sum_v mask[v] * B_i[v]^2, sum_v tmpl[v] * B_i[v]), where B_i is the float32 box vt_volume_extract
 * writes for matrix i (the handle's interpolation and boundary contract, VT_EDGE_SCIPY handles included; voxels that map outside are 0)
 * and v runs over all box voxels: what scoring n candidate (position, orientation) pairs against one template needs.  tmpl, mask: host
 * float32 arrays of the box shape in C order, uploaded on every call into a buffer the handle recycles; mask NULL = all 1.
 * out: n x 3 float64 (host, or device with VT_OUT_DEVICE).  Each sample is widened to float64; mask * b and tmpl * b are exact,
 * (mask * b) * b is rounded once, every addition is rounded.  A thread of the fused kernel (last_kernel 14) adds its own voxels in a fixed
 * order, a workgroup reduces its 256 partial triples by a tree of fixed shape, and the tiles of a box are added in ascending tile index by
 * a second small kernel; there are no atomics.  One workgroup serves one (matrix, box tile) pair with vt_volume_extract's tile, stepping
 * and routing, so the samples are vt_volume_extract's bit for bit and out[i] is a fixed expression of (M_i, tmpl, mask, source, box
 * shape, interpolation, route): it does not depend on n, on the other matrices or on its place in the batch, and repeated calls, host or
 * device output and whatever the handle did before leave the bits unchanged.  Matrices whose tile footprint fits no LDS box gather from
 * global memory inside the same launch; VT_FORCE_DIRECT forces every entry onto that gather, VT_FORCE_TILED is the default route.
 * The partials (n x box tiles x 3 float64) live in a buffer the handle recycles; a call whose partials would exceed 64 MiB is split
 * into several launches.  last_tile / last_lds_dims / last_lds_bytes as for vt_volume_extract, last_grid = box tiles x matrices of the
 * last launch.  The handle's own output shape is neither read nor changed; VT_KEEP_OUTSIDE is ignored.
 * Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  Slab handles and handles not yet
 * finalized: VT_EINVAL; n <= 0, NULL tmpl or out, non-positive box dims, non-finite matrix, template or mask entries: VT_EINVAL. */
int vt_volume_extract_dot(vt_volume_t* vol, int n, const float* m4x4s, const float* tmpl, const float* mask /* or NULL = all 1 */,
                          int box_d, int box_h, int box_w, double* out /* n x 3 */, int flags);
int vt_volume_extract_dot_f64(vt_volume_t* vol, int n, const double* m4x4s, const float* tmpl, const float* mask /* or NULL = all 1 */,
                              int box_d, int box_h, int box_w, double* out /* n x 3 */, int flags);

/* ---- per-box scores against k templates: 2 + k float64 sums over each of n boxes, each box staged and sampled once ----
 * out[i] = (sum_v mask[v] * B_i[v], sum_v mask[v] * B_i[v]^2, sum_v tmpls[0][v] * B_i[v], .., sum_v tmpls[k-1][v] * B_i[v]) with B_i as
 * for vt_volume_extract_dot: what classifying n candidate poses against k references under one mask needs.  tmpls: k host float32 boxes
 * of the box shape back to back in C order; mask: one such box, or NULL = all 1; both are uploaded on every call into a buffer the
 * handle recycles.  out: n x (2 + k) float64 (host, or device with VT_OUT_DEVICE).
 * Bit identity: for every j, columns 0, 1 and 2 + j hold exactly the bits vt_volume_extract_dot(vol, n, m4x4s, tmpls[j], mask, ..., flags)
 * writes into its columns 0, 1, 2 -- on the default route, with VT_FORCE_TILED, with VT_FORCE_DIRECT, for entries that gather from global
 * memory inside the tiled launch, on VT_EDGE_SCIPY handles and with a NULL mask.  The fused kernel (last_kernel 15 for every k, k = 1
 * included) keeps vt_volume_extract_dot's roundings (exact products, (mask * b) * b rounded once, every addition rounded) and order (a
 * thread's voxels in a fixed order, the tree of fixed shape over the 256 threads, the tiles of a box in ascending index by a second small
 * kernel; no atomics), but stages each (matrix, box tile) and samples each (matrix, voxel) once, whatever k is: a thread holds the samples
 * of its 4, 8 or 16 voxels in registers and accumulates the template sums three columns at a time.  A column is a fixed expression of
 * (M_i, that template, mask, source, box shape, interpolation, route): it does not depend on n, on k, on the other templates, on the
 * template's place in the stack, on the other matrices, on earlier calls or on host versus device output.  A box wholly outside gives a
 * row of exact +0.
 * The partials (box tiles x (2 + k) float64 per matrix) live in a buffer the handle recycles; a call whose partials would exceed 64 MiB
 * is split into launches of at least one matrix each.  last_tile / last_lds_dims / last_lds_bytes as for vt_volume_extract, last_grid =
 * box tiles x matrices of the last launch.  The handle's own output shape is neither read nor changed; VT_KEEP_OUTSIDE is ignored.
 * Bounds: a box as for vt_volume_extract_dot ((box_d + 16) x box_h x box_w < 2^31: a voxel offset within one template has 32 bits;
 * template j is addressed by a 64-bit base, so k x box voxels may exceed 2^31), and box tiles x (2 + k) < 2^31; beyond them
 * VT_EUNSUPPORTED.  Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  Slab handles and
 * handles not yet finalized: VT_EINVAL; k <= 0, n <= 0, NULL tmpls or out, non-positive box dims, non-finite matrix, template or mask
 * entries: VT_EINVAL.  A refusal leaves the handle usable. */
int vt_volume_extract_dot_multi(vt_volume_t* vol, int n, const float* m4x4s, int k, const float* tmpls /* k boxes, C order */,
                                const float* mask /* or NULL = all 1 */, int box_d, int box_h, int box_w,
                                double* out /* n x (2 + k) */, int flags);
int vt_volume_extract_dot_multi_f64(vt_volume_t* vol, int n, const double* m4x4s, int k, const float* tmpls /* k boxes, C order */,
                                    const float* mask /* or NULL = all 1 */, int box_d, int box_h, int box_w,
                                    double* out /* n x (2 + k) */, int flags);

/* ---- g weighted sums of the same n extracted boxes, each box sampled once (class averages, half-set maps, bootstrap replicas) ----
 * out: g boxes of box_d * box_h * box_w float32 back to back (host, or device with VT_OUT_DEVICE):
 *     out[j][d, h, w] = float32(sum_i weights[i * g + j] * B_i[d, h, w])
 * with B_i the float32 box vt_volume_extract writes for matrix i.  weights: n x g float64 in C order, required (there is no NULL form).
 * Bit identity: for every j, box j holds exactly the bits vt_volume_extract_sum(vol, n, m4x4s, column j of weights, ..., flags) writes --
 * on the default route, with VT_FORCE_TILED, with VT_FORCE_DIRECT, for entries that gather from global memory inside the tiled launch and
 * on VT_EDGE_SCIPY handles -- provided every sample is finite: a matrix whose weights are all exactly 0 in a workgroup's share of the
 * columns is passed over without being sampled, where vt_volume_extract_sum would add 0 x NaN for a non-finite sample.  A column is
 * therefore a fixed expression of (matrices in their order, that column, source, box shape, interpolation, route): it does not depend on
 * g, on the other columns, on the column's place in the matrix, on earlier calls or on host versus device output.
 * The fused kernel (last_kernel 16 for every g, g = 1 included) keeps vt_volume_extract_sum's tile, segments of consecutive matrices,
 * stepping, inside tests and per-sample expression; one workgroup serves a (segment, chunk of 2 / 4 / 8 consecutive columns for the
 * 16^3 / 8x16x16 / 8x8x16 tile, box tile) triple, holds the samples of its threads' voxels in registers and adds each into the chunk's
 * float64 accumulators.  No atomics.  last_tile / last_lds_dims / last_lds_bytes as for vt_volume_extract_sum; last_grid = workgroups of
 * the last launch (box tiles x segments x column chunks of that launch).
 * Device memory beyond the source: n x (192 + 8 g) bytes of tables and, with more than one segment, float64 partials of g x segments x box
 * voxels in a buffer the handle recycles; a call whose partials would exceed 64 MiB is split into launches of whole column chunks (at
 * least one), each followed by its reduction; the split does not show in the result.  The handle's own output shape is neither read nor
 * changed; VT_KEEP_OUTSIDE is ignored.
 * Bounds: the box as for vt_volume_extract_sum, and box tiles x segments x column chunks of a launch < 2^31; beyond them VT_EUNSUPPORTED.
 * Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  Slab handles and handles not yet
 * finalized: VT_EINVAL; n <= 0, g <= 0, NULL weights, non-positive box dims, non-finite matrix entries or weights: VT_EINVAL.  A refusal
 * leaves the handle usable. */
int vt_volume_extract_sum_multi(vt_volume_t* vol, int n, const float* m4x4s, int g, const double* weights /* n x g, C order */,
                                int box_d, int box_h, int box_w, float* out /* g boxes, C order */, int flags);
int vt_volume_extract_sum_multi_f64(vt_volume_t* vol, int n, const double* m4x4s, int g, const double* weights /* n x g, C order */,
                                    int box_d, int box_h, int box_w, float* out /* g boxes, C order */, int flags);

/* ---- n posed, weighted copies of the resident map summed into one (usually much larger) map: "place-back" model tomograms from refined
 * poses, synthetic tomograms, and, with negative weights and VT_ACCUMULATE, subtraction of picked particles from a tomogram.  The handle
 * holds the small map T (any shape, any interpolation, VT_EDGE_SCIPY handles included).  m4x4s: n x 16 pull matrices, output voxel index ->
 * T coordinate, s = P_i[:3,:3] . (d,h,w) + P_i[:3,3].  out: out_d * out_h * out_w float32 (host, or device with VT_OUT_DEVICE):
 *     out[v] = float32(b[v] + w_0 * A_0[v] + w_1 * A_1[v] + ...)        ascending i, only the i listed for the tile of v
 * with A_i the float32 volume vt_volume_affine would write for P_i at that output shape (the handle's interpolation and boundary contract,
 * 0 outside).  weights: n float64, or NULL for all 1.  Each term is widened to float64, multiplied by its float64 weight and added
 * to a float64 accumulator by vt_volume_extract_sum's accumulation step (the same function text compiled with the same options, so the
 * same instructions); the sum is rounded to float32 once.  b[v] is +0, or with VT_ACCUMULATE double(out[v]) as found.
 * The output is cut into the tiles vt_volume_extract_sum uses for a box of that shape; the host lists for every tile the matrices whose
 * copy can reach it (a superset of those that do: the kernel still tests each listed one, so an over-listed matrix adds nothing) and ONE
 * workgroup per non-empty tile (last_kernel 17) walks its list in ascending i.  A voxel whose tile has an empty list is +0 by default (one
 * memset of the output precedes the launch); with VT_ACCUMULATE it is neither read nor written -- NaN, -0 and everything else keep their
 * bits.  No segments, no atomics: the expression does not depend on n, on the binning or on what the handle did before.
 * Identity: wherever vt_volume_extract_sum(vol, n, m4x4s, weights, out_d, out_h, out_w, out, flags) runs one segment (1024 tiles or more)
 * this call without VT_ACCUMULATE writes the same bits, up to the sign of a zero.  VT_PLACE_DENSE lists every matrix for every tile
 * (same bits); VT_FORCE_DIRECT makes every matrix gather from global memory inside the same kernel, as matrices whose tile footprint fits
 * no LDS box always do; VT_FORCE_TILED selects the same kernel as the default; VT_KEEP_OUTSIDE is ignored.
 * last_grid = non-empty tiles launched (0: no kernel ran); last_tile / last_lds_dims / last_lds_bytes as for vt_volume_extract_sum.
 * Device memory beyond the source: n x 200 bytes of tables, 8 bytes per non-empty tile and 4 bytes per list entry, in a buffer the
 * handle recycles.  Output tiles and the total list length must stay below 2^31: VT_EUNSUPPORTED beyond.
 * Host `out`: returns after the copy back (with VT_ACCUMULATE the caller's array is uploaded first); VT_OUT_DEVICE: asynchronous on the
 * handle's stream.  Slab handles and handles not yet finalized: VT_EINVAL; n <= 0, non-positive dims, non-finite matrix entries or
 * weights: VT_EINVAL. */
int vt_volume_place(vt_volume_t* vol, int n, const float* m4x4s, const double* weights /* n, or NULL = all 1 */,
                    int out_d, int out_h, int out_w, float* out, int flags);
int vt_volume_place_f64(vt_volume_t* vol, int n, const double* m4x4s, const double* weights /* n, or NULL = all 1 */,
                        int out_d, int out_h, int out_w, float* out, int flags);

/* ---- back-projection: a stack of images (a tilt series) summed into one volume, the transpose of vt_volume_project_batch: weighted
 * back-projection of a filtered series, the second half of a SIRT step, sub-tomograms straight from a resident series.  The handle holds
 * the stack S as its (depth, height, width) = (T, H, W).  m4x4s: n x 16 pull matrices, output voxel index -> image coordinate,
 * y = M_i[1,:3] . (d,h,w) + M_i[1,3], x = M_i[2,:3] . (d,h,w) + M_i[2,3]; rows 0 and 3 are ignored.  planes: n image indices inside [0, T),
 * or NULL for planes[i] = i (then n must equal T).  out: out_depth * out_height * out_width float32 (host, or device with VT_OUT_DEVICE):
 *     out[v] = float32(b[v] + w_0 * B_0[v] + w_1 * B_1[v] + ...)        ascending i
 * with B_i[v] the float32 value of the handle's interpolation taken in TWO dimensions in image planes[i] at (y, x): bilinear, or the 4 x 4
 * cubic B-spline with the weights of the handle's 3-D kind; taps outside the image read 0; B_i[v] counts only where -0.5 <= y < H - 0.5 and
 * -0.5 <= x < W - 0.5, evaluated by the float64 fma chain of every other entry point.  weights: n float64, or NULL for all 1.  Each term is
 * widened to float64, multiplied by its weight and added by vt_volume_place's accumulation step; the sum is rounded to float32 once.  b[v]
 * is +0, or with VT_ACCUMULATE double(out[v]) as found.  Repeated calls give identical bits.
 * filt_* interpolations need coefficients that were prefiltered in-plane only: a handle created with VT_STACK; without it the call is
 * refused with VT_EUNSUPPORTED, as it is on VT_EDGE_SCIPY handles.
 * ONE workgroup per output tile (vt_volume_place's tile for that output shape; last_kernel 18, last_grid = output tiles) walks all n
 * entries, skips those whose tile maps outside the image, stages ONE image patch per entry into one of two LDS buffers -- the next
 * entry's patch is in flight while the current one is sampled -- and adds; no lists, no memset, no atomics.  With VT_ACCUMULATE a tile no
 * entry reaches is neither read nor written.  Identity: with a linear handle, vt_volume_place with the matrices whose row 0 is
 * (0, 0, 0, planes[i]) writes the same bits (up to the sign of a zero sample), with twice the staged bytes and taps.
 * last_tile = the tile, last_lds_dims = (2, Ly, Lx) of the largest staged patch, last_lds_bytes = the launch's allocation (two buffers).
 * Entries of which two patches do not fit the LDS gather from global memory inside the same launch; VT_FORCE_DIRECT makes every entry do
 * so, VT_FORCE_TILED selects the default.  Every other flag is ignored.  Device memory beyond the source: n x 200 bytes of tables.
 * Host `out`: returns after the copy back (with VT_ACCUMULATE the caller's array is uploaded first); VT_OUT_DEVICE: asynchronous on the
 * handle's stream.  Slab handles and handles not yet finalized: VT_EINVAL; n <= 0, non-positive dims, non-finite matrix entries or
 * weights, a plane index outside [0, T), planes == NULL with n != T: VT_EINVAL. */
int vt_volume_backproject(vt_volume_t* vol, int n, const float* m4x4s, const int32_t* planes /* n, or NULL */,
                          const double* weights /* n, or NULL = all 1 */, int out_depth, int out_height, int out_width,
                          float* out, int flags);
int vt_volume_backproject_f64(vt_volume_t* vol, int n, const double* m4x4s, const int32_t* planes /* n, or NULL */,
                              const double* weights /* n, or NULL = all 1 */, int out_depth, int out_height, int out_width,
                              float* out, int flags);

/* ---- nb sub-volumes of one shape back-projected from one resident stack in ONE launch: a box around every particle straight from the
 * tilt series (per-particle reconstruction of sub-tomogram workflows), the input of vt_volume_extract_dot_multi / _sum_multi.  The handle
 * holds the stack (T, H, W) as for vt_volume_backproject.  m4x4s: nb x n x 16 pull matrices in C order, entry (b, i) sends a voxel index
 * INSIDE box b to a pixel of image planes[i]; rows 1 and 2 count, rows 0 and 3 are ignored.  planes: n image indices shared by all boxes,
 * or NULL for planes[i] = i (then n must equal T).  weights: nb x n float64 in C order, or NULL for all 1.  out: nb consecutive boxes of
 * box_d * box_h * box_w float32 (host, or device with VT_OUT_DEVICE):
 *     out[b][v] = float32(base[b][v] + w_{b,0} * B_{b,0}[v] + w_{b,1} * B_{b,1}[v] + ...)        ascending i
 * with B, the skirt rule, the float64 fma chain, the accumulation step and the single rounding those of vt_volume_backproject, and base =
 * +0, or with VT_ACCUMULATE double(out[b][v]) as found; a tile that no entry of its box reaches is then neither read nor written.
 * Bit identity: box b holds exactly what vt_volume_backproject(vol, n, m4x4s + 16 n b, planes, weights + n b, box_d, box_h, box_w, ..,
 * flags) writes -- on the default route, with VT_FORCE_DIRECT, with VT_ACCUMULATE, and for entries that gather from global memory inside
 * the staged launch.  A box is therefore a fixed expression of (its matrices and weights, planes, source, box shape, interpolation,
 * route): it does not depend on nb, on the other boxes, on its place in the batch, on earlier calls or on host versus device output.
 * ONE workgroup per (box, box tile) (last_kernel 19, last_grid = nb x box tiles, box-major so that the tiles of a box share an XCD's L2)
 * runs vt_volume_backproject's kernel with a box index.  Whether an entry stages its patch in LDS follows from that entry and the LDS
 * limit alone, as in vt_volume_backproject; the largest staged patch of the batch only sizes the allocation.  last_tile = the tile
 * vt_volume_backproject uses for that box shape, last_lds_dims = (2, Ly, Lx) of the largest staged patch, last_lds_bytes = the
 * allocation.  VT_FORCE_DIRECT / VT_FORCE_TILED as for vt_volume_backproject; every other flag is ignored.  Device memory beyond the
 * source: nb x n x 200 bytes of tables in a buffer the handle recycles (callers with very many boxes cut the call along the box axis;
 * the cut cannot show in the result).
 * Bounds (VT_EUNSUPPORTED beyond): nb x box tiles < 2^31, nb x n < 2^31, a box as for vt_volume_backproject, nb x box bytes within size_t.
 * Host `out`: returns after the copy back (with VT_ACCUMULATE the caller's array is uploaded first); VT_OUT_DEVICE: asynchronous on the
 * handle's stream.  Slab handles and handles not yet finalized: VT_EINVAL; filt_* without VT_STACK and VT_EDGE_SCIPY handles:
 * VT_EUNSUPPORTED; nb <= 0, n <= 0, non-positive box dims, non-finite matrix entries or weights, a plane index outside [0, T), planes ==
 * NULL with n != T: VT_EINVAL.  A refusal leaves the handle usable. */
int vt_volume_backproject_boxes(vt_volume_t* vol, int nb, int n, const float* m4x4s /* nb x n x 16 */,
                                const int32_t* planes /* n, or NULL */, const double* weights /* nb x n, or NULL = all 1 */,
                                int box_d, int box_h, int box_w, float* out /* nb boxes, C order */, int flags);
int vt_volume_backproject_boxes_f64(vt_volume_t* vol, int nb, int n, const double* m4x4s /* nb x n x 16 */,
                                    const int32_t* planes /* n, or NULL */, const double* weights /* nb x n, or NULL = all 1 */,
                                    int box_d, int box_h, int box_w, float* out /* nb boxes, C order */, int flags);

/* ---- per-image 2-D transforms of a resident stack: a resident stack in, a stack out -- each tilt's alignment (shift, in-plane rotation,
 * magnification) before reconstruction, movie frames shifted onto each other, every image resampled onto another grid.  The handle holds
 * the stack (T, H, W) as for vt_volume_backproject.  m4x4s: n x 16 pull matrices, planes: n image indices inside [0, T), or NULL for
 * planes[i] = i (then n must equal T), weights: n float64, or NULL for all 1.  out: n images of out_h x out_w float32 in C order (host, or
 * device with VT_OUT_DEVICE).  For output pixel (h, w) of output image i
 *     y = fma(M_i[1,1], h, fma(M_i[1,2], w, M_i[1,3]))        float64
 *     x = fma(M_i[2,1], h, fma(M_i[2,2], w, M_i[2,3]))
 *     out[i, h, w] = float32(weighted_add(+0.0, w_i, B))   if -0.5 <= y < H - 0.5 and -0.5 <= x < W - 0.5, else +0
 * with B the float32 value of the handle's interpolation taken in TWO dimensions in image planes[i] at ((int)floor(y), (float)(y -
 * floor(y))), the same for x: bilinear, or the 4 x 4 cubic B-spline with the weights of the handle's 3-D kind; taps outside the image
 * read 0.  weighted_add(a, w, v) = a + w * double(v) with both roundings, vt_volume_place's accumulation step.  This is
 * vt_volume_backproject's definition for one entry and an output of depth 1.  Row 0, row 3 and column 0 of a matrix are ignored.
 * Image i is a fixed expression of (M_i, planes[i], w_i, source, (out_h, out_w), interpolation, route): it does not depend on n, on the
 * other entries, on its place in the batch, on host versus device output or on earlier calls.  A linear handle writes the same bits on
 * both routes; with VT_FORCE_DIRECT every interpolation writes the bits of vt_volume_backproject(vol, 1, M_i, &planes[i], &w_i, 1, out_h,
 * out_w, .., VT_FORCE_DIRECT).
 * ONE workgroup per (entry, 2-D output tile) (last_kernel 21, last_grid = n x tiles, entry-major so that the tiles of an image share an
 * XCD's L2) stages ONE image patch in LDS and takes one sample per pixel, coordinates by the chain above.  last_tile = (1, TH, TW), 32 x
 * 32 or 16 x 16, a function of (out_h, out_w, interpolation).  An entry whose patch, cubic halo included, exceeds 32 KiB gathers from
 * global memory inside the same launch; that follows from the entry and the output shape alone, the largest staged patch of the batch
 * only sizes the allocation: last_lds_dims = (1, Ly, Lx) of that patch, (0, 0, 0) when no entry stages, last_lds_bytes = 4 Ly Lx.
 * VT_FORCE_DIRECT makes every entry gather, VT_FORCE_TILED selects the default; every other flag but VT_OUT_DEVICE is ignored.  Device
 * memory beyond the source: n x 200 bytes of tables in a buffer the handle recycles.
 * Bounds (VT_EUNSUPPORTED beyond): n x tiles < 2^31, an image as for vt_volume_backproject, n x image bytes within size_t.
 * Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  Slab handles and handles not yet
 * finalized: VT_EINVAL; filt_* without VT_STACK and VT_EDGE_SCIPY handles: VT_EUNSUPPORTED; n <= 0, non-positive dims, non-finite matrix
 * entries or weights, a plane index outside [0, T), planes == NULL with n != T, NULL vol / m4x4s / out: VT_EINVAL.  A refusal leaves the
 * handle usable. */
int vt_volume_affine_stack(vt_volume_t* vol, int n, const float* m4x4s, const int32_t* planes /* n, or NULL */,
                           const double* weights /* n, or NULL = all 1 */, int out_h, int out_w, float* out, int flags);
int vt_volume_affine_stack_f64(vt_volume_t* vol, int n, const double* m4x4s, const int32_t* planes /* n, or NULL */,
                               const double* weights /* n, or NULL = all 1 */, int out_h, int out_w, float* out, int flags);

/* ---- warp: the resident volume resampled through a displacement grid (no reference counterpart on the GPU; the CPU analogue is
 * scipy.ndimage.map_coordinates, of which affine_transform is the affine special case) ----
 *     out[v] = sample(src, s(v)),   s(v) = a(v) + u(v)   in float64, for every voxel v = (d, h, w) of an output of out_d x out_h x out_w.
 * a(v): the float64 fma chain of the pull matrix m4x4 (rows 0..2; NULL = identity), the one vt_volume_extract documents.
 * u(v): the trilinear interpolation, in float64, of the control grid `grid` (host memory, grid_d x grid_h x grid_w x 3 float32 in C
 * order): component c of a node is a displacement in source voxels along array axis c.  The nodes span the output corner to corner:
 * node (i, j, k) sits at output coordinate (i (out_d - 1) / (grid_d - 1), ..).  Per axis either g_k == 1 (constant along that axis) or
 * 2 <= g_k <= o_k; g == o is a dense field.  The expression is fixed:
 *     r_k = (g_k - 1) / (o_k - 1) (one float64 division; 0 where g_k == 1),  q_k = v_k * r_k,  c_k = min(floor(q_k), g_k - 2),  f_k = q_k - c_k,
 *     lerp(f, a, b) = fma(f, b - a, a) per component along axis 2, then axis 1, then axis 0 (where g_k == 1: the node itself).
 * Inside test: the skirt rule on s (vlo <= s_r < vhi on every axis); outside voxels are written as +0.  Value: the handle's interpolation
 * at (int)floor(s_r), (float)(s_r - floor(s_r)).  On VT_EDGE_SCIPY handles the pad is folded into the matrix translation, as in
 * vt_volume_extract; the displacement is additive.
 * A voxel is a function of (v, m4x4, grid, shapes, source, interpolation): it does not depend on the route its tile took (trilinear
 * handles: bit for bit; the cubic kinds to rounding only -- the staged route sums the 16 tap rows per column first, the global-memory route
 * per row first), on host versus device output or on earlier calls.
 * ONE workgroup per output tile (vt_volume_place's tile for that output shape; last_kernel 20, last_grid = output tiles) loads the nodes
 * its voxels touch into LDS and bounds its source box by their range.  A tile whose own box fits 96 KiB stages it in LDS; the others, and
 * tiles whose displacements are beyond (2^20 / (max_k g_k - 1)) voxels, gather from global memory inside the same launch.  VT_FORCE_DIRECT
 * makes every tile gather; VT_FORCE_TILED is the default route; every other flag but VT_OUT_DEVICE is ignored.  last_lds_dims = the staged
 * dims of the largest staged tile, (0, 0, 0) when none stages; last_lds_bytes = node block + that box.  The grid is uploaded per call
 * into a buffer the handle recycles (12 bytes per node).
 * Bounds (VT_EUNSUPPORTED beyond, decided before any array is read): output tiles < 2^31, nodes x 3 < 2^31, the output as for
 * vt_volume_place.  Slab handles and handles not yet finalized: VT_EINVAL; VT_STACK handles with a filt_* interpolation: VT_EUNSUPPORTED;
 * grid dims outside the rule above, non-positive output dims, non-finite matrix entries or grid values, NULL vol / grid / out: VT_EINVAL.
 * Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  A refusal leaves the handle usable. */
int vt_volume_warp(vt_volume_t* vol, const float* m4x4 /* or NULL = identity */, const float* grid /* grid_d x grid_h x grid_w x 3 */,
                   int grid_d, int grid_h, int grid_w, int out_d, int out_h, int out_w, float* out, int flags);
int vt_volume_warp_f64(vt_volume_t* vol, const double* m4x4 /* or NULL = identity */, const float* grid /* grid_d x grid_h x grid_w x 3 */,
                       int grid_d, int grid_h, int grid_w, int out_d, int out_h, int out_w, float* out, int flags);

/* ---- warp_stack: every image of a resident stack resampled through its own 2-D displacement grid -- local, patch-based motion correction
 * of movie frames, per-tilt beam-induced deformation, a lens or detector distortion shared by every image.  This is vt_volume_warp's grid
 * rule on axes 1 and 2 added to vt_volume_affine_stack's pixel.  The handle holds T images of H x W as for vt_volume_affine_stack; m4x4s,
 * planes, weights and out are that call's (m4x4s == NULL: the identity for every entry).  grids: host memory, n_grids x grid_h x grid_w x 2
 * float32 in C order, n_grids == 1 (one grid shared by every entry) or n_grids == n; component 0 of a node moves y, component 1 moves x,
 * in source pixels.  The nodes span the output image corner to corner; per axis either g_k == 1 or 2 <= g_k <= o_k, and a grid of the
 * output's shape is a dense field.  For output pixel (h, w) of output image i, in float64:
 *     a_y = fma(M_i[1,1], h, fma(M_i[1,2], w, M_i[1,3])),  a_x likewise with row 2
 *     per in-plane axis k in {1, 2}:  r_k = (g_k - 1) / (o_k - 1)  (one float64 division on the host; 0 where g_k == 1)
 *                                     q_k = v_k * r_k  (a rounded value of its own),  c_k = min(floor(q_k), g_k - 2),  f_k = q_k - c_k
 *     u(h, w) = bilinear interpolation of grid G_i widened to float64: lerp(f, a, b) = fma(f, b - a, a) along axis 2, then axis 1; where
 *               g_k == 1 the node itself
 *     y = a_y + u_y,  x = a_x + u_x
 *     out[i, h, w] = float32(weighted_add(+0.0, w_i, B))   if -0.5 <= y < H - 0.5 and -0.5 <= x < W - 0.5, else +0
 * with B vt_volume_affine_stack's: the handle's interpolation taken in two dimensions in image planes[i] at ((int)floor(y), (float)(y -
 * floor(y))), the same for x.
 * Image i is a fixed expression of (M_i, G_i, planes[i], w_i, source, (out_h, out_w), interpolation, route): it does not depend on n, on its
 * neighbours or its place in the batch, on whether its grid arrived as the shared grid or as its own copy, on host versus device output
 * or on earlier calls.  An all-zero grid gives vt_volume_affine_stack's bits on the same route.  A linear handle writes the same bits on
 * both routes; the cubic kinds agree to rounding.
 * ONE workgroup per (entry, 2-D output tile) (last_kernel 22, last_grid = n x tiles entry-major, last_tile = (1, TH, TW) of
 * vt_volume_affine_stack) loads the nodes its pixels touch into LDS -- at most (TH + 1)(TW + 1) -- and bounds its source patch by their
 * range.  A tile stages its patch iff its entry's affine extents are below 4096 and its chain terms below 2^24 over the output, the
 * tile's displacements are within 2^20 / (max(grid_h, grid_w) - 1) pixels, and its own patch (the affine patch with each extent grown by
 * the range of the tile's nodes) fits 32 KiB; the other tiles gather from global memory inside the same launch.  VT_FORCE_DIRECT makes
 * every tile gather, VT_FORCE_TILED selects the default; every other flag but VT_OUT_DEVICE is ignored.  The launch is sized without
 * visiting tiles: the node block is (largest node count over the tile rows) x (largest over the tile columns) x 8 bytes rounded up to 16,
 * the patch allocation is the largest over the entries that may stage of the patch formula with the range of the entry's WHOLE grid, and
 * the 32 KiB cap itself (reported as 64 x 128) as soon as one of those bounds exceeds it.  last_lds_bytes = 128 + node block + allocation;
 * last_lds_dims = (1, Ly, Lx) of the allocation, (0, 0, 0) when no entry may stage.  Tables and grids are uploaded per call, in one copy,
 * into a buffer the handle recycles (n x 200 bytes + 8 bytes per node).
 * Bounds (VT_EUNSUPPORTED beyond, decided before any array is read): n_grids x nodes x 2 < 2^31, n x tiles < 2^31, an image as for
 * vt_volume_backproject, n x image bytes within size_t.  Handle kinds, filt_* without VT_STACK and VT_EDGE_SCIPY handles, n, dims, planes,
 * non-finite matrices or weights: as vt_volume_affine_stack.  n_grids not 1 or n, grid dims outside the rule above, a non-finite node,
 * NULL vol / grids / out: VT_EINVAL.  Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  A
 * refusal leaves the handle usable. */
int vt_volume_warp_stack(vt_volume_t* vol, int n, const float* m4x4s /* n x 16, or NULL = identity for every entry */,
                         const float* grids /* n_grids x grid_h x grid_w x 2 */, int n_grids /* 1 = shared by all entries, or n */,
                         int grid_h, int grid_w, const int32_t* planes /* n, or NULL */, const double* weights /* n, or NULL */,
                         int out_h, int out_w, float* out, int flags);
int vt_volume_warp_stack_f64(vt_volume_t* vol, int n, const double* m4x4s /* n x 16, or NULL = identity for every entry */,
                             const float* grids /* n_grids x grid_h x grid_w x 2 */, int n_grids /* 1 = shared by all entries, or n */,
                             int grid_h, int grid_w, const int32_t* planes /* n, or NULL */, const double* weights /* n, or NULL */,
                             int out_h, int out_w, float* out, int flags);

/* ---- warp_stack_sum: the images vt_volume_warp_stack would write, summed under g weight columns without being written -- the
 * motion-corrected sum of a movie, its even / odd half sums and exposure-window sums from ONE sampling of every frame.  The arguments
 * are vt_volume_warp_stack's with two changes: weights is n x g float64 in C order (NULL: one column of ones, then g must be 1), and out
 * is g images of out_h x out_w float32.  With B_i[h, w] exactly vt_volume_warp_stack's float32 sample -- the same chain, the same grid
 * rule, the same inside test with 0 outside, the same (floor, fraction), the same route per (entry, tile) --
 *     out[c, h, w] = float32(b + sum_i W[i, c] * B_i[h, w]),   i ascending
 * every term added by weighted_add (the product rounded to float64, then the sum rounded), the sum rounded to float32 once; b is +0, or
 * double(out[c, h, w]) as found with VT_ACCUMULATE (host out: copied in first).  VT_OUT_DEVICE, VT_FORCE_DIRECT and VT_FORCE_TILED are
 * as in vt_volume_warp_stack; every other flag is ignored.
 * Column c is a fixed expression of (entries in their order, column c of the weights, source, (out_h, out_w), interpolation, route): it
 * does not depend on g, on the other columns or the column's place in the matrix, on host versus device output, on earlier calls or on
 * whether a grid arrived as the shared grid or as n copies of it -- provided every sample is finite: an entry whose weights are exactly 0
 * in all of a workgroup's columns is passed over without being sampled, where the loop below would add 0 x NaN for a non-finite sample.
 * Bit identities: (1) column c holds the bits of the host loop acc = b; for i ascending: acc = acc + W[i, c] * double(S_i[h, w]);
 * float32(acc), with S = vt_volume_warp_stack(..., weights = NULL) from the same handle with the same flags -- for every interpolation
 * on both routes (a pixel that maps outside adds +0 to a sum that started at +0; with VT_ACCUMULATE the identity holds up to the sign of
 * a zero found in out); (2) a one-hot column (W[k, c] = w, 0 elsewhere) holds vt_volume_warp_stack's image k under weight w.
 * ONE workgroup per (chunk of 4 consecutive columns, 2-D output tile) (last_kernel 26, last_grid = column chunks x tiles chunk-major,
 * last_tile = (1, TH, TW) of vt_volume_warp_stack) walks the n entries in ascending order with float64 accumulators in registers; per
 * entry it runs vt_volume_warp_stack's steps with that call's tile, node block, per-tile route rule and patch allocation.  A tile
 * classified wholly outside an entry adds nothing; with VT_ACCUMULATE a tile no entry reaches is not written.  The next entry's patch
 * and the nodes of the entry after it are loaded while the current entry is sampled: with a grid per entry LDS holds NB = 3 node blocks,
 * with a shared grid NB = 1 (loaded once per workgroup), then two patch allocations:
 *     last_lds_bytes = 4 * NB * node_floats + 2 * allocation bytes
 * node_floats = 2 x (largest node count over the tile rows) x (largest over the tile columns) rounded up to 4, the allocation
 * vt_volume_warp_stack's; last_lds_dims = (2, Ly, Lx) of the allocation, (0, 0, 0) when no entry may stage.  No atomics, no memset.
 * Tables and grids are uploaded per call, in one copy (n x (192 + 8 g) bytes + 8 bytes per node); no image but the g results exists.
 * Bounds (VT_EUNSUPPORTED beyond, decided before any array is read): vt_volume_warp_stack's on grids and image, column chunks x tiles
 * < 2^31, g x image bytes within size_t.  Checks in vt_volume_warp_stack's order; g <= 0, weights == NULL with g != 1, non-finite
 * weights: VT_EINVAL.  Slab handles, filt_* without VT_STACK and VT_EDGE_SCIPY handles as for vt_volume_warp_stack.  Host `out`: returns
 * after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  A refusal leaves the handle usable. */
int vt_volume_warp_stack_sum(vt_volume_t* vol, int n, const float* m4x4s /* n x 16, or NULL = identity for every entry */,
                             const float* grids /* n_grids x grid_h x grid_w x 2 */, int n_grids /* 1 = shared by all entries, or n */,
                             int grid_h, int grid_w, const int32_t* planes /* n, or NULL */,
                             int g, const double* weights /* n x g, C order, or NULL = all 1 (then g must be 1) */,
                             int out_h, int out_w, float* out /* g images, C order */, int flags);
int vt_volume_warp_stack_sum_f64(vt_volume_t* vol, int n, const double* m4x4s /* n x 16, or NULL = identity for every entry */,
                                 const float* grids /* n_grids x grid_h x grid_w x 2 */, int n_grids /* 1 = shared by all entries, or n */,
                                 int grid_h, int grid_w, const int32_t* planes /* n, or NULL */,
                                 int g, const double* weights /* n x g, C order, or NULL = all 1 (then g must be 1) */,
                                 int out_h, int out_w, float* out /* g images, C order */, int flags);

/* ---- filter_stack: every image of a resident stack convolved with a 1-D filter along axis 1 or 2 -- the ramp filter of weighted
 * back-projection between alignment and reconstruction (after alignment the tilt axis lies along an array axis, and the filter runs along
 * the other one), per-tilt low-pass, smoothing before cross-correlation, derivative taps.  The handle holds the stack (T, H, W) as for
 * vt_volume_affine_stack; planes, weights and out are that call's, the output is n images of the source's own shape H x W.  taps: host
 * memory, n_taps x k float64 in C order, n_taps == 1 (one row shared by every entry) or n_taps == n; k odd.  With L the extent of `axis`,
 * r = (k - 1) / 2 and t the tap row of entry i, for output pixel (h, w) of image i with p = planes[i], axis 2:
 *     acc = +0.0                                               float64
 *     for j = 0 .. k-1 ascending, skipping every j with t[j] == 0 (either sign):
 *         x = w + r - j
 *         s = S[p, h, x] if 0 <= x < L;  pad 0: such a j is skipped like a zero tap;  pad 1: S[p, h, clamp(x, 0, L-1)]
 *         acc = fma(t[j], (double)s, acc)
 *     out[i, h, w] = float32(w_i * acc)
 * and with axis 1 the same along h.  This is numpy.convolve(line, t, 'same'), scipy.ndimage.convolve1d(.., mode='constant' | 'nearest',
 * origin=0).  Zero taps are skipped by definition: a non-finite sample spreads only through non-zero taps, and the even-offset zeros of
 * a Ram-Lak row cost nothing.  An all-zero row writes +0.  (The kernel reads pad-0 samples outside the line as +0 instead of skipping
 * them; the two differ only where acc is -0, which takes a product that underflows float64.)
 * Image i is a fixed expression of (t, planes[i], w_i, source, axis, pad): it does not depend on n, on the other entries, on its place
 * in the batch, on whether its row arrived as the shared row or as its own, on host versus device output or on earlier calls; zero taps
 * added on both sides of a row change nothing, and filtering the transposed images along the other axis gives the transposed bits.
 * ONE workgroup per (entry, strip of 64 lines across the unfiltered axis, segment of 64 outputs along the filtered axis) (last_kernel 23,
 * last_grid = n x strips x segments entry-major, last_tile = (1, 64, 64) laid out (1, h, w)) walks the non-zero taps 128 consecutive j
 * at a time and stages, per step, the 191 positions its outputs reach for its 64 lines in LDS, pad values included: last_lds_dims =
 * (1, 191, 65), last_lds_bytes = 49660 whatever the image and k are.  A lane owns one line and 16 consecutive outputs as float64
 * accumulators, and takes the taps 16 consecutive j at a time from a register window of 31 widened samples.  There is one route; every flag but VT_OUT_DEVICE is ignored.
 * Device memory beyond the source: 32 bytes per entry, 16 bytes per non-zero tap and 8 (k + 128) bytes per tap row in a buffer the
 * handle recycles.
 * Bounds (VT_EUNSUPPORTED beyond, decided before any array is read): n_taps x k <= 2^26 (every odd k <= 2L - 1 is served up to there: no
 * bound on k of its own), n x strips x segments < 2^31, n x image bytes within size_t, L <= 2^31 - 257.  The handle must hold samples: filt_*
 * interpolations hold prefilter coefficients and are refused with VT_EUNSUPPORTED, VT_STACK or not (filter on a linear handle and build
 * the filt_* handle from the result), as are VT_EDGE_SCIPY handles; VT_STACK is not required.  Slab handles and handles not yet
 * finalized, n <= 0, k even, k < 1 or k > 2L - 1 (taps beyond reach nothing), n_taps not 1 or n, axis not 1 or 2, pad not 0 or 1,
 * non-finite taps or weights, a plane index outside [0, T), planes == NULL with n != T, NULL vol / taps / out: VT_EINVAL.  Host `out`:
 * returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  The handle's output shape is neither read nor
 * changed.  A refusal leaves the handle usable. */
int vt_volume_filter_stack(vt_volume_t* vol, int n, const int32_t* planes /* n, or NULL */,
                           const double* taps /* n_taps x k, C order */, int n_taps /* 1 or n */, int k,
                           int axis /* 1 or 2 */, int pad /* 0 zero, 1 edge */,
                           const double* weights /* n, or NULL = all 1 */, float* out /* n x H x W */, int flags);

/* ---- correlate_stack: the cross-correlation of every image of a resident stack, or of every patch of it, with a reference over a window
 * of integer shifts -- the scores that coarse tilt alignment (every tilt against its neighbour), patch tracking and local motion
 * correction (every patch against the frame sum) take their shifts from: the step that produces vt_volume_affine_stack's shifts and
 * vt_volume_warp_stack's grids.  The handle holds samples S (T, H, W); the rules for the handle are vt_volume_filter_stack's.  Entry i
 * pairs image p = planes[i] (NULL: image i, n = T) with a reference r_i (H, W), float32: host memory `refs`, n_refs x H x W in C order
 * with n_refs == 1 (shared) or n, or, with refs == NULL, the resident image ref_planes[i] (nothing is uploaded: a tilt against its
 * neighbour).  A patch grid (grid_h, grid_w), 1 <= grid_h <= H and 1 <= grid_w <= W, cuts the image into rectangles in integer
 * arithmetic: patch (a, b) covers rows [a H / grid_h, (a+1) H / grid_h) and columns [b W / grid_w, (b+1) W / grid_w) by floor
 * division.  The shift window is (r_h, r_w), 0 <= r_h <= H - 1 and 0 <= r_w <= W - 1 (shifts beyond overlap nothing).
 *     out[i, a, b, u, v] = sum over (y, x) in patch (a, b) of  (double) r_i[y, x] * (double) s(y + u - r_h, x + v - r_w)
 *     s(y', x') = S[p, y', x'] inside the image, +0 outside
 * out: float64, n x grid_h x grid_w x (2 r_h + 1) x (2 r_w + 1) in C order, host memory or device memory with VT_OUT_DEVICE.  Every
 * product is exact in float64 (both factors carry 24 bits); every addition is rounded, by fma.  Outside samples are +0 MULTIPLIED, not
 * skipped: a non-finite reference pixel makes every score of its patch non-finite, a non-finite image pixel reaches exactly the
 * (patch, shift) pairs whose window covers it.  Host refs with non-finite entries are refused (VT_EINVAL), like vt_volume_extract_dot's
 * template; resident references are taken as they are.
 * The order of additions is fixed by the patch's rows and columns alone.  A patch is cut from its own first row and column into pieces
 * of 64 x 64 pixels, piece (py, px) row-major, and a piece into four bands of 16 rows.  A band sum starts from +0 and takes its
 * pixels row by row, ascending x within a row, acc = fma(r, s, acc).  A piece sum is ((band 0 + band 1) + band 2) + band 3 (a band
 * the piece does not reach is +0).  A score is the piece sums added in ascending piece index, starting from piece 0 itself, by a second
 * small launch; no atomics, no memset.  A score is therefore a fixed expression of (r_i, image p, patch, shift, H, W): it does not
 * depend on n, on the other entries or its place in the batch, on the other patches, on r_h and r_w beyond the shift lying inside the
 * window, on whether the reference came shared, per entry or resident, on host versus device output, on earlier calls or on recycled
 * memory; repeated calls give identical bits.
 * ONE workgroup per (entry, patch, piece, block of shifts) (last_kernel 24, last_tile = (1, 64, 64): the piece).  A lane owns one
 * shift row and a run of cv consecutive column shifts as float64 accumulators, cv = 11 if that pads 2 r_w + 1 to fewer columns than 9
 * does, else 9; runs = min(7, ceil((2 r_w + 1) / cv)) runs lie side by side and rows_blk = min(64 / runs, 2 r_h + 1) shift rows on top of
 * each other in a wave, so a block is rows_blk x runs cv shifts and a larger window goes onto the grid.  The workgroup stages the
 * reference piece (16 KiB) and the 64 + rows_blk - 1 rows of 63 + runs cv image samples the block reaches, at a pitch of 64 + runs cv
 * floats, zeros outside the image included: last_lds_dims = (1, 64 + rows_blk - 1, 64 + runs cv), last_lds_bytes = 16384 + 4 x rows x
 * pitch, at most 56992.  Every patch gets the piece grid of the call's largest patch (a piece past a smaller patch's end adds +0);
 * last_grid = the workgroups of the call's last launch, (entries x patches of it) x pieces x blocks.  A call whose partial sums (pieces
 * x shifts x 8 bytes per (entry, patch) when a patch has several pieces) would exceed 64 MiB is split into launches inside the call.
 * Every flag but VT_OUT_DEVICE is ignored.  Device memory beyond the source: 8 bytes per entry and the host references, in the table
 * buffer, and the partial sums, in a buffer the handle recycles.
 * Bounds (VT_EUNSUPPORTED beyond, decided before any array is read): n x grid_h x grid_w x (2 r_h + 1) x (2 r_w + 1) < 2^31 output
 * elements; pieces x blocks of one patch < 2^31 workgroups and pieces x shifts of one patch < 2^31 partial sums (more workgroups than
 * that in a call are split into launches); n_refs x H x W <= 2^30 host reference pixels.  filt_* handles hold prefilter coefficients
 * and are refused with VT_EUNSUPPORTED, as are VT_EDGE_SCIPY handles; VT_STACK is not required.  Slab handles and handles not yet
 * finalized, n <= 0, n_refs not 0, 1 or n (0 only with ref_planes, which ignores it), refs and ref_planes both NULL or both given, a
 * plane or reference plane outside [0, T), planes == NULL with n != T, a grid or window outside the ranges above, NULL vol / out:
 * VT_EINVAL.  Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  The handle's output shape
 * is neither read nor changed.  A refusal leaves the handle usable. */
int vt_volume_correlate_stack(vt_volume_t* vol, int n, const int32_t* planes /* n, or NULL */,
                              const float* refs /* n_refs x H x W, or NULL */, int n_refs /* 1 or n; 0 with ref_planes */,
                              const int32_t* ref_planes /* n, or NULL */, int grid_h, int grid_w, int r_h, int r_w,
                              double* out /* n x grid_h x grid_w x (2 r_h + 1) x (2 r_w + 1) */, int flags);

/* ---- moments_stack: the sum and the sum of squares of the samples that lie under every patch at every shift of vt_volume_correlate_stack's
 * window -- with the reference's own two sums, what turns a raw score into a correlation coefficient (voltools_amd.utils.
 * normalized_scores).  The handle, the entries, the patch grid and the window follow vt_volume_correlate_stack's rules word for word:
 * samples S (T, H, W); entry i is image p = planes[i] (NULL: image i, n = T); patch (a, b) of the grid (grid_h, grid_w), 1 <= grid_h <= H
 * and 1 <= grid_w <= W, covers rows [a H / grid_h, (a+1) H / grid_h) and columns [b W / grid_w, (b+1) W / grid_w) by floor division;
 * the window is (r_h, r_w), 0 <= r_h <= H - 1 and 0 <= r_w <= W - 1.
 *     out[i, a, b, u, v, 0] = sum over (y, x) in patch (a, b) of  (double) s(y + u - r_h, x + v - r_w)
 *     out[i, a, b, u, v, 1] = the same sum of                     (double) s(..)^2
 *     s(y', x') = S[p, y', x'] inside the image, +0 outside
 * out: float64, n x grid_h x grid_w x (2 r_h + 1) x (2 r_w + 1) x 2 in C order, host memory or device memory with VT_OUT_DEVICE.  Every
 * square is exact in float64 (the factor carries 24 bits); every addition is rounded.  Every sum starts from +0, and the order of
 * additions is a fixed expression of the patch's own rows and columns, the shift and (H, W):
 *   - a row sum R[y', b, dv], for image row y' in [0, H), patch column b and column displacement dv = v - r_w, starts from +0 and takes
 *     the samples s(y', x + dv) of the patch's columns x in ascending order, acc0 = acc0 + s and acc1 = fma(s, s, acc1); a sample
 *     outside the image is +0;
 *   - out[i, a, b, u, v, k] starts from +0 and takes the row sums R[y + u - r_h, b, v - r_w][k] of the patch's rows y in ascending
 *     order; a row outside the image is +0.
 * Every value is a plain sum of its own samples: there are no running sums that add the entering sample and subtract the leaving one.
 * A value therefore does not depend on n, on the other entries or its place in the batch, on the other patches, on r_h and r_w beyond
 * the shift lying inside the window, on host versus device output, on earlier calls or on recycled memory; repeated calls give identical
 * bits.  No atomics, no memset.  A non-finite image pixel reaches exactly the (patch, shift) pairs whose window covers it, and no
 * others.  out[.., 0] equals vt_volume_correlate_stack against a reference of ones, and out[.., 1] the same on a handle holding the
 * squared samples, up to the rounding of the two orders of addition (exactly, where every partial sum is exact); the work here is
 * pixels x (2 r_w + 1) additions and fmas, not pixels x shifts.
 * TWO launches per run of entries (last_kernel 25).  The first forms the row sums: one workgroup per (entry, block of rows_wg image
 * rows, patch column, block of column shifts).  A lane owns one image row and a run of cv consecutive column shifts as 2 cv float64
 * accumulators, cv = 11 if that pads 2 r_w + 1 to fewer columns than 9 does, else 9; runs = min(7, ceil((2 r_w + 1) / cv)) runs lie
 * side by side in a wave, which holds 64 / runs rows, and rows_wg = 4 x (64 / runs); a block of column shifts is runs cv wide and a
 * wider window goes onto the grid.  The workgroup walks its patch column in chunks of 32 pixels and stages, per chunk, rows_wg rows
 * of 31 + runs cv samples at a pitch of 32 + runs cv floats, zeros outside the image included: last_tile = (1, rows_wg, 32),
 * last_lds_dims = (1, rows_wg, 32 + runs cv), last_lds_bytes = 4 x rows_wg x pitch, at most 44032.  The second launch has one thread
 * per value.  last_grid = the workgroups of the first launch of the call's last run of entries, entries of it x ceil(H / rows_wg) x
 * grid_w x blocks of column shifts.  A call whose row sums (H x grid_w x (2 r_w + 1) x 16 bytes per entry) would exceed 64 MiB is
 * split into runs of entries inside the call, one entry per run at least.
 * Every flag but VT_OUT_DEVICE is ignored.  Device memory beyond the source: 8 bytes per entry, in the table buffer, and the row sums,
 * in the buffer the handle recycles for partial sums.
 * Bounds (VT_EUNSUPPORTED beyond, decided before any array is read): n x grid_h x grid_w x (2 r_h + 1) x (2 r_w + 1) x 2 < 2^31 output
 * elements; the workgroups of one entry < 2^31 (more than that in a call are split into runs of entries) and H x grid_w x (2 r_w + 1) x
 * 2 < 2^31 row sums per entry.  filt_* handles hold
 * prefilter coefficients and are refused with VT_EUNSUPPORTED, as are VT_EDGE_SCIPY handles; VT_STACK is not required.  Slab handles
 * and handles not yet finalized, n <= 0, a plane outside [0, T), planes == NULL with n != T, a grid or window outside the ranges above,
 * NULL vol / out: VT_EINVAL.  Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  The
 * handle's output shape is neither read nor changed.  A refusal leaves the handle usable. */
int vt_volume_moments_stack(vt_volume_t* vol, int n, const int32_t* planes /* n, or NULL */, int grid_h, int grid_w, int r_h, int r_w,
                            double* out /* n x grid_h x grid_w x (2 r_h + 1) x (2 r_w + 1) x 2 */, int flags);

/* ---- projection: the transformed volume summed over axis 0, without materialising it ----
 * Replaces `static_volume.transform(...).sum(axis=0)` of examples/projections.py:20-26 (a cupy reduction after the
 * kernel of volume.py:78).  out_hw: out_height * out_width float32 (host, or device with VT_OUT_DEVICE).
 * Matrices of the form [1 0 0 tz; 0 a b ty; 0 c d tx] (the example's rotation=(i,0,0) 'sxyz') are computed as one
 * weighted streaming sum of the resident planes followed by a 2-D interpolation (last_kernel 7); other matrices
 * transform into an internal buffer and sum it.  Outside voxels contribute 0; VT_KEEP_OUTSIDE is ignored. */
int vt_volume_project(vt_volume_t* vol, const float* m4x4, float* out_hw, int flags);
int vt_volume_project_f64(vt_volume_t* vol, const double* m4x4, float* out_hw, int flags);

/* ---- a stack of projections per call: a tilt series (the loop of examples/projections.py:20-26 with the rotation about an axis
 * perpendicular to the projection axis) without materialising any transformed volume.
 * m4x4s: n x 16 pull matrices; image i, of shape (height, width), holds at [h, w] the sum over d < depth of what vt_volume_affine would
 * write at (d, h, w) for matrix i if the handle's output shape were (depth, height, width), under the handle's interpolation and boundary
 * contract (VT_EDGE_SCIPY handles included).  Outside voxels contribute 0; VT_KEEP_OUTSIDE is ignored.  out: n consecutive images.
 * The handle's own output shape is not read, and is what it was when the call returns.
 * The fused kernel (last_kernel 12) serves every (matrix, image tile, depth segment) in one launch: the samples of a pixel are added in
 * float64 in depth order, depth segments are summed in ascending order by a second small launch and rounded to float32 once; matrices
 * whose tile footprint fits no LDS box gather from global memory inside the same launch.  Image i depends on M_i, the source, (depth,
 * height, width) and the route only, bit for bit -- not on n, the other matrices or its place in the batch -- and repeated calls give
 * identical bits.  Its float64 partial sums live in a buffer the handle recycles, never larger than max(depth * height * width * 4 bytes,
 * one matrix's partials); larger batches are split into several launches inside the call.
 * VT_FORCE_TILED selects kernel 12 whatever the shape; VT_FORCE_DIRECT runs the path of vt_volume_project once per matrix inside the call
 * (last_kernel is what that path reports; it sets the handle's output shape to (depth, height, width) for the duration of the call, and
 * its internal volume and lazily built copies grow and stay as vt_volume_project would leave them for that shape); otherwise the
 * route follows from (interpolation, depth, height, width) alone
 * (kernel 12 for trilinear outputs up to 256 and bspline / filt_bspline outputs up to 64 in every dimension, where it was measured
 * faster than the loop; the loop elsewhere).
 * Host `out`: returns after the copy back; VT_OUT_DEVICE: asynchronous on the handle's stream.  Slab handles and handles not yet
 * finalized: VT_EINVAL; n <= 0, non-positive dims, non-finite matrix entries: VT_EINVAL. */
int vt_volume_project_batch(vt_volume_t* vol, int n, const float* m4x4s,
                            int depth, int height, int width, float* out, int flags);
int vt_volume_project_batch_f64(vt_volume_t* vol, int n, const double* m4x4s,
                                int depth, int height, int width, float* out, int flags);

/* ---- timing: replaces the cupy event pairs of profile=True (transforms.py:167-169,214-219; volume.py:65-67,80-85)
 * Events are recorded on the handle's stream. vt_timer_stop synchronises and returns milliseconds. */
int vt_timer_start(vt_volume_t* vol);
int vt_timer_stop(vt_volume_t* vol, float* ms);

/* ---- prefilter on a caller-owned device array: replaces _bspline_prefilter (transforms.py:290-309;
 * kernels SamplesToCoefficients3DX/Y/Z, bspline.h:58-99).  In place from the caller's point of view. */
int vt_prefilter_inplace(int dev, float* d_volume, int depth, int height, int width);

/* ---- one-shot transform(): replaces the GPU branch of affine (transforms.py:164-226):
 * host in -> upload -> (prefilter) -> kernel -> host out. */
int vt_affine_oneshot(int dev, const float* h_volume, int depth, int height, int width, int interp,
                      const float* m4x4, float* h_out, int flags, float* elapsed_ms /* may be NULL */);

const char* vt_last_error(void);
const char* vt_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VOLTOOLS_HIP_H */
