/*
 * mvs.h -- C ABI of the MI355X-native dense-MVS depth engine (libmvs_hip.so).
 *
 * This is the drop-in boundary for the hot path of addam/mesh-reconstruction: every entry point
 * replaces one call the reference's driver makes through its link-time renderer seam
 * (recon.hpp:93-100, `class Render` + `spawnRender`; Makefile:2,16,21 `render_${SYSTEM_OPENGL}.cpp`)
 * or through the free functions of recon.hpp:40-50.  Plain pointers and sizes only; no C++ or
 * torch types.  The C++ shim that turns these into `class RenderHIP : public Render`,
 * `spawnRender` and `calculateFlow` lives in mesh-reconstruction_amd/host/ (see INTEGRATION.md).
 *
 * Conventions:
 *   - camera matrices: 4x4 float, row-major, applied as P*(x,y,z,1)^T       (render_glx.cpp:265,338,375)
 *   - images: top-down, row-major, tightly packed                           (cv::flip at render_glx.cpp:365,392)
 *   - depth maps: NDC z in [-1,1], 1.0f == backgroundDepth == "no geometry" (recon.hpp:30)
 *   - every function returns 0 on success, a negative MVS_E* code on error; the message is
 *     available from mvs_last_error().  Nothing aborts, asserts or exits (the reference does:
 *     recon.cpp:49, util.cpp:442).
 *   - a context is bound to one GPU; calls on one context must be serialised by the caller
 *     (the reference is single-threaded: one GL context, render_glx.cpp:152-208).
 *   - the library never retains caller pointers after a call returns.
 *   - there is NO CPU fallback: without a usable HIP device mvs_create() fails.
 */
#ifndef MVS_H
#define MVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVS_OK 0
#define MVS_EINVAL (-1)   /* bad argument */
#define MVS_EHIP (-2)     /* HIP runtime error */
#define MVS_ESTATE (-3)   /* call sequence error (e.g. sweep run before inputs were set) */
#define MVS_ENOMEM (-4)   /* device or host allocation failed */

#define MVS_BACKGROUND_DEPTH 1.0f /* recon.hpp:30 */

typedef struct mvs_ctx mvs_ctx;

/* ---- life cycle: replaces RenderGLX::RenderGLX / ~RenderGLX (render_glx.cpp:152-227) -------- */
mvs_ctx *mvs_create(int device, int width, int height);
void mvs_destroy(mvs_ctx *ctx);
/* last error text of `ctx`; with ctx == NULL the last error of a failed mvs_create() */
const char *mvs_last_error(const mvs_ctx *ctx);
/* run all subsequent work of `ctx` on the caller's hipStream_t (NULL = the context's own stream) */
int mvs_set_stream(mvs_ctx *ctx, void *hip_stream);
/* page-locked host memory for frames / results handed to the entry points below (optional: any host pointer works; from pinned
 * memory the one-call entries upload at the full PCIe rate and overlap with the device-side preparation).  NULL on failure. */
void *mvs_host_alloc(size_t bytes);
void mvs_host_free(void *p);
/* block until all queued work of the context has finished */
int mvs_synchronize(mvs_ctx *ctx);
int mvs_width(const mvs_ctx *ctx);
int mvs_height(const mvs_ctx *ctx);

/* Render::depth restricted to the pixels a caller actually reads: Heuristic::chooseCameras renders 200 face cameras per
 * outer iteration (heuristic.cpp:445-456) and filterCameras looks ONE pixel up per real camera in each map
 * (heuristic.cpp:307-312).  Rasterises the depth map for `cam` on the device and returns out[i] = depth[rows[i]][cols[i]]
 * (same values as mvs_depth, without moving the map across PCIe).  Pixels outside the map are an error. */
int mvs_depth_probe(mvs_ctx *ctx, const float cam[16], int n, const int32_t *rows, const int32_t *cols, float *out);

/* ---- renderer: replaces class Render (recon.hpp:93-99) ---------------------------------------- */
/* Render::loadMesh, render_glx.cpp:230-258: verts4 = nverts homogeneous rows (x,y,z,w), faces3 = int32 triples */
int mvs_load_mesh(mvs_ctx *ctx, const float *verts4, int nverts, const int32_t *faces3, int nfaces);
/* Render::depth, render_glx.cpp:369-397: out_hw = H*W float NDC z, empty pixels 1.0 */
int mvs_depth(mvs_ctx *ctx, const float cam[16], float *out_hw);
/* Render::projected, render_glx.cpp:261-367: out_hw3 = H*W*3 u8 (warped side intensity, mask, mask) */
int mvs_projected(mvs_ctx *ctx, const float cam[16], const uint8_t *frame_hw, const float projector[16],
                  uint8_t *out_hw3);

/* ---- photometric helpers: replace util.cpp:332-403 -------------------------------------------- */
/* mixBackground, util.cpp:366-387: depth_hw_inout is mutated (masked pixels := 1.0) */
int mvs_mix_background(mvs_ctx *ctx, const uint8_t *img_hw3, const uint8_t *bg_hw, float *depth_hw_inout,
                       uint8_t *out_hw);
/* compare, util.cpp:332-361: multi-scale L1 pyramid difference, out_hw = H*W float */
int mvs_compare(mvs_ctx *ctx, const uint8_t *prev_hw, const uint8_t *next_hw, float *out_hw);
/* flowRemap, util.cpp:390-403: bicubic remap by flow (flow_stride floats per pixel, first two used).  The sample position (x + u, y + v) is
 * taken in 1/32 pixel, rounded half to even; samples outside the frame read the constant border, 0.  A coordinate whose x32 value is NaN,
 * infinite or outside int32 reads the border too -- the pixel's output is 0 -- as the reference's x86 build does (cvRound gives INT_MIN). */
int mvs_flow_remap(mvs_ctx *ctx, const float *flow, int flow_stride, const uint8_t *image_hw, uint8_t *out_hw);
/* calculateFlow, flow.cpp:19-42: out_hw4 = H*W*4 float (u, v, variance, 0).  With use_farneback the window is (H + W) / 100 (flow.cpp:24),
 * which is 0 below H + W = 100 (the reference divides by its square there and returns NaN everywhere): such a call is refused with
 * MVS_EINVAL and a message that names the window, before anything is queued -- by mvs_flow, mvs_process_frame and mvs_process_frame_slots
 * alike.  The variational form (use_farneback = 0) has no window and is valid for every context size, 2 x 2 included. */
int mvs_flow(mvs_ctx *ctx, const uint8_t *prev_hw, const uint8_t *next_hw, int use_farneback, float *out_hw4);

/* ---- per-pixel triangulation + normals: replaces triangulatePixels (util.cpp:167-329, recon.cpp:114) -------------- */
/* flows_hw4: nviews pointers to H*W*4 floats (u, v, variance, 0) as mvs_flow writes them; depth_hw: the (mixBackground-
 * updated) depth map; out_points7: room for H*W rows of (x, y, z, w, nx, ny, nz); *out_count = rows written, in pixel
 * scan order like the reference's pixelId. */
int mvs_triangulate(mvs_ctx *ctx, int nviews, const float *const *flows_hw4, const float main_cam[16],
                    const float *side_cams /* nviews*16 */, const float *depth_hw, float *out_points7, int *out_count);

/* ---- one main frame, device resident: the body of the loop recon.cpp:65-117 ------------------------------------------ */
/* depth(main) -> for every side view: projected -> mixBackground (depth mutated cumulatively) -> calculateFlow ->
 * triangulatePixels, with every intermediate kept in HBM: frames go up once, only the points come back.  Bit-identical
 * to calling mvs_depth / mvs_projected / mvs_mix_background / mvs_flow / mvs_triangulate in that order.
 * out_points7 needs room for H*W rows; depth_after_hw (nullable) receives the depth map after the last mixBackground. */
int mvs_process_frame(mvs_ctx *ctx, const float main_cam[16], const uint8_t *main_frame_hw, int nside,
                      const float *side_cams /* nside*16 */, const uint8_t *const *side_frames_hw, int use_farneback,
                      float *out_points7, int *out_count, float *depth_after_hw);
/* The same with the frames taken from the context's frame store (mvs_frame_store / mvs_frame_upload, below): recon.cpp:65-117 reads every frame of a
 * sequence about five times -- once as a main frame (configuration.cpp frame(i), recon.cpp:68), four times as a side view (:80) -- and through the
 * store it crosses PCIe once.  main_slot / side_slots name filled slots (MVS_ESTATE otherwise); results are those of mvs_process_frame on the
 * same frames, bit for bit; stream-ordered behind the uploads that filled the slots. */
int mvs_process_frame_slots(mvs_ctx *ctx, const float main_cam[16], int main_slot, int nside, const float *side_cams /* nside*16 */,
                            const int *side_slots, int use_farneback, float *out_points7, int *out_count, float *depth_after_hw);

/* cv::resize(frame, Size(dw, dh)) as Configuration applies it to every decoded frame when -s / the clip size asks for it
 * (configuration.cpp:233: INTER_LINEAR -- the CV_INTER_AREA in that call lands in the ignored fx argument): OpenCV's fixed-point
 * bilinear resize on u8, 1 or 3 interleaved channels, host buffers in and out. */
int mvs_resize_u8(mvs_ctx *ctx, const uint8_t *src, int src_w, int src_h, int channels, uint8_t *dst, int dst_w, int dst_h);

/* Texture filter of Render::projected's frame texture.  The reference uploads the side frame with glGenerateMipmap and samples it
 * with GL_LINEAR_MIPMAP_LINEAR (render_glx.cpp:83-85): MVS_FILTER_MIPMAP (default) builds the mip chain (2 x 2 box, u8 levels) per
 * frame and blends the two levels the pixel's footprint calls for (fine derivatives on the 2 x 2 pixel quad, isotropic; DESIGN.md
 * section 5 states the arithmetic, the oracle restates it); under magnification and at 1 : 1 it IS level-0 bilinear.
 * MVS_FILTER_LEVEL0 samples level 0 only (rounds 1-2 of this library; the sweep's samplers always do). */
#define MVS_FILTER_MIPMAP 0
#define MVS_FILTER_LEVEL0 1
int mvs_set_texture_filter(mvs_ctx *ctx, int filter);
int mvs_texture_filter(const mvs_ctx *ctx);

/* ---- point-cloud filter: replaces Heuristic::filterPoints (heuristic.cpp:55-176, recon.cpp:125) ------------------- */
/* points4: npoints homogeneous rows; alpha = the reference's alphaVals.back() (radius = alpha/4, compared with squared
 * distances as the reference does).  keep_out receives the ascending indices of the retained points, *out_count how
 * many; the caller compacts points and normals with them (heuristic.cpp:166-175). */
int mvs_filter_points(mvs_ctx *ctx, const float *points4, int npoints, float alpha, int32_t *keep_out, int *out_count);
/* The npoints densities (heuristic.cpp:103-136, after the last counted update) the last successful mvs_filter_points of this context
 * ranked its points by, in input order; they stay on the device in a buffer no other stage writes, so calls of other stages in between
 * do not disturb them.  MVS_ESTATE before any mvs_filter_points, after one that failed and after one with npoints = 0.  Synchronises.
 * mvs_filter_density_count: how many densities the fetch would write (0 where it would return MVS_ESTATE, and for a NULL ctx). */
int mvs_filter_density_fetch(mvs_ctx *ctx, float *density_n);
int mvs_filter_density_count(const mvs_ctx *ctx);

/* ---- plane sweep: the D-plane generalisation of shader.frag:11-25 ------ */
/*
 * One-call form on host buffers.  For every pixel of the main view and every plane
 * z_d = z_lo + (z_hi - z_lo)(d + 1/2)/nplanes (main-camera NDC z) the side frames are warped into the
 * main view exactly as shader.frag does for the mesh position, quantised to u8 like the RGB8
 * read-back (render_glx.cpp:359), and the cost is the mean over in-frame views of |I_main - I_warp|.
 * depth_hw: H*W float, NDC z of the lowest-cost plane (ties -> lowest d), 1.0 where no view is in frame.
 * cost_hw (nullable): H*W float best cost.  volume_dhw (nullable): nplanes*H*W float normalised
 * cost, +inf where no view is in frame.
 */
int mvs_sweep(mvs_ctx *ctx, const float main_cam[16], const uint8_t *main_hw, int nviews,
              const float *side_cams /* nviews*16 */, const uint8_t *const *side_frames, int nplanes,
              float z_lo, float z_hi, float *depth_hw, float *cost_hw, float *volume_dhw);

/* The sweep's sampler at ONE plane per pixel, z = depth_hw[p] (e.g. the output of mvs_depth): out_hw2 = H*W pairs
 * (warped u8 intensity, mask 255/0); background pixels and out-of-frame samples give (0, 0).  With the renderer's depth
 * map this reproduces Render::projected (render_glx.cpp:261-367) minus its shadow test -- the parity hook between the
 * D-plane sweep and the reference's single-hypothesis warp. */
int mvs_warp_by_depth(mvs_ctx *ctx, const float main_cam[16], const float *depth_hw, const float side_cam[16],
                      const uint8_t *frame_hw, uint8_t *out_hw2);

/* Texture-fetch arithmetic of the sweep.  The reference leaves this to the OpenGL driver (GL_LINEAR on a
 * GL_RED8 texture, render_glx.cpp:75-85, read back as RGB8, :359), which pins neither sub-texel precision nor weight width.
 *   MVS_SAMPLER_FIXED (default): positions quantised to 1/32 texel and 8-bit weights from a 32 x 32 table -- the model of
 *     fixed-function samplers and of OpenCV's fixed-point remap (INTER_BITS = 5, the path of the reference's flowRemap,
 *     util.cpp:401); the warped intensity keeps the table's precision and a packed cell is count << 24 | sum |w.t - 255 I_main|
 *     (sums in 1/255 grey levels; at most 255 views; images of up to 16383 x 16383).  About 30 % fewer instructions per sample on gfx950.
 *   MVS_SAMPLER_EXACT_F32: bilinear interpolation in f32 with one rounding per operation, result rounded to u8 like the RGB8
 *     read-back; a packed cell is count << 16 | sum |u8 - I_main| (at most 257 views).
 * Both are restated bit for bit by the CPU oracle; they select the same plane except where two planes' costs are within the
 * quantisation step (measured: DESIGN.md).  Changing the sampler invalidates the region plan, not the uploaded inputs.
 * The RESULTS stay in the layout they were written in: the context records the sampler under which the library last wrote the packed
 * volume (any sweep with MVS_SWEEP_VOLUME) and the windowed volume Wv (mvs_sweep_window); for a caller's volume the layout is unknown
 * until a sweep writes it (mvs_sweep_use_volume).  A reader that would decode cells of a known layout under the other sampler --
 * mvs_sweep_argmin, _refine_depth, _aggregate, _clean (through mvs_sweep_set_volume_source's volume), mvs_sweep_window and
 * mvs_sweep_fetch with a packed_volume_dhw -- returns MVS_ESTATE, names both samplers and changes nothing; switching back makes the cells
 * readable again, and so does the next sweep.  A row band (mvs_sweep_run_rows) or plane group (mvs_sweep_run_planes) written under the
 * other sampler than the rest of the volume leaves cells of both layouts: the readers then return MVS_ESTATE under either sampler until
 * one sweep has written all rows and planes.  mvs_sweep_argmin_partial and mvs_sweep_combine_partials take the caller's pointers and
 * decode them as the current sampler's.  The depth / cost / index maps, S, the clean report and the band depth hold no cells and stay
 * readable. */
#define MVS_SAMPLER_FIXED 0
#define MVS_SAMPLER_EXACT_F32 1
int mvs_sweep_set_sampler(mvs_ctx *ctx, int sampler);
int mvs_sweep_sampler(const mvs_ctx *ctx);

/* Staged form: inputs stay resident in HBM between runs (bench, multi-GPU view sharding). */
int mvs_sweep_set_main(mvs_ctx *ctx, const float main_cam[16], const uint8_t *main_hw);
int mvs_sweep_set_views(mvs_ctx *ctx, int nviews, const float *side_cams, const uint8_t *const *side_frames);
int mvs_sweep_set_planes(mvs_ctx *ctx, int nplanes, float z_lo, float z_hi);
/* The same with frames that already live in the memory of the context's GPU (a decoder's output, a previous stage's result; no counterpart
 * in the reference, whose frames are host cv::Mat: Configuration::frame, configuration.cpp:437-440): H*W u8,
 * tightly packed.  Stream-ordered like a kernel launch: nothing crosses PCIe, nothing synchronises, and the frames are read by work
 * queued on the context's stream -- they must stay unchanged until that work has run (mvs_synchronize, or the caller's own stream
 * order when mvs_set_stream shares a stream).  The side views' quad images are written straight from the raw frames in one pass.
 * (Any of the view setters: when the new set has the view matrices and planes of the last planned one -- a fixed camera rig
 * delivering its next frames -- the region plan in memory is reused; it depends on the cameras, not on the frames.) */
int mvs_sweep_set_main_device(mvs_ctx *ctx, const float main_cam[16], const void *main_dev);
int mvs_sweep_set_views_device(mvs_ctx *ctx, int nviews, const float *side_cams, const void *const *side_frames_dev);

#define MVS_SWEEP_VOLUME 1u       /* materialise the packed cost volume in HBM */
#define MVS_SWEEP_FUSED_ARGMIN 2u /* select depth inside the sweep kernel (no volume read-back pass) */
#define MVS_SWEEP_FORCE_GENERIC 4u /* use the un-tiled global-gather kernel (test / fallback path) */
#define MVS_SWEEP_NO_RECT 8u       /* never take the rectified-view kernels (sweep_fx_rect / sweep_exact_rect); results are bit-identical either way */
/* accumulate views [view_first, view_first + view_count) into the packed volume / fused outputs (async) */
int mvs_sweep_run(mvs_ctx *ctx, int view_first, int view_count, unsigned flags);
/* the same for planes [plane_first, plane_first + plane_count) only (MVS_SWEEP_VOLUME; boundaries on multiples of
 * mvs_sweep_plane_granularity(), the last group may end at nplanes): lets a view-sharded job all-reduce one plane group
 * over xGMI while the next one is being swept (bench.py --shard views --plane-groups G) */
int mvs_sweep_run_planes(mvs_ctx *ctx, int view_first, int view_count, int plane_first, int plane_count, unsigned flags);
int mvs_sweep_plane_granularity(void);
/* the same for pixel rows [row_first, row_first + row_count) only, all planes (any flags; boundaries on multiples of
 * mvs_sweep_row_granularity(), the last band may end at the image height): rows are independent (SURVEY 8e sharding 2),
 * so G ranks sweep one band each of the SAME main view and exchange only the depth rows (bench.py --shard rows).
 * Volume cells and depth / cost / index outside the band are left untouched. */
int mvs_sweep_run_rows(mvs_ctx *ctx, int view_first, int view_count, int row_first, int row_count, unsigned flags);
int mvs_sweep_row_granularity(void);                    /* valid for either sampler (16) */
int mvs_sweep_row_granularity_of(const mvs_ctx *ctx);   /* what the context's current sampler needs (fixed sampler: 8): finer bands balance better */
/* diagnostic: thread shape the region planner chose for the current (views, planes): 0 = no plan yet,
 * 1 = exact sampler, 2 pixels x 32 planes per thread (64x8-pixel tiles), 2 = exact sampler, 4 pixels x 16 planes (64x16 tiles:
 * bit-identical to 1; the choice follows how many warped 32-plane footprints fit the LDS staging buffer), 3 = fixed sampler
 * (2 pixels x 16 planes, 64x8-pixel tiles), 4 = fixed sampler, every side view rectified against the main view (pure translation
 * in its focal plane, equal intrinsics): the kernel sweep_fx_rect (8 pixels x 4 planes per thread, wave-uniform sampling
 * positions; bit-identical to 3, which MVS_SWEEP_NO_RECT selects), 5 = exact sampler on rectified views: the kernel sweep_exact_rect
 * (same thread shape; projection, reciprocal, trunc / fract and frame tests once per (column, plane, view) and per (row, plane, view);
 * bit-identical to 1 / 2).  For the exact sampler the value names what served the LAST run. */
int mvs_sweep_plan_shape(const mvs_ctx *ctx);
/* diagnostic: the fixed sampler reuses its region plan when a new view set has the view matrices, planes and slots of the last planned
 * one (a fixed rig's next frames; the plan depends on the cameras, not on the frames).  enable = 0 makes every view set plan again
 * (bench.py's cold step times the planner that way); results are identical either way.  Default: enabled. */
int mvs_sweep_set_plan_cache(mvs_ctx *ctx, int enable);
/* per-pixel depth selection over the packed volume (async); valid after MVS_SWEEP_VOLUME runs or
 * after the caller has reduced the volume across ranks in place */
int mvs_sweep_argmin(mvs_ctx *ctx);
/* Sub-plane refinement (optional): replaces the selected plane's depth in the depth map by the vertex of
 * the parabola through the mean costs of that plane and its two neighbours (clamped to half a plane step; planes at either end, or
 * with a neighbour that no view sees, keep their depth).  Needs the packed volume and a depth selection of the same run
 * (MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN, or MVS_SWEEP_VOLUME + mvs_sweep_argmin); best cost and index are unchanged.
 * The plane step is what makes two samplers that pick neighbouring planes of equal cost differ by 1/D in depth; refined depths of the
 * two samplers agree to a small fraction of it.
 * Errors: MVS_ESTATE without planes, a packed volume or a depth selection; MVS_ESTATE when the depth selection was made over another
 * plane count than the current one (mvs_sweep_set_planes with a new nplanes since: select again; the same nplanes changes nothing;
 * fused row-band runs over new planes count as a selection once their bands, each touching the last, cover every row);
 * MVS_EINVAL when the caller's volume (mvs_sweep_use_volume) is smaller than nplanes * H * W cells, MVS_ESTATE when the context's own is
 * (allocated for fewer planes).  A refused call launches nothing: the maps are untouched. */
int mvs_sweep_refine_depth(mvs_ctx *ctx);
/* Semi-global aggregation of the packed volume before depth selection (DESIGN.md section 13 is the arithmetic contract; exact integer
 * arithmetic, bit-identical to tests/sgm_mirror.py).  Every cell's matching cost C = min(floor(16 mean cost), cost_cap) in 1/16 grey levels
 * (a cell no view sees: cost_cap, and never selected) is aggregated along `paths` (4 or 8) image directions,
 *   L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d -+ 1) + p1, min_k L_r(p - r, k) + p2) - min_k L_r(p - r, k),
 * the sums S = sum_r L_r (uint16, [nplanes][H][W]) are kept on the device, and the context's depth / cost / index maps are rewritten from
 * them: index = lowest plane with the smallest S among the seen cells, depth = z[index], cost = S / (16 paths) in grey levels; a pixel no
 * view sees gets index -1, MVS_BACKGROUND_DEPTH, +inf (as mvs_sweep_argmin).  MVS_AGGREGATE_REFINE: the parabola of mvs_sweep_refine_depth
 * on S.  Asynchronous on the context's stream, like mvs_sweep_argmin; reads the context's packed volume (its own or the caller's, either
 * sampler) and does not modify it, so mvs_sweep_argmin afterwards restores the winner-take-all maps; everything that consumes the maps
 * (mvs_sweep_fetch, mvs_sweep_depth_device, mvs_depth_upload_device ...) works unchanged.  Timed under MVS_K_ARGMIN.
 * Errors: MVS_EINVAL for a NULL ctx, paths not 4 or 8, p1 < 0, p2 < p1, cost_cap outside 1..4080, paths (cost_cap + p2) > 65535, unknown
 * flag bits, nplanes outside 2..256; MVS_ESTATE without planes or a packed volume; MVS_ENOMEM.  mvs_sweep_aggregated_device: S and its
 * size (NULL before the first call).  mvs_sweep_aggregate_fetch synchronises and downloads S (diagnostic; MVS_ESTATE before the first call). */
#define MVS_AGGREGATE_REFINE 1u
int mvs_sweep_aggregate(mvs_ctx *ctx, int paths, int p1, int p2, int cost_cap, unsigned flags);
void *mvs_sweep_aggregated_device(mvs_ctx *ctx, size_t *bytes);
int mvs_sweep_aggregate_fetch(mvs_ctx *ctx, uint16_t *s_dhw);
/* Cleaning of the selected depth / cost / index maps before they vote into a fusion (DESIGN.md section 16 is the contract; integer
 * arithmetic, bit-identical to tests/clean_mirror.py).  A rejected pixel gets index -1, MVS_BACKGROUND_DEPTH, +inf -- what everything
 * downstream already reads as "empty" -- and every other pixel keeps its three values bit for bit, a refined depth included (so call it
 * after mvs_sweep_refine_depth or MVS_AGGREGATE_REFINE).  With cell = packed volume cell of the pixel's selected plane i, n its count:
 *   rule 1, view count (min_views 0..255; 0 and 1 reject nothing the library selected): rejected when n(i) < min_views;
 *   rule 2, uniqueness (uniqueness_percent u 0..99; 0 = off): of the pixels rule 1 kept, rejected when some plane d that a view sees with
 *     |d - i| >= 2 has score(d) (100 - u) < score(i) 100 (StereoSGBM's uniquenessRatio); the score is the cell's mean cost compared as an
 *     exact rational, s_d n_i (100 - u) < s_i n_d 100 in 64 bits, or with MVS_CLEAN_SCORES_AGGREGATED the sum S of the last
 *     mvs_sweep_aggregate;
 *   rule 3, speckle (speckle_min_size 0 = off; speckle_max_diff 0..255 planes): on the index map rules 1-2 left, 4-neighbours are
 *     connected when both have an index and the indices differ by at most speckle_max_diff; a pixel whose connected component
 *     (transitive closure) has fewer than speckle_min_size pixels is rejected.  All sizes are computed before any pixel is rewritten;
 *     the size map (0 for a pixel without an index) stays on the device for mvs_sweep_clean_sizes_*.
 * Rules 1 and 2 are evaluated on the incoming maps; a pixel that fails rule 1 is counted under rule 1 only.  Asynchronous on the
 * context's stream, like mvs_sweep_argmin, and timed under MVS_K_ARGMIN; the number of launches does not depend on the maps.  Neither the
 * packed volume nor S is modified: mvs_sweep_argmin or mvs_sweep_aggregate afterwards restores the uncleaned maps.  Cleaning twice with
 * the same parameters rejects nothing the second time.  mvs_sweep_clean_report synchronises: pixels with an index before the call, and
 * pixels rejected by rule 1, 2, 3.
 * Errors: MVS_EINVAL for a NULL ctx or array, a parameter outside its range, unknown flag bits; MVS_ESTATE without a depth selection,
 * for a depth selection made over another plane count than the current one (mvs_sweep_set_planes with a new nplanes since), for
 * min_views >= 2 or uniqueness_percent > 0 without a packed volume of nplanes * H * W cells (min_views 1 is tested where the context
 * has one), for MVS_CLEAN_SCORES_AGGREGATED without an S of the current plane count, for mvs_sweep_clean_report before the first clean
 * and for mvs_sweep_clean_sizes_fetch unless the last clean ran rule 3 (mvs_sweep_clean_sizes_device: NULL then); MVS_ENOMEM.  After an error
 * the maps are untouched.  Speckle-only cleaning needs no volume (it works after an MVS_SWEEP_FUSED_ARGMIN run). */
#define MVS_CLEAN_SCORES_AGGREGATED 1u
int mvs_sweep_clean(mvs_ctx *ctx, int min_views, int uniqueness_percent, int speckle_min_size, int speckle_max_diff, unsigned flags);
int mvs_sweep_clean_report(mvs_ctx *ctx, int out[4]);
void *mvs_sweep_clean_sizes_device(mvs_ctx *ctx);
int mvs_sweep_clean_sizes_fetch(mvs_ctx *ctx, int32_t *sizes_hw);
/* Windowed matching cost: gated box aggregation of the packed volume (csrc/window.hip; DESIGN.md section 18 is the arithmetic contract;
 * exact integer arithmetic, bit-identical to tests/window_mirror.py).  A cell of the packed volume is the cost of ONE pixel; the windowed
 * volume Wv holds, in the same cell format, the mean cost over a support window.  For pixel p and plane d the window is every pixel q of
 * the frame with |q.row - p.row| <= radius and |q.col - p.col| <= radius whose guide value is close to p's, |G(q) - G(p)| <= tau (p
 * itself always is; tau = 255 is the plain box and G is not read).  With S and N the sums of the members' cost sums and view counts (a
 * member no view sees adds nothing) and n the pixel's own count, the cell of Wv is  n << CS | floor(S n / N)  (exact 64-bit integers), or
 * 0 when n = 0: a hypothesis no view sees stays unseen.  The count field still is the pixel's own view count, the mean cost of the cell is
 * the window's mean cost, so every reader of the packed volume works on Wv unchanged; radius 0 reproduces the volume cell for cell.
 *   mvs_sweep_window reads the context's packed volume (its own or the caller's, either sampler), never modifies it, and writes every
 * cell of Wv, a context-owned buffer of nplanes * H * W cells allocated by the first call.  guide_dev: H * W u8 on the context's GPU, NULL =
 * the staged main image (mvs_sweep_set_main or the frame-store slot of mvs_sweep_handles).  Asynchronous on the context's stream, timed
 * under MVS_K_ARGMIN.  MVS_WINDOW_SELECT: the same pass also rewrites the depth / cost / index maps with what mvs_sweep_argmin gives on Wv
 * (lowest mean cost as an exact rational, ties to the lowest plane; -1 / MVS_BACKGROUND_DEPTH / +inf for a pixel nothing sees);
 * MVS_WINDOW_REFINE (with SELECT): the depth map is what mvs_sweep_refine_depth then gives on Wv.  Both are bit-identical to the two-step
 * form and cost no second read of the volume.
 *   mvs_sweep_set_volume_source chooses the packed volume that mvs_sweep_argmin, mvs_sweep_refine_depth, mvs_sweep_aggregate (its matching
 * cost C) and mvs_sweep_clean (rules 1 and 2) read: MVS_VOLUME_RAW (default) or MVS_VOLUME_WINDOWED (Wv).  Everything else --
 * mvs_sweep_volume_device, mvs_sweep_fetch, mvs_sweep_use_volume, the sweep itself, the partial / combine pair, the communicator -- keeps
 * meaning the raw volume.  The source survives sweeps and changes only through the setter.
 * Errors: MVS_EINVAL for a NULL ctx, radius outside 0..4, tau outside 0..255, unknown flag bits, MVS_WINDOW_REFINE without
 * MVS_WINDOW_SELECT, an unknown source, a NULL array for the fetch; MVS_ESTATE without planes or a packed volume of nplanes * H * W cells,
 * for tau < 255 (and radius > 0) with a NULL guide and no staged main image, for mvs_sweep_window_fetch before the first window, and for
 * any of the four readers under MVS_VOLUME_WINDOWED while there is no Wv of the current plane count; MVS_ENOMEM.  After an error nothing
 * is written and the context stays usable.  mvs_sweep_windowed_device: Wv and its size (NULL before the first call);
 * mvs_sweep_window_fetch synchronises and downloads Wv (diagnostic). */
#define MVS_WINDOW_SELECT 1u
#define MVS_WINDOW_REFINE 2u
int mvs_sweep_window(mvs_ctx *ctx, int radius, int tau, const void *guide_dev, unsigned flags);
void *mvs_sweep_windowed_device(mvs_ctx *ctx, size_t *bytes);
int mvs_sweep_window_fetch(mvs_ctx *ctx, uint32_t *cells_dhw);
#define MVS_VOLUME_RAW 0
#define MVS_VOLUME_WINDOWED 1
int mvs_sweep_set_volume_source(mvs_ctx *ctx, int source);
int mvs_sweep_volume_source(const mvs_ctx *ctx);
/* Band sweep: the planes in a per-pixel band around a depth prior (csrc/band.hip; DESIGN.md section 19 is the arithmetic contract; all
 * f32, one rounding per operation, bit-identical to tests/band_mirror.py).  Fixed sampler only.  Plane d of pixel p is
 * z = prior(p) + delta_d, so the planes are spent where a coarser result -- a coarse sweep's refined map, mvs_depth of a proxy mesh,
 * mvs_tsdf_raycast -- says the surface is.
 *   1. Prior: prior_dev is H * W f32 on the context's GPU in the library's depth convention for the main camera.  A pixel has a prior when
 *      -1 < z0 < 1 (NaN has none).  The call copies the map into a context-owned buffer (device to device, on the context's stream;
 *      allocated by the first call), so prior_dev may be mvs_sweep_depth_device(ctx) itself.
 *   2. Offsets: delta is the context's plane table, mvs_sweep_set_planes(ctx, D, lo, hi) with -1 < lo < hi < 1, typically (-hb, +hb).
 *      z_d(p) = z0 + delta_d is one f32 add; plane d of pixel p is live when -1 < z_d(p) < 1.
 *   3. Cell: for a pixel with a prior and a live plane, the sum of (1 << 24) + |dot - 255 I_main| over the views of
 *      [view_first, view_first + view_count) that the fixed sampler's sample at (xn, yn, z_d(p)) finds in frame -- the sample of
 *      mvs_sweep_run, bit for bit; otherwise 0.  Layout [D][H][W] u32 in the context's packed volume (its own or the caller's); as in
 *      mvs_sweep_run the cells are the sums of the listed views, not added to what was there.
 *   4. Selection: MVS_SWEEP_FUSED_ARGMIN gives what mvs_sweep_argmin gives on that volume with the table delta: lowest mean cost as an
 *      exact rational, ties to the lowest plane, cost and index as usual, -1 / MVS_BACKGROUND_DEPTH / +inf for a pixel with no seen cell.
 *      THE DEPTH MAP HOLDS OFFSETS: delta[index], not depths, after a band run and after every re-selection on its volume
 *      (mvs_sweep_argmin, _refine_depth, _window, _aggregate, _clean: all work in the index domain and run unchanged), until resolved.
 *      An offset never is 1.0 for a selected pixel (hi < 1, and refinement moves at most half a step).  A band run without
 *      MVS_SWEEP_FUSED_ARGMIN leaves the context WITHOUT a depth selection (the index map is not one on this volume) until
 *      mvs_sweep_argmin or another selecting call.
 *   5. Resolve: mvs_sweep_band_resolve writes band_depth, a separate context-owned H * W f32 map: for a pixel with index >= 0,
 *      z = z0 + depth(p) in one add, written if -1 < z < 1, else MVS_BACKGROUND_DEPTH; MVS_BACKGROUND_DEPTH for index < 0.  The depth /
 *      cost / index maps are not modified, so the call is idempotent and can follow any re-selection.  The same kernel counts, for
 *      mvs_sweep_band_report: out[0] pixels with a prior, [1] pixels with an index, [2] pixels whose index is 0 or D - 1 ("band edge":
 *      the sign of a band too narrow for its prior), [3] pixels emptied by the range test.
 * mvs_sweep_run_band works on the context's staged state however it got there (mvs_sweep_set_main / _views, host or device forms, or the
 * slots left staged by mvs_sweep_handles); flags: MVS_SWEEP_VOLUME and / or MVS_SWEEP_FUSED_ARGMIN.  It is asynchronous on the context's
 * stream and timed under MVS_K_SWEEP; mvs_sweep_band_resolve is asynchronous and timed under MVS_K_ARGMIN; mvs_sweep_band_fetch and
 * mvs_sweep_band_report synchronise.  mvs_sweep_band_depth_device: band_depth (NULL before the first resolve), e.g. for
 * mvs_depth_upload_device(ctx, slot, cam, mvs_sweep_band_depth_device(ctx), mvs_sweep_cost_device(ctx)); mvs_sweep_band_prior_device: the
 * context's copy of the prior (NULL before the first band run).  A wrong prior confines the band to the wrong place: outliers of the
 * prior stay outliers.
 * Errors: MVS_EINVAL for a NULL ctx, prior or array, a view range outside 0..V, flags that select neither output, unknown flag bits
 * (MVS_SWEEP_FORCE_GENERIC and MVS_SWEEP_NO_RECT are unknown here); MVS_ESTATE without main view, views or planes, for a plane table not
 * inside (-1, 1), for the exact sampler; MVS_ESTATE from resolve, fetch and report before a band run, after an ordinary mvs_sweep_run*
 * or a new prior (mvs_pyramid_prior into this context's prior buffer) since, without a depth selection over the current plane count, when the plane count has changed since the band run, and from fetch and
 * report before the band run's resolve; MVS_ENOMEM.  After an error nothing is written and the context stays usable. */
int mvs_sweep_run_band(mvs_ctx *ctx, int view_first, int view_count, const void *prior_dev, unsigned flags);
int mvs_sweep_band_resolve(mvs_ctx *ctx);
void *mvs_sweep_band_depth_device(mvs_ctx *ctx);
void *mvs_sweep_band_prior_device(mvs_ctx *ctx);
int mvs_sweep_band_fetch(mvs_ctx *ctx, float *depth_hw);
int mvs_sweep_band_report(mvs_ctx *ctx, int out[4]);
/* ZNCC sweep: zero-mean normalised cross-correlation over a support window as the matching cost (csrc/zncc.hip; DESIGN.md section 21 is
 * the arithmetic contract; the window sums are exact integers, the last steps f32 with one rounding per operation and no contraction;
 * bit-identical to tests/zncc_mirror.py).  Fixed sampler only.  The cost of mvs_sweep_run, |dot - 255 I_main|, assumes that a surface
 * point has the same grey level in every frame; this one is invariant to a local affine change of intensity (exposure, vignetting).
 * The planes are the context's plane table z_d, the views [view_first, view_first + view_count), radius 1..4.
 *   1. Warped grey level: for pixel q, plane d, view v the fixed sampler's sample at (xn(q), yn(q), z_d) -- the sample of mvs_sweep_run,
 *      bit for bit -- has a frame test ok(q) and a weighted sum dot; B(q) = (dot + 127) / 255 in integer division, the grey level
 *      mvs_warp_by_depth returns with the fixed sampler.  A(q) is the staged main image.
 *   2. Members: for the centre pixel p the window M is every pixel q of the frame with |q.row - p.row| <= radius,
 *      |q.col - p.col| <= radius and ok(q); pixels outside the frame are no members.  The view counts for the cell only if ok(p).
 *   3. Sums over M: N = |M|, Sa, Sb, Sab, Saa, Sbb of A, B, A B, A A, B B; cov = N Sab - Sa Sb, va = N Saa - Sa Sa, vb = N Sbb - Sb Sb
 *      (all below 2^31 at radius 4).  The view counts only if va > 0 and vb > 0: a flat patch carries no correlation and is treated
 *      like a sample out of frame.
 *   4. Cost of a counted view: den = sqrtf((float)va * (float)vb); ncc = (float)cov / den, clamped to [-1, 1];
 *      c = (uint32)floorf(32512.0f * (1.0f - ncc)), 0..65024.
 *   5. Cell: the sum of (1 << 24) + c over the counted views of the listed range, 0 if there are none; layout [D][H][W] u32 in the
 *      context's packed volume (its own or the caller's).  As in mvs_sweep_run the cells are the sums of the listed views, not added to
 *      what was there; the volumes of disjoint view ranges add as u32, so the view-sharded reductions stay valid.
 *   6. Reading the cost map: every reader takes a cell's mean cost as sum / (255 count), so the cost map reads 127.5 (1 - ncc) "grey
 *      levels": 0 is perfect correlation, 127.5 none, 255 inverted.  That is the scale of mvs_fuse_depth's max_cost, of
 *      mvs_sweep_aggregate's cost_cap (in 1/16 of it) and of what mvs_sweep_clean's uniqueness_percent compares on this volume.
 *   7. Selection: MVS_SWEEP_FUSED_ARGMIN gives what mvs_sweep_argmin gives on that volume (lowest mean as an exact rational, ties to the
 *      lowest plane, -1 / MVS_BACKGROUND_DEPTH / +inf where nothing is counted) and records a full selection over the current plane
 *      count; without the flag the context has no depth selection until a selecting call, as after a band run.
 * For every later call it is an ordinary sweep (mvs_sweep_argmin, _refine_depth, _window, _aggregate, _clean, the depth store and the TSDF
 * run on its result unchanged; it ends a band run's state exactly as mvs_sweep_run does).  It works on the staged state however it got
 * there (host setters, the _device forms, the slots left staged by mvs_sweep_handles), is asynchronous on the context's stream and timed
 * under MVS_K_SWEEP.  A context that never calls it allocates nothing for it.
 * Errors: MVS_EINVAL for a NULL ctx, radius outside 1..4, a view range outside 0..V, flags that select neither output, unknown flag bits
 * (MVS_SWEEP_FORCE_GENERIC and MVS_SWEEP_NO_RECT are unknown here), a caller's volume that is too small; MVS_ESTATE without main view,
 * views or planes, for the exact sampler; MVS_ENOMEM.  After an error nothing is written and the context stays usable. */
int mvs_sweep_run_zncc(mvs_ctx *ctx, int view_first, int view_count, int radius, unsigned flags);
/* Occlusion-robust sweep: the cell keeps the K best views (csrc/bestk.hip; DESIGN.md section 22 is the contract; integers throughout
 * except rule 4 of the ZNCC cost; bit-identical to tests/bestk_mirror.py).  Fixed sampler only.  Every other sweep merges the side views
 * of a cell by summing their costs, so a view in which a nearer surface hides the point adds a wrong cost; next to a depth step the sum
 * then picks the wrong plane.  This one merges only the `keep` lowest per-view costs of the cell (Kang and Szeliski's best-half rule).
 * The planes are the context's plane table, the views [view_first, view_first + view_count).
 *   1. Per-view cost of (pixel p, plane d, view v), a flag `counted` and an integer c:
 *      MVS_COST_ZNCC, radius 1..4: counted and c (0..65024) exactly as rules 1-4 of mvs_sweep_run_zncc.
 *      MVS_COST_ABSDIFF, radius 0..4: e(q) = |dot(q) - 255 A(q)| and ok(q) are mvs_sweep_run's own sample at every pixel q, bit for bit.
 *      The members M are the pixels q of the frame with |q.row - p.row| <= radius, |q.col - p.col| <= radius and ok(q); pixels outside
 *      the frame are no members.  The view is counted iff ok(p).  N = |M|, S = the sum of e over M (at most 81 * 65025, below 2^23),
 *      c = S / N in integer division, 0..65025; no float is used anywhere.  At radius 0, c = e(p).
 *   2. Cell: n = the number of counted views of the range, k = min(keep, n); the cell is k << 24 | (the sum of the k smallest c), and 0
 *      if n = 0.  The sum of the k smallest values does not depend on how equal values are ordered: there is no tie rule.  keep is 1..8,
 *      or MVS_KEEP_ALL (0) for every counted view: with MVS_COST_ZNCC that is mvs_sweep_run_zncc's volume, with MVS_COST_ABSDIFF at
 *      radius 0 mvs_sweep_run's.  Layout [D][H][W] u32 in the context's packed volume (its own or the caller's), written, not added to.
 *   3. The cell keeps the packed format and its scale (mean cost = sum / (255 count), rule 6 of mvs_sweep_run_zncc for the ZNCC cost), so
 *      mvs_sweep_argmin, _refine_depth, _window, _aggregate, _clean, the depth store and the TSDF run on it unchanged, and
 *      MVS_SWEEP_FUSED_ARGMIN gives what mvs_sweep_argmin gives on that volume and records a full selection; without the flag the context
 *      has no depth selection until a selecting call.  It ends a band run's state exactly as mvs_sweep_run does.
 *   4. Unlike the summing sweeps, the volumes of disjoint view ranges DO NOT ADD: the k best of a range are not the k best of its parts.
 *      mvs_comm's view-sharded modes must not be fed with it; the rows mode needs nothing.
 * Use it with a window: the minimum over views of a single-pixel cost is mostly texture aliasing, and best-K of them is WORSE than the
 * sum (DESIGN.md section 22 has the figures).  Radius 0 exists as a cross-check against mvs_sweep_run.
 * It works on the staged state however it got there, is asynchronous on the context's stream and timed under MVS_K_SWEEP.  A context that
 * never calls it allocates nothing for it.
 * Errors: MVS_EINVAL for a NULL ctx, an unknown cost, a radius outside the cost's range (0 with MVS_COST_ZNCC is one), keep outside 0..8,
 * a view range outside 0..V, flags that select neither output, unknown flag bits (MVS_SWEEP_FORCE_GENERIC and MVS_SWEEP_NO_RECT are
 * unknown here), a caller's volume that is too small; MVS_ESTATE without main view, views or planes, for the exact sampler; MVS_ENOMEM.
 * After an error nothing is written and the context stays usable. */
#define MVS_COST_ABSDIFF 0   /* windowed |dot - 255 I_main| */
#define MVS_COST_ZNCC    1   /* rules 1-4 of mvs_sweep_run_zncc */
#define MVS_KEEP_ALL     0   /* keep: every counted view */
int mvs_sweep_run_bestk(mvs_ctx *ctx, int view_first, int view_count, int cost, int radius, int keep, unsigned flags);
/* mvs_sweep_run_bestk with a guide-gated support window (csrc/bestk_gated.hip; DESIGN.md section 26 is the contract; bit-identical to
 * tests/gated_mirror.py).  Fixed sampler only.  Beside a depth step the square window of p holds pixels of the other surface; where the
 * step coincides with an edge of a guide image G, the gate takes them out: G is the H x W u8 image at guide_dev (on the context's GPU,
 * read during the call's kernel), or the staged main image when guide_dev is NULL.
 *   Rule 1 of mvs_sweep_run_bestk changes in one place: q is a member of M(p) iff it is inside the frame within the window, ok(q), and
 *   |G(q) - G(p)| <= tau.  p passes its own gate; the gate depends on neither plane nor view.  Everything else is rules 3-4 of
 *   mvs_sweep_run_zncc and rules 1-4 of mvs_sweep_run_bestk over that M: the same exact integers, the same one-rounding f32, the same packed
 *   cell, maps and state afterwards.  A view counts iff ok(p) and, for MVS_COST_ZNCC, va > 0 and vb > 0 over the gated members.
 * radius is 1..4 for both costs (radius 0 has no window to gate), tau 0..255, keep 1..8 or MVS_KEEP_ALL; MVS_COST_ZNCC with MVS_KEEP_ALL is
 * the gated ZNCC sweep.  tau = 255, or a constant guide at any tau, writes mvs_sweep_run_bestk's bytes.
 * WARNING: a tau below the texture's own contrast takes most members out, and ZNCC then has little or no variance left to correlate (a view
 * whose gated va or vb is 0 does not count): on the occluder scene tau 15 is worse than tau 30 with keep 2.  Choose
 * tau between the texture's contrast and the contrast across the edges that matter.
 * The window is not separable, so a pixel reads (2 radius + 1)^2 elements per (plane, view) where mvs_sweep_run_bestk reads about
 * 2 (2 radius + 1).  Asynchronous on the context's stream, timed under MVS_K_SWEEP; it allocates nothing of its own.
 * Errors: those of mvs_sweep_run_bestk, and MVS_EINVAL for radius 0 and for tau outside 0..255.  Every check comes before the first
 * allocation; after an error nothing is written and the context stays usable. */
int mvs_sweep_run_bestk_gated(mvs_ctx *ctx, int view_first, int view_count, int cost, int radius, int keep, int tau, const void *guide_dev, unsigned flags);
/* Band sweep with windowed costs: mvs_sweep_run_bestk with plane d of pixel q at prior(q) + delta_d (csrc/bestk.hip; DESIGN.md
 * section 24 is the contract; bit-identical to tests/band_bestk_mirror.py).  Fixed sampler only.  It joins the band sweep's planes, spent
 * where a prior says the surface is, with the matching costs that survive exposure drift (ZNCC) and occlusion (best-K), so that the
 * coarse-to-fine paths can run on frames on which the absolute difference fails.  MVS_COST_ZNCC with MVS_KEEP_ALL is the ZNCC band sweep.
 *   1. Prior and planes: rules 1-2 of mvs_sweep_run_band.  A pixel q has a prior when -1 < prior(q) < 1; z_d(q) = prior(q) + delta_d is one
 *      f32 add, delta the context's plane table inside (-1, 1); plane d is live at q when q has a prior and -1 < z_d(q) < 1.
 *   2. Sample: ok(q) and dot(q) of (q, d, v) are the fixed sampler's sample of mvs_sweep_run, bit for bit, at (xn(q), yn(q), z_d(q)).  A q
 *      outside the frame, without a prior or on a dead plane is not ok.  EVERY WINDOW MEMBER IS SAMPLED AT ITS OWN PRIOR: the window
 *      follows the prior surface, a slanted support window where the prior is smooth.
 *   3. Per-view cost of (p, d, v): rule 1 of mvs_sweep_run_bestk on those samples -- the ZNCC cost (rules 1-4 of mvs_sweep_run_zncc,
 *      B(q) = (dot(q) + 127) / 255; radius 1..4) or the integer mean of |dot(q) - 255 A(q)| over the members (radius 0..4).  The members
 *      are the q of the window with ok(q); the view counts iff ok(p), and for ZNCC also va > 0 and vb > 0.
 *   4. Cell: rule 2 of mvs_sweep_run_bestk, k << 24 | (the sum of the k smallest c), keep 1..8 or MVS_KEEP_ALL; layout [D][H][W] u32 in the
 *      context's packed volume (its own or the caller's), written, not added to.  The volumes of disjoint view ranges add only with
 *      MVS_KEEP_ALL.
 *   5. Selection and state: rules 4-5 of mvs_sweep_run_band unchanged.  MVS_SWEEP_FUSED_ARGMIN gives what mvs_sweep_argmin gives on that
 *      volume; THE DEPTH MAP HOLDS OFFSETS.  The call copies the prior into the context's prior buffer, so prior_dev may be
 *      mvs_sweep_depth_device(ctx), mvs_sweep_band_prior_device(ctx) (no copy) or mvs_depth_filtered_device(ctx).  It leaves the band
 *      state exactly as mvs_sweep_run_band does: mvs_sweep_band_resolve / _report / _fetch, mvs_sweep_argmin, _refine_depth, _window,
 *      _aggregate, _clean and mvs_pyramid_prior work on it unchanged, and an ordinary sweep ends it.
 * Three identities hold bit for bit: with prior == 0.0 everywhere the volume is mvs_sweep_run_bestk's on the same table; MVS_COST_ABSDIFF
 * at radius 0 with MVS_KEEP_ALL gives mvs_sweep_run_band's volume; MVS_COST_ZNCC with MVS_KEEP_ALL and prior == 0.0 gives
 * mvs_sweep_run_zncc's.
 * A wrong prior confines the band to the wrong place, and a windowed cost makes that worse, not better: on a RAW coarse map the windowed
 * band is worse than the global windowed sweep at equal samples; filter the prior first (mvs_depth_filter; DESIGN.md section 24 has the
 * figures).  Asynchronous on the context's stream, timed under MVS_K_SWEEP.  A context that never calls it allocates nothing for it.
 * Errors: MVS_EINVAL for a NULL ctx or prior, an unknown cost, a radius outside the cost's range, keep outside 0..8, a view range outside
 * 0..V, flags that select neither output, unknown flag bits, a caller's volume that is too small; MVS_ESTATE without main view, views or
 * planes, for a plane table not inside (-1, 1), for the exact sampler; MVS_ENOMEM.  After an error nothing is written and the context
 * stays usable. */
int mvs_sweep_run_band_bestk(mvs_ctx *ctx, int view_first, int view_count, const void *prior_dev, int cost, int radius, int keep, unsigned flags);
/* Resolution pyramid: a half-resolution coarse level for the band sweep (csrc/pyramid.hip; DESIGN.md section 20 is the contract;
 * bit-identical to tests/pyramid_mirror.py).  The levels are separate contexts on the SAME GPU: `fine` is W x H with W and H even,
 * `coarse` exactly (W/2) x (H/2).  The cameras are NDC matrices and the centre of a coarse pixel is the mean of the centres of its four
 * fine pixels, so the same 4 x 4 matrices serve every level.  Fixed sampler.  Opt-in: a context that never calls these allocates nothing
 * and behaves bit for bit as before.
 *   Rule D (frames, exact integers): coarse[r][c] = (f[2r][2c] + f[2r][2c+1] + f[2r+1][2c] + f[2r+1][2c+1] + 2) >> 2.
 *   Rule U (prior, f32, one rounding per operation, no contraction): for fine pixel (r, c), r0 = (r - 1) >> 1 (arithmetic shift),
 *      r1 = r0 + 1, both clamped to [0, H/2 - 1]; row weights wy0 = (r & 1) ? 3 : 1, wy1 = 4 - wy0; columns alike.  The four taps, in the
 *      order (r0,c0), (r0,c1), (r1,c0), (r1,c1), have the integer weights w = wy * wx (a clamped tap keeps its weight).  A tap is valid
 *      when -1 < z < 1 (false for NaN).  With tau < 255 a valid tap is a member when |Gc(tap) - Gf(r, c)| <= tau, Gc and Gf being the
 *      staged main images of the coarse and the fine context; if no valid tap is a member, every valid tap is one.  With tau = 255 the
 *      guides are not read and every valid tap is a member.  num = the sum of (float)w * z over the members in tap order, starting at
 *      the first member's product; z = num / (float)(sum of the members' w); the output is z if -1 < z < 1, else MVS_BACKGROUND_DEPTH,
 *      and MVS_BACKGROUND_DEPTH without a valid tap.
 *   mvs_pyramid_downsample_device(fine, src, dst, n)   rule D on n (1..65535) tightly packed W x H frames on fine's GPU into n tightly
 *      packed (W/2) x (H/2) frames, one launch, asynchronous on fine's stream; MVS_EINVAL when the two ranges overlap.
 *   mvs_pyramid_stage(fine, coarse)   stages on `coarse` the rule-D copy of what is staged on `fine` -- the main image as the sweep reads
 *      it, every side view, the same cameras -- however it got there: mvs_sweep_set_main / _views, the _device forms, mvs_sweep, the slots
 *      left staged by mvs_sweep_handles, or an earlier mvs_pyramid_stage (full -> 1/2 -> 1/4 works).  The frames go into a coarse-owned
 *      buffer of (V + 1)(W/2)(H/2) bytes allocated by the first call; the call then is mvs_sweep_set_main_device +
 *      mvs_sweep_set_views_device on `coarse` with those frames, so the coarse context's state is byte for byte that of those two calls
 *      and the plan cache applies.  The planes stay the caller's: mvs_sweep_set_planes(coarse, ...).
 *   mvs_pyramid_prior(fine, coarse, coarse_depth_dev, tau)   rule U on coarse_depth_dev, (H/2)(W/2) f32 on the GPU -- NULL: the coarse
 *      context's depth map (mvs_sweep_depth_device(coarse), after a refined sweep); mvs_sweep_band_depth_device(coarse) when the coarse
 *      level was itself a band level -- into the fine context's own prior buffer, the one mvs_sweep_band_prior_device(fine) returns
 *      (allocated if need be), so mvs_sweep_run_band(fine, v0, n, mvs_sweep_band_prior_device(fine), flags) runs without a copy.
 *      That buffer is also the prior of fine's LAST band run, which mvs_sweep_band_resolve adds the offsets to: the call therefore ENDS
 *      that band run, resolved or not -- mvs_sweep_band_resolve, _fetch and _report return MVS_ESTATE until the next band run (fetch a
 *      resolved map before asking for the next prior).  The maps, the volume and the selection of `fine` stay as they are.
 * Ordering between the two contexts' streams is the library's job: a kernel that reads one context's buffers and writes the other's
 * runs on the consumer's stream behind an event recorded on the producer's stream, and the producer's stream then waits for an event
 * recorded behind that kernel, so the producer's next work cannot overwrite what is still being read.  The events are created once per
 * context, without timing; nothing synchronises the host.  mvs_pyramid_downsample_device and mvs_pyramid_stage are timed under
 * MVS_K_PROJECT (the stage's launches in the coarse context's profile), mvs_pyramid_prior under MVS_K_ARGMIN (in the fine context's).
 * Errors: MVS_EINVAL for a NULL context or source, fine == coarse, contexts on different devices, W or H odd, a coarse context that is
 * not exactly (W/2, H/2), tau outside 0..255, nframes out of range, overlapping ranges; MVS_ESTATE from mvs_pyramid_stage without a main
 * view and side views on `fine` or with the exact sampler on either context, from mvs_pyramid_prior with a NULL coarse_depth_dev and no
 * depth map on `coarse`, or with tau < 255 and no staged main image on either context; MVS_ENOMEM.  After an error nothing is written and
 * both contexts stay usable (the message is on `fine`). */
int mvs_pyramid_downsample_device(mvs_ctx *fine, const void *src_dev, void *dst_dev, int nframes);
int mvs_pyramid_stage(mvs_ctx *fine, mvs_ctx *coarse);
int mvs_pyramid_prior(mvs_ctx *fine, mvs_ctx *coarse, const void *coarse_depth_dev /* NULL: coarse's depth map */, int tau);
/* Depth-map filter: a gated median and a gated mean of a selected depth map (csrc/depth_filter.hip; DESIGN.md section 23 is the contract;
 * all f32, one rounding per operation and no contraction, bit-identical to tests/depth_filter_mirror.py).  The windowed costs assume a
 * fronto-parallel surface inside their window, so the depth they select on a slanted surface is biased and noisy, and the band sweep's
 * window follows its prior: a smooth prior makes it a slanted support window.  This smooths a map without crossing the edges of a guide
 * image or of the map itself, and fills the holes mvs_sweep_clean leaves.
 *   1. Valid: a value z of the map is valid when -1 < z < 1 (NaN, +-inf, -1 and 1 are not) and is read as z + 0.0f (-0.0 becomes +0.0).
 *   2. Window of pixel p: every pixel q of the frame with |q.row - p.row| <= radius and |q.col - p.col| <= radius, in row-major order.
 *      Guide gate: |G(q) - G(p)| <= tau in integers (p itself always passes; tau = 255 lets every pixel pass and G is not read).
 *   3. Median stage (MVS_FILTER_MEDIAN): the members of p are the valid q that pass the guide gate, n their number.  A valid p gets the
 *      lower median, the member of rank (n - 1) / 2 in ascending order.  An invalid p gets MVS_BACKGROUND_DEPTH; with MVS_FILTER_FILL and
 *      n >= min_members it gets the lower median of its members instead.  No arithmetic: the output is one of the inputs.
 *   4. Mean stage (MVS_FILTER_MEAN), on the median stage's output m when both flags are given, else on the input: for a valid p the
 *      members are the valid q that pass the guide gate and the depth gate fabsf(m(q) - m(p)) <= max_step (+inf: no depth gate, 0: equal
 *      values only); the output is (the sum of the members, added one at a time in window order starting from 0.0f) / (float)n.  An
 *      invalid p stays MVS_BACKGROUND_DEPTH: holes are filled by the median stage only.
 *   5. The output holds 1.0 only as background and never -1.0: a mean of values inside (-1, 1) stays inside.
 * max_step is in depth units: a few plane steps of the sweep that selected the map.  A max_step below the surface's own change of depth
 * across the window cuts a slanted surface into terraces and makes it worse than no filter (DESIGN.md section 23 has the figures).
 *   depth_dev: H * W f32 on the context's GPU in the library's depth convention -- mvs_sweep_depth_device, mvs_sweep_band_depth_device,
 * mvs_tsdf_raycast_depth_device, mvs_depth_slot_device, mvs_depth_filtered_device itself (the filtered map of an earlier call), or a band
 * run's offset map (its values lie inside (-1, 1)).  guide_dev: H * W u8, NULL = the staged main image, exactly as in mvs_sweep_window.
 * The filtered map is a context-owned H * W f32 map, allocated by the first call together with one intermediate map; a context that
 * never calls the filter allocates nothing.  Asynchronous on the context's stream, timed under MVS_K_ARGMIN.  The call touches no other
 * state: the sweep's depth / cost / index maps, the selection state, the band state and the volume source are as they were.
 * Errors: MVS_EINVAL for a NULL ctx, depth_dev or fetch array, a radius outside 1..4, tau outside 0..255, a negative or NaN max_step,
 * flags with neither stage or with unknown bits, MVS_FILTER_FILL without MVS_FILTER_MEDIAN, min_members outside 1..81 with
 * MVS_FILTER_FILL (ignored without); MVS_ESTATE for tau < 255 with a NULL guide and no staged main image, and for
 * mvs_depth_filter_fetch before the first call; MVS_ENOMEM.  After an error nothing is written and the context stays usable.
 * mvs_depth_filtered_device: the filtered map (NULL before the first call; the address does not change afterwards);
 * mvs_depth_filter_fetch synchronises and downloads it. */
#define MVS_FILTER_MEDIAN 1u
#define MVS_FILTER_MEAN 2u
#define MVS_FILTER_FILL 4u
int mvs_depth_filter(mvs_ctx *ctx, const void *depth_dev, const void *guide_dev /* NULL: the staged main image */, int radius, int tau, float max_step, int min_members,
                     unsigned flags);
void *mvs_depth_filtered_device(mvs_ctx *ctx);
int mvs_depth_filter_fetch(mvs_ctx *ctx, float *depth_hw);
/* Hypothesis propagation: PatchMatch refinement of a depth map (csrc/propagate.hip; DESIGN.md section 25 is the contract; bit-identical
 * to tests/propagate_mirror.py).  Every other estimator scores the hypotheses of a plane table; here every pixel carries a depth and a
 * slope, tests the hypotheses of its neighbours and a few perturbations of its own, and keeps what matches best: good hypotheses spread
 * into bad regions, depth is continuous, the window lies on a slanted plane and no D x H x W volume exists.  Fixed sampler only.  All f32
 * arithmetic below has one rounding per operation and no FMA, except inside the sampler.
 *   State per pixel p: a hypothesis (z, gx, gy) -- NDC depth at the pixel centre, its change per column and per row -- and a packed cell
 * k << 24 | sum in mvs_sweep_run_bestk's format.  p has a hypothesis when -1 < z < 1; without one it holds exactly MVS_BACKGROUND_DEPTH,
 * 0, 0 and cell 0.
 *   1. Member depth: for the hypothesis (z, gx, gy) at p and window member q, dc = q.col - p.col, dr = q.row - p.row:
 *      z_q = (z + gx (float)dc) + gy (float)dr.  q is live when it is inside the frame and -1 < z_q < 1 (false for NaN).
 *   2. Sample: ok(q) and dot(q) of view v are the fixed sampler's sample of mvs_sweep_run at (xn(q), yn(q), z_q), bit for bit; a member
 *      that is not live is not ok.
 *   3. Per-view cost and cell: rules 1 and 2 of mvs_sweep_run_bestk on those samples -- MVS_COST_ZNCC (radius 1..4) or MVS_COST_ABSDIFF
 *      (radius 0..4), keep 1..8 or MVS_KEEP_ALL -- over the views [view_first, view_first + view_count) given to init.  The plane table
 *      is not read and not required.
 *   4. Better: cell c beats cell b iff c >> 24 != 0 and (b == 0 or s_c k_b < s_b k_c): the depth selection's rule.  It is strict, so a
 *      tie keeps the earlier hypothesis.
 *   5. mvs_propagate_init copies depth_dev (H * W f32 on the context's GPU: any map in the library's depth convention, or the stage's own
 *      z map) into z, invalid values as MVS_BACKGROUND_DEPTH.  Slopes are 0; with MVS_PROPAGATE_SLOPES gx = (z(col + 1) - z(col - 1)) 0.5f
 *      when both neighbours are usable, else the one-sided difference z(col + 1) - z(col) or z(col) - z(col - 1), else 0, and gy likewise
 *      along rows; a neighbour is usable when it has a hypothesis and fabsf(z_n - z_p) <= max_step (INFINITY: no gate; max_step is
 *      ignored without the flag but must not be negative or NaN).  Then every pixel's cell is evaluated (rules 1-3), cost, radius, keep
 *      and the view range are recorded and the iteration counter is set to 0.
 *   6. mvs_propagate_run runs `iterations` >= 1 iterations.  Iteration t, counted from init, has the halves h = 0, 1; in half h the
 *      pixels with (row + col + h) & 1 == 0 are active.  They read neighbours at odd Manhattan distance only, which are inactive, so a
 *      half is free of races in place.  An active pixel walks this list and takes every candidate that is better (rule 4) than what it
 *      holds at that moment:
 *        near: the offsets (dc, dr) = (-1, 0), (1, 0), (0, -1), (0, 1); far: (-5, 0), (5, 0), (0, -5), (0, 5).  If n = p + (dc, dr) is
 *          inside the frame and has a hypothesis, whatever its cell, the candidate is z' = (z_n - gx_n (float)dc) - gy_n (float)dr with
 *          gx_n, gy_n: the neighbour's plane extended to p.
 *        random j = 0 .. nrandom - 1 (nrandom 0..4), only if the pixel has a hypothesis by now: z' = z + dz_t u0, gx' = gx + dg_t u1,
 *          gy' = gy + dg_t u2 from the pixel's CURRENT hypothesis; dz_t is dz halved t times (dz_t = dz_(t-1) * 0.5f), dg_t likewise;
 *          u_c = ((float)(int32)(x >> 8) - 8388608.0f) * (1.0f / 8388608.0f) with
 *          x = mix(mix(mix(seed + (2 t + h)) ^ (row W + col)) ^ (4 j + c)) in u32 arithmetic and
 *          mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *      A candidate whose centre is not live has no counted view, hence cell 0, and never wins.  For every active pixel of every half the
 *      call counts the class of what the pixel holds at the end of its list: kept / near / far / random.  Consequence: run(a) then run(b)
 *      with the same dz, dg, nrandom and seed equals run(a + b).
 *   7. Outputs: mvs_propagate_fetch downloads z, gx, gy and the cells (each pointer may be NULL; synchronises).
 *      mvs_propagate_depth_device is the z map, a depth map in the library's convention: it feeds mvs_depth_upload_device,
 *      mvs_depth_filter, the band sweeps as a prior, mvs_pyramid_prior and mvs_tsdf_shade.  mvs_propagate_cost_device is the cells as
 *      mean costs, (float)sum / (float)(255 k), +inf for cell 0, refreshed by init and run.  Both are NULL before the first init and do
 *      not change afterwards.  mvs_propagate_report: out[0..3] = kept, near, far, random since init, out[4] = the pixels that hold a
 *      cell != 0 now; it synchronises.
 * It propagates the preference of a window across a depth step for the nearer surface as well: beside occluders it does not help and
 * random steps of a coarse plane step make it worse (DESIGN.md section 25 has the figures).
 *   The stage touches no sweep, band, selection or filter state; it reads the staged frames however they got there (host setters,
 * _device forms, frame-store slots).  Its maps -- five H * W maps, H * W bytes for a guide (mvs_propagate_set_gate), H * W support bytes and a table of 1184 bytes
 * (mvs_propagate_set_consistency) and the counters -- are allocated by the first mvs_propagate_init; a
 * context that never calls it allocates nothing.  Asynchronous on the context's stream (one launch per half, no host synchronisation),
 * timed under MVS_K_SWEEP.
 * Errors: MVS_EINVAL for a NULL ctx, depth_dev or out, an unknown cost, a radius outside the cost's range, keep outside 0..8, a view
 * range outside 0..V, unknown flag bits, a negative or NaN max_step, iterations < 1, nrandom outside 0..4, a negative or non-finite dz or
 * dg; MVS_ESTATE without main view or views, for the exact sampler, for run, fetch and report before init, and for run when fewer views
 * are staged than init's range needs; MVS_ENOMEM.  All checks come before the first allocation; after an error nothing is written and the
 * context stays usable. */
#define MVS_PROPAGATE_SLOPES 1u
int mvs_propagate_init(mvs_ctx *ctx, const void *depth_dev, int view_first, int view_count, int cost, int radius, int keep, float max_step, unsigned flags);
int mvs_propagate_run(mvs_ctx *ctx, int iterations, float dz, float dg, int nrandom, unsigned seed);
/* Guide gate of the propagation's windows.  Rule 1 above gains one clause: member q of p's window is live iff it is
 * live as stated there AND |G(q) - G(p)| <= tau; everything else stands (candidates, the strict rule 4, the counters, run(a) then run(b)
 * = run(a + b)).  The call only records (tau, guide_dev) on the context; the default is (255, NULL), with which every call is bit-identical
 * to an ungated one.  The NEXT mvs_propagate_init takes the recorded gate, and the mvs_propagate_run calls that follow use what that init
 * took: a set_gate between init and run changes nothing until the next init.  With guide_dev NULL, G is the staged main image; otherwise
 * init copies H * W bytes from guide_dev (u8, on the context's GPU) on the context's stream into the stage's own allocation, so the
 * caller's buffer must be valid from this call to the end of that init and not longer.
 * WARNING, as for mvs_sweep_run_bestk_gated: a tau below the texture's own contrast starves ZNCC of variance.
 * Errors: MVS_EINVAL for a NULL ctx or tau outside 0..255 (nothing is recorded then). */
int mvs_propagate_set_gate(mvs_ctx *ctx, int tau, const void *guide_dev);
/* Geometric consistency against stored neighbour depth maps (tests/consistency_mirror.py is the arbiter, bit for
 * bit).  An opt-in term on the propagation's cells: a hypothesis also pays for disagreeing with what `nslots` (0..8) slots of the depth
 * store hold, and every pixel knows how many of them confirm what it holds.  The call only records its arguments (the slots are copied;
 * a slot listed twice counts twice); the default is off (nslots 0, slots may be NULL then), with which every call writes the bytes it
 * wrote before.  The NEXT mvs_propagate_init takes the recorded term, and the mvs_propagate_run calls that follow use what that init
 * took.  Everything is f32 with one rounding per operation, as in mvs_fuse_depth.  For the candidate depth cz at pixel p = (row, col):
 *   1. M is the staged main camera at init, M^-1 made as the depth store makes a slot's inverse; P_j, P_j^-1 are what
 *      mvs_depth_slot_matrices returns for neighbour j's slot, copied at init.
 *   2. X = dehomogenised M^-1 (xn(p), yn(p), cz, 1), fusion rule 2.
 *   3. q = P_j (X, 1); a = q_x / q_w, b = q_y / q_w; u = (a + 1)(W 0.5) - 0.5, v = (1 - b)(H 0.5) - 0.5; the pixel (floorf(v + 0.5),
 *      floorf(u + 0.5)) is tested against the frame as floats; z_j is the slot's depth there, valid when -1 < z_j < 1.
 *   4. X_j = the un-projection of (a, b, z_j) through P_j^-1 -- the CONTINUOUS position with the nearest pixel's depth, not the pixel
 *      centre as in fusion rule 3; s = M (X_j, 1), u_r, v_r as in 3; e = sqrtf(du du + dv dv) with du = u_r - col, dv = v_r - row.
 *   5. Neighbour j ANSWERS iff q_w > 0, the pixel is in the frame, z_j is valid, s_w > 0 and e <= max_px; e_j = e then, else max_px.
 *   6. g_j = (uint32)floorf(e_j (weight 255.0f)); g = (sum_j g_j) / nslots in integer division.
 *   7. A cell c = k << 24 | sum of section 25's rules with k > 0 becomes k << 24 | (sum + k g): its mean cost is the photometric mean
 *      plus g / 255 grey levels of the cost map's scale (ZNCC: 127.5 (1 - ncc)), and rule 4 there compares these cells.
 *   8. support(p) = the number of listed neighbours that answer for the hypothesis p HOLDS; 0 for a pixel without one (z not inside
 *      (-1, 1)) and everywhere when the term is off.  mvs_propagate_support_device is that map (H * W u8, in the stage's allocation; NULL
 *      before the first init), current after every init and run; mvs_propagate_support_fetch downloads it and synchronises.
 * The cost map, the report, the candidate list and run(a) then run(b) = run(a + b) stand.  The neighbours' maps are read in the depth
 * store when the kernel runs, not copied: overwriting a listed slot between init and run is the caller's business (the matrices stay
 * those of init).  weight 0 leaves z, slopes, cells, cost map and report as without the term and still fills the support map.
 * WARNING: consistently wrong neighbours confirm each other -- with neighbour maps estimated by the same recipe the gain is small and
 * can be negative (DESIGN.md section 27 has the figures); the weight is on the cost map's scale.
 * Errors: at the setter MVS_EINVAL for a NULL ctx, nslots outside 0..8, NULL slots with nslots > 0, a negative slot, a negative or
 * non-finite weight, a max_px not finite or <= 0, floorf(max_px weight 255) > 1 000 000 (nothing is recorded then).  At init with a term
 * recorded: MVS_ESTATE without a depth store, for a slot outside it or an unfilled one; MVS_EINVAL for a singular main camera, and for
 * MVS_KEEP_ALL with so many views that views (65025 + floorf(max_px weight 255)) reaches 2^24 (the cells' sums have 24 bits; keep <= 8
 * always fits).  At run: MVS_ESTATE when the depth store was re-sized since init or a listed slot is no longer filled.  All checks come
 * before the first allocation; after an error nothing is written. */
int mvs_propagate_set_consistency(mvs_ctx *ctx, int nslots, const int *slots, float weight, float max_px);
void *mvs_propagate_support_device(mvs_ctx *ctx);
int mvs_propagate_support_fetch(mvs_ctx *ctx, uint8_t *support_hw);
int mvs_propagate_fetch(mvs_ctx *ctx, float *z_hw, float *gx_hw, float *gy_hw, unsigned int *cells_hw);
void *mvs_propagate_depth_device(mvs_ctx *ctx);
void *mvs_propagate_cost_device(mvs_ctx *ctx);
int mvs_propagate_report(mvs_ctx *ctx, long long out[5]);
/* The same selection in two steps, for a view-sharded job that REDUCE-SCATTERS the packed volume instead of all-reducing it
 * (half the bytes over xGMI): rank r owns the summed cells of planes [plane_first, plane_first + plane_count) in
 * `volume_slice_dev` ([plane_count][H][W] u32) and selects a partial best per pixel over them -- `partial_out_dev` receives
 * H*W records of 8 bytes (packed best cell, best absolute plane index; 0xffffffff = none).  The ranks all-gather their
 * records into [nparts][H*W] in ascending plane order and every rank merges them with mvs_sweep_combine_partials, a later part
 * winning only if strictly better (ties -> lowest plane, like mvs_sweep_argmin).  Both are asynchronous on the context's stream. */
int mvs_sweep_argmin_partial(mvs_ctx *ctx, const void *volume_slice_dev, int plane_first, int plane_count, void *partial_out_dev);
int mvs_sweep_combine_partials(mvs_ctx *ctx, const void *partials_dev, int nparts);
/* device pointer + size of the packed volume: nplanes*H*W uint32 cells (count << 24 | sum with the fixed sampler,
 * count << 16 | sum with the exact one); sums and counts add exactly, so an integer sum-all-reduce across view
 * shards is bit-identical to the single-GPU result */
void *mvs_sweep_volume_device(mvs_ctx *ctx, size_t *bytes);
/* make the sweep write into caller-owned device memory (e.g. a torch tensor handed to RCCL) */
int mvs_sweep_use_volume(mvs_ctx *ctx, void *device_ptr, size_t bytes);
/* device pointers of the per-pixel results (H*W each): depth f32, best cost f32, best index i32 */
void *mvs_sweep_depth_device(mvs_ctx *ctx);
void *mvs_sweep_cost_device(mvs_ctx *ctx);
void *mvs_sweep_index_device(mvs_ctx *ctx);
/* copy results to host (synchronises); any pointer may be NULL */
int mvs_sweep_fetch(mvs_ctx *ctx, float *depth_hw, float *cost_hw, int32_t *index_hw, uint32_t *packed_volume_dhw);
/* read back the f32 view matrices the sweep uses (nviews*12), for parity checks */
int mvs_sweep_view_matrices(mvs_ctx *ctx, float *q_out);

/* ---- a sequence on one GPU: frames uploaded once, several main frames per launch (recon.cpp:65-117) -------------------------
 * The reference sweeps every chosen main frame against a handful of neighbouring frames; through mvs_sweep each frame of the
 * sequence crosses PCIe once per main frame that uses it, and a 640 x 480 frame leaves most of the chip idle.  The frame store keeps
 * every frame of the sequence resident (raw and as quad image: 5 bytes per pixel); mvs_sweep_batch then sweeps nmain
 * main frames, each against its own nside side views -- all of them slots of the store -- in ONE launch of the general tiled kernel
 * (fixed sampler) and returns the nmain depth maps (and best costs) tightly packed.  Results are bit-identical to mvs_sweep on the
 * same frames and cameras.
 *   mvs_frame_store(ctx, capacity)   sizes the store (1..8191 frames); re-sizing empties it
 *   mvs_frame_upload(ctx, slot, f)   copies frame f (H*W u8) into a slot and prepares it (asynchronous; `f` must stay valid until the
 *                                    next synchronising call on the context, e.g. mvs_sweep_batch or mvs_synchronize)
 *   mvs_sweep_batch(...)             main_slots[nmain], main_cams[nmain*16], side_slots[nmain*nside], side_cams[nmain*nside*16];
 *                                    depth_out[nmain*H*W], cost_out nullable; synchronises */
int mvs_frame_store(mvs_ctx *ctx, int capacity);
int mvs_frame_upload(mvs_ctx *ctx, int slot, const uint8_t *frame_hw);
int mvs_frame_upload_device(mvs_ctx *ctx, int slot, const void *frame_dev); /* the frame is already on the context's GPU (stream-ordered) */
/* ONE main view over the frame store -- the resident-handle form of mvs_sweep for a caller that keeps its sequence on the device
 * (the loop of recon.cpp:65-117 through RenderHIP): main and side views are slots, nothing is uploaded, copied or
 * re-prepared (the quad images were built by mvs_frame_upload); the call pays the view matrices, the region plan, the sweep with depth
 * selection and the download of depth_hw (and cost_hw, nullable).  Bit-identical to mvs_sweep on the same frames and cameras; fixed
 * sampler; synchronises.  Afterwards the context's staged state (mvs_sweep_run, mvs_sweep_depth_device ...) refers to these views
 * until the next setter; re-uploading one of the slots in between changes the frame under it. */
int mvs_sweep_handles(mvs_ctx *ctx, int main_slot, const float main_cam[16], int nside, const int *side_slots, const float *side_cams /* nside*16 */,
                      int nplanes, float z_lo, float z_hi, float *depth_hw, float *cost_hw);
int mvs_sweep_batch(mvs_ctx *ctx, int nmain, const int *main_slots, const float *main_cams, int nside, const int *side_slots,
                    const float *side_cams, int nplanes, float z_lo, float z_hi, float *depth_out, float *cost_out);
/* The same without waiting: the batch is queued and the call returns; depth_out / cost_out (which must stay valid, and should be
 * page-locked: mvs_host_alloc) are complete when mvs_sweep_batch_wait returns.  Two batches can be in flight -- the results of one
 * cross PCIe on a second stream while the next is planned and swept, and the host prepares that next one meanwhile; a third call waits
 * for the oldest.  Frames a queued batch uses must not be re-uploaded before it has been waited for.  (mvs_sweep_batch = this + wait.) */
int mvs_sweep_batch_async(mvs_ctx *ctx, int nmain, const int *main_slots, const float *main_cams, int nside, const int *side_slots,
                          const float *side_cams, int nplanes, float z_lo, float z_hi, float *depth_out, float *cost_out);
int mvs_sweep_batch_wait(mvs_ctx *ctx);

/* ---- lens: distorted frames -> the pinhole frames the cameras describe (csrc/lens.hip) ------------------------
 * The cameras of a tracks file are a tracker's solution for UNDISTORTED image coordinates; the frames that go with them are as the lens
 * saw them.  A context can carry the clip's radial lens model -- the reference's cameraToScreen (configuration.cpp:248-259) with the
 * pixel mapping of configuration.cpp:292-293 -- and resample frames through it on the device: for every pixel centre of the output
 * (pinhole) frame the model gives the position in the distorted frame, which is sampled with mvs_flow_remap's fixed-point bicubic rule
 * (1/32-pixel positions, Q15 weights) and a REPLICATED border (a tap outside the frame takes the nearest frame pixel; every output
 * pixel is written).  The arithmetic is f32 with one rounding per operation, stated in DESIGN.md section 17 and restated by
 * tests/lens_mirror.py; the device is bit-identical to it.  With zero coefficients and the centre at (W/2, H/2) the output is the input.
 * Opt-in: a context without a lens behaves exactly as before, and nothing is allocated for one.
 *   mvs_set_lens(ctx, k, cx, cy)     k = the three radial coefficients (distortion: [k1, k2, k3] of the tracks file; the reference uses
 *                                    two), (cx, cy) = the clip's center-x / center-y in pixels of the context's frame, cy measured from
 *                                    the BOTTOM as the tracks files do.  k == NULL clears the lens.  Touches nothing already uploaded.
 *                                    MVS_EINVAL for a non-finite coefficient or centre, |k_i| > MVS_LENS_MAX_COEFFICIENT, or a lens whose
 *                                    radial map rho -> rho k(rho^2) folds over inside the frame: d/d rho = 1 + 3 k1 rho^2 + 5 k2 rho^4 +
 *                                    7 k3 rho^6 <= 0, in double, at one of the 1024 radii rho_max i / 1024, i = 1..1024, rho_max^2 =
 *                                    (1 + (H/W)^2) / 4 (the farthest corner in the model's units).
 *   mvs_lens(ctx, k, &cx, &cy)       1 and the lens (each pointer nullable) when one is set, 0 when none
 *   mvs_undistort(ctx, src, dst)     one frame, host buffers (H*W u8 each); synchronises
 *   mvs_undistort_device(ctx, src, dst, n)   n (1..65535) tightly packed H*W frames on the context's GPU in one launch; asynchronous and
 *                                    stream-ordered like mvs_frame_upload_device; MVS_EINVAL when the two ranges overlap (src == dst too)
 *   mvs_undistort_map(ctx, map)      diagnostic: the source position (x, y), in pixel indices of the distorted frame, of every output
 *                                    pixel (H*W*2 f32), computed by the device; synchronises
 *   mvs_frame_upload_lens(ctx, slot, f) / mvs_frame_upload_lens_device: mvs_frame_upload / _device with the frame taken through the lens
 *                                    on its way into the store: the slot's bytes (raw frame and quad image) are those of mvs_undistort
 *                                    followed by mvs_frame_upload, so everything that reads slots (mvs_sweep_handles, mvs_sweep_batch*,
 *                                    mvs_process_frame_slots, mvs_tsdf_integrate_frames) sees pinhole frames.  A host frame is staged in
 *                                    a W*H device buffer allocated by the first such call.
 * Errors: MVS_EINVAL for a NULL ctx or pointer and for a slot outside the store (an unsized store has no slots); MVS_ESTATE from all but
 * mvs_set_lens and mvs_lens when no lens is set; MVS_ENOMEM.  After an error nothing is written.  The launches are timed under
 * MVS_K_PROJECT. */
#define MVS_LENS_MAX_COEFFICIENT 16
int mvs_set_lens(mvs_ctx *ctx, const float k[3], float center_x, float center_y);
int mvs_lens(mvs_ctx *ctx, float k_out[3], float *center_x, float *center_y);
int mvs_undistort(mvs_ctx *ctx, const uint8_t *src_hw, uint8_t *dst_hw);
int mvs_undistort_device(mvs_ctx *ctx, const void *src_dev, void *dst_dev, int nframes);
int mvs_undistort_map(mvs_ctx *ctx, float *map_hw2);
int mvs_frame_upload_lens(mvs_ctx *ctx, int slot, const uint8_t *frame_hw);
int mvs_frame_upload_lens_device(mvs_ctx *ctx, int slot, const void *frame_dev);

/* ---- depth store + fusion: depth maps of a sequence -> one multi-view-consistent oriented point cloud (csrc/fuse.hip) ----
 * The store keeps depth maps in the library's convention (main-camera NDC z, 1.0 = empty: a sweep's result, or mvs_depth of a mesh) with
 * their best costs and cameras in HBM.  Life cycle as the frame store's: mvs_depth_store sizes it (1..8191 slots, re-sizing empties it);
 * uploads are stream-ordered (host buffers must stay valid until the next synchronising call, e.g. mvs_fuse_depth).  cost may be NULL;
 * mvs_depth_upload_device(ctx, slot, cam, mvs_sweep_depth_device(ctx), mvs_sweep_cost_device(ctx)) stores a sweep's result device to device.
 * mvs_fuse_depth: for every pixel (row, col) of ref_slot with depth z, all in f32, one rounding per operation, no contraction:
 *   1 valid: -1 < z < 1 (and cost <= max_cost when max_cost is finite)
 *   2 X = h.xyz / h.w with h = P_r^-1 (xn, yn, z, 1), xn / yn the sweep's pixel centres; w_r = (P_r (X, 1)).w must be > 0
 *   3 neighbour j (listed order): q = P_j (X, 1), q.w > 0; u = (q.x/q.w + 1) W/2 - 1/2, v = (1 - q.y/q.w) H/2 - 1/2; pixel
 *     (floor(v + 1/2), floor(u + 1/2)) in the frame and valid in j; X_j = its back-projection through P_j^-1; s = P_r (X_j, 1), s.w > 0;
 *     j agrees when the reprojection (u_r, v_r) of X_j lies within max_reproj_px of (col, row) and |s.w - w_r| / w_r <= max_rel_depth
 *   4 kept when at least min_consistent neighbours agree; point = (X + agreeing X_j, summed in listed order) / count, w = 1
 *   5 normal from the reference map alone: tangents along columns and rows from the valid 4-neighbours whose linear depth is within
 *     max_rel_depth of w_r (central difference, else one-sided, else none: the pixel is dropped); n = normalize(t_col x t_row), flipped
 *     to face the camera centre (outward, as mvs_poisson_surface needs)
 * Rows (x, y, z, 1, nx, ny, nz) in ascending pixel index, the same from run to run.  mvs_fuse_depth synchronises and returns the row count;
 * out_points7 (nullable, room for H*W rows) receives the rows; they stay in HBM for mvs_fuse_points_device until the next mvs_fuse_depth.
 * Errors: MVS_EINVAL for a NULL ctx, a slot outside the store, nneighbours outside 0..16, a neighbour equal to ref_slot, min_consistent
 * outside 0..nneighbours, a negative (or NaN) threshold, a singular camera; MVS_ESTATE for an unfilled slot, or a finite max_cost when a
 * slot involved was stored without cost.  max_cost = INFINITY: costs are not read. */
int mvs_depth_store(mvs_ctx *ctx, int capacity);
int mvs_depth_upload(mvs_ctx *ctx, int slot, const float cam[16], const float *depth_hw, const float *cost_hw /* nullable */);
int mvs_depth_upload_device(mvs_ctx *ctx, int slot, const float cam[16], const void *depth_dev, const void *cost_dev /* nullable */);
int mvs_fuse_depth(mvs_ctx *ctx, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px,
                   float max_rel_depth, float max_cost, float *out_points7 /* nullable: H*W*7 */, int *out_count);
void *mvs_fuse_points_device(mvs_ctx *ctx); /* rows of the last mvs_fuse_depth, in HBM; NULL before the first */
/* diagnostic: the slot's matrices as the kernels use them: out[0..15] = P, out[16..31] = P^-1 (inverted in double, rounded once),
 * out[32..35] = camera centre (x, y, z, 1): the null vector of P's rows x, y, w, dehomogenised in double, rounded once */
int mvs_depth_slot_matrices(const mvs_ctx *ctx, int slot, float out[36]);

/* ---- TSDF fusion: every stored depth map votes into one truncated signed distance volume, meshed at its zero level set ----------
 * (csrc/tsdf.hip; Curless & Levoy 1996.)  The context owns one cubic volume of G^3 nodes, G = 16..512: node (i, j, k)
 * at (ox + h i, oy + h j, oz + h k), an f32 sum and an i32 count per node in the order (k G + j) G + i, 8 bytes per node.  mvs_tsdf_volume
 * sizes and zeroes it (again: clears it); the depth store does not touch it.  mvs_tsdf_integrate adds the listed slots' maps in list order,
 * asynchronous and stream-ordered like mvs_sweep_run; a slot listed twice counts twice, and a list split over several calls gives the same
 * bytes as one call.  All f32, one rounding per operation, no contraction; inv_tau = 1 / truncation rounded once on the host:
 *   1 per listed slot, a w-map: pixel valid by fusion rule 1 (with max_cost) and w = (P (X, 1)).w > 0 with X from rule 2: w, else NaN
 *   2 per node (x = ox + h i, ... each a product then a sum) and slot: q_r = P[r][0] x + ((P[r][1] y + P[r][2] z) + P[r][3]), r = 0, 1, 3;
 *     no update unless q_w > 0
 *   3 inv = 1 / q_w, u = (q_x inv + 1) (W 0.5) - 0.5, v = (1 - q_y inv) (H 0.5) - 0.5; pixel (floor(v + 0.5), floor(u + 0.5)), tested
 *     against the frame as floats; no update outside it or where the w-map holds NaN
 *   4 t = (wd - q_w) inv_tau (positive in front of the surface, on the camera's side); when t >= -1: sum += min(t, 1), count += 1
 *   5 mvs_tsdf_surface: F = sum / (float)count where count >= min_observations, else 1; a cell is meshed when all 8 corners have
 *     count >= min_observations; surface nets at iso 0 as mvs_poisson_surface meshes chi, faces along +grad F (toward the cameras).
 *     The surface has grid = {G, origin, h}, iso 0, spacing h (mvs_surface_spacing), ratio_kept 1, support 0, no chi or splat; the
 *     mvs_surface_* calls all work on it.  An empty volume gives 0 vertices and 0 faces.
 * mvs_tsdf_fetch synchronises and downloads the fields (diagnostic).  Errors: MVS_EINVAL for a NULL ctx, out or slots, G outside 16..512,
 * a non-finite origin, a spacing or truncation not finite and > 0, nslots < 1, a slot outside the store, a negative or NaN max_cost,
 * min_observations < 1; MVS_ESTATE before mvs_tsdf_volume, for an unfilled slot, or a finite max_cost when a slot was stored without cost.
 * max_cost = INFINITY: costs are not read.  MVS_K_TSDF times mvs_tsdf_integrate's launches. */
struct mvs_surface;
int mvs_tsdf_volume(mvs_ctx *ctx, int nodes_per_axis /* 16..512 */, const float origin3[3], float node_spacing, float truncation);
int mvs_tsdf_integrate(mvs_ctx *ctx, int nslots, const int *slots, float max_cost /* INFINITY: costs not read */);
int mvs_tsdf_fetch(mvs_ctx *ctx, float *sdf_sum /* G^3, nullable */, int32_t *count /* G^3, nullable */);
int mvs_tsdf_surface(mvs_ctx *ctx, int min_observations /* >= 1 */, struct mvs_surface **out);

/* ---- ray-cast of the TSDF volume: the fused model as depth and normal maps of any camera (csrc/raycast.hip) ----
 * mvs_tsdf_raycast marches one ray per pixel of the context's W x H frame through the volume's field F (rule 5 above, with this call's
 * min_observations) and writes the first front-face crossing of its zero level set: NDC z of `cam` in the library's depth convention
 * (1.0 = empty) and the unit normal +grad F (toward free space, like the mesh's faces; (0, 0, 0) = empty).  Every pixel is written on every
 * call; the maps hold the last raycast (mvs_tsdf_volume and mvs_depth_store do not touch them) and stay in HBM:
 * mvs_depth_upload_device(ctx, slot, cam, mvs_tsdf_raycast_depth_device(ctx), NULL) stores the model's depth map device to device.
 * `cam` is any projective camera with a finite centre (it need not be a stored one); P, P^-1 and the centre C are those of a depth slot
 * (mvs_depth_slot_matrices).  All f32, one rounding per operation, no contraction; inv_h = 1 / h and delta = step_nodes h rounded once
 * on the host, K_max = floor(1.75 (G - 1) / step_nodes) + 2:
 *   1 ray: X1 = P^-1 (xn, yn, 0, 1) dehomogenised (xn / yn the sweep's pixel centres), (P (X1, 1)).w > 0; d = X1 - C,
 *     len = sqrt((dx^2 + dy^2) + dz^2) finite and > 0, d = d / len
 *   2 box: per axis lo = o_a, hi = o_a + h (float)(G - 1); d_a != 0: the slab between (lo - C_a) / d_a and (hi - C_a) / d_a; d_a = 0: unbounded
 *     when lo <= C_a <= hi, else empty; t_in = max(0, near ends), t_out = min(far ends); empty unless t_in <= t_out
 *   3 samples k = 0 .. K_max while t_k = t_in + delta (float)k <= t_out: X = C + t_k d, g = (X - o) inv_h, cell i_a = clamp(floor(g_a), 0, G - 2)
 *     (NaN: 0), fraction f_a = clamp(g_a - (float)i_a, 0, 1) (NaN: 0); valid when the cell's mask is set; value: the trilinear interpolant of
 *     the cell's 8 corners of F, each lerp a + f (b - a), along i, then j, then k
 *   4 hit: the first k >= 1 with sample k - 1 valid and > 0 and sample k valid and <= 0; t* = t_(k-1) + delta (F_(k-1) / (F_(k-1) - F_k)).
 *     Back faces (<= 0 to > 0) are ignored; a ray that starts behind a surface leaves it without a hit
 *   5 at X* = C + t* d: cell and fractions as in 3, empty if its mask is clear; gradient of the interpolant (per axis the 4 corner differences
 *     along it, lerped along the other two in the order i, j, k), n = g / sqrt((gx^2 + gy^2) + gz^2) (length finite and > 0);
 *     z = (P (X*, 1)).z / (P (X*, 1)).w, empty unless -1 < z < 1 (a hit nearer than the near plane has no value in the depth convention)
 * A surface is missed where step_nodes h exceeds the band observed behind it (the truncation): keep step_nodes <= truncation / (2 h).
 * mvs_tsdf_raycast is asynchronous and stream-ordered like mvs_tsdf_integrate and timed under MVS_K_TSDF; mvs_tsdf_raycast_fetch
 * synchronises.  mvs_tsdf_upload is the counterpart of mvs_tsdf_fetch (checkpoint and resume; crafted fields): it replaces both fields
 * and synchronises; values are taken as given (a count below min_observations is "unobserved" wherever that is tested).
 * Errors: MVS_EINVAL for a NULL ctx, cam or (upload) array, a camera with a non-finite entry, singular or without a finite centre,
 * min_observations < 1, step_nodes not finite or outside [1/16, 4]; MVS_ESTATE before mvs_tsdf_volume, and for mvs_tsdf_raycast_fetch
 * before the first raycast; MVS_ENOMEM. */
int mvs_tsdf_upload(mvs_ctx *ctx, const float *sdf_sum /* G^3 */, const int32_t *count /* G^3 */);
int mvs_tsdf_raycast(mvs_ctx *ctx, const float cam[16], int min_observations /* >= 1 */, float step_nodes /* 1/16 .. 4 */);
void *mvs_tsdf_raycast_depth_device(mvs_ctx *ctx);   /* H*W f32, NDC z of cam, 1.0 = empty; NULL before the first raycast */
void *mvs_tsdf_raycast_normals_device(mvs_ctx *ctx); /* H*W*3 f32, unit, (0,0,0) = empty; NULL before the first raycast */
int mvs_tsdf_raycast_fetch(mvs_ctx *ctx, float *depth_hw /* nullable */, float *normals_hw3 /* nullable */);

/* ---- appearance of the TSDF volume: the frames' grey levels fused beside the distances (csrc/tsdf.hip, csrc/appearance.hip, DESIGN.md
 * section 15) ----  The volume can carry what the surface looks like: the frames of the frame store (mvs_frame_upload; one u8 per pixel)
 * vote their intensities into it while their depth maps are integrated, and the result is read back at the surface points of any depth
 * map (mvs_tsdf_shade: the image that goes with mvs_tsdf_raycast's depth and normals, comparable with a frame by mvs_compare) or at a
 * caller's points (mvs_tsdf_sample_appearance: vertex grey levels of mvs_tsdf_surface's mesh).  Integer votes, f32 reads with one rounding
 * per operation and no contraction:
 *   A cell: one uint32 per node in the volume's node order, count << 24 | sum: count 0..255 votes, sum of their u8 intensities
 *     (<= 255 * 255); 4 bytes per node.  The appearance volume is allocated and zeroed by the first mvs_tsdf_integrate_frames or
 *     mvs_tsdf_appearance_upload after mvs_tsdf_volume; mvs_tsdf_volume drops it ("no appearance"); mvs_tsdf_integrate and mvs_tsdf_upload
 *     do not touch it.  A caller who never asks for appearance allocates nothing.
 *   B mvs_tsdf_integrate_frames takes the pairs (depth_slots[e], frame_slots[e]) in list order: rules 1-4 of mvs_tsdf_integrate on
 *     (sum, count), the same bytes as mvs_tsdf_integrate(ctx, n, depth_slots, max_cost) gives; and where rule 4 updates with t < 1 (so
 *     -1 <= t < 1: the unclamped band around the observed surface) and the cell's count is < 255: sum += I[r][c], count += 1, with I the
 *     raw frame in frame-store slot frame_slots[e] and (r, c) the pixel of rule 3.  A cell at count 255 ignores later votes (list order
 *     is fixed: deterministic); a pair listed twice votes twice; a list split over calls gives the same bytes.
 *   C appearance at a point X: g_a = (X_a - o_a) inv_h (inv_h = 1 / h rounded once); every 0 <= g_a <= (float)(G - 1) (NaN fails), else
 *     none: no clamping into the box.  Cell and fractions as in the raycast's rule 3; corner d = dk 4 + dj 2 + di has weight
 *     w_d = (wx wy) wz, wx = di ? fx : 1 - fx (wy, wz alike), and is present when its count > 0 with a_d = (float)sum_d / (float)count_d;
 *     over the present corners in ascending d: num = num + w_d a_d, den = den + w_d, both from 0; none unless den > 0, else num / den.
 *     Independent of F, of the cell mask and of min_observations.
 *   D mvs_tsdf_shade(ctx, cam, depth_dev): depth_dev is H*W f32 on the context's GPU in the library's depth convention for cam
 *     (mvs_tsdf_raycast_depth_device, mvs_sweep_depth_device, mvs_depth_slot_device, ...); P and P^-1 are a depth slot's for cam.  Per
 *     pixel: -1 < z < 1 (fusion rule 1), X = P^-1 (xn, yn, z, 1) dehomogenised with the sweep's pixel centres (fusion rule 2),
 *     (P (X, 1)).w > 0, then C.  Output H*W pairs of u8 like mvs_warp_by_depth's: (min(floor(value + 0.5), 255), 255), or (0, 0) where
 *     any of that fails; every pixel is written.  Asynchronous and stream-ordered; the map stays in HBM (mvs_tsdf_shade_device: NULL
 *     before the first shade); mvs_tsdf_shade_fetch synchronises.
 *   E mvs_tsdf_sample_appearance(ctx, points4, n, out): host rows (x, y, z, w) as mvs_surface_fetch returns them; X = (x / w, y / w, z / w),
 *     then C; out[i] is the value, NaN for none.  Synchronises.
 *   F mvs_tsdf_appearance_fetch / _upload: the G^3 cells, the counterparts of mvs_tsdf_fetch / mvs_tsdf_upload (checkpoint; crafted
 *     fields); upload takes values as given (a sum above 255 * count is the caller's affair) and both synchronise.
 * Errors: MVS_EINVAL for a NULL ctx or array, n < 1, a depth slot outside the depth store, a frame slot outside the frame store, a negative
 * or NaN max_cost, a camera mvs_tsdf_raycast would refuse, a NULL depth_dev; MVS_ESTATE before mvs_tsdf_volume, for an unfilled depth or
 * frame slot, a finite max_cost with a slot stored without cost, for _appearance_fetch, _shade and _sample_appearance while there is no
 * appearance volume, and for mvs_tsdf_shade_fetch before the first shade; MVS_ENOMEM.  All launches are timed under MVS_K_TSDF.
 * mvs_depth_slot_device: the device address of a filled depth slot's H*W f32 map (NULL for an unfilled slot or one outside the store). */
int mvs_tsdf_integrate_frames(mvs_ctx *ctx, int n, const int *depth_slots, const int *frame_slots, float max_cost /* INFINITY: costs not read */);
int mvs_tsdf_appearance_fetch(mvs_ctx *ctx, uint32_t *cells /* G^3 */);
int mvs_tsdf_appearance_upload(mvs_ctx *ctx, const uint32_t *cells /* G^3 */);
int mvs_tsdf_shade(mvs_ctx *ctx, const float cam[16], const void *depth_dev /* H*W f32 on the context's GPU */);
void *mvs_tsdf_shade_device(mvs_ctx *ctx); /* H*W pairs of u8 (grey, 255) or (0, 0); NULL before the first shade */
int mvs_tsdf_shade_fetch(mvs_ctx *ctx, uint8_t *shaded_hw2);
int mvs_tsdf_sample_appearance(mvs_ctx *ctx, const float *points4 /* n x 4 */, int n, float *out /* n */);
void *mvs_depth_slot_device(mvs_ctx *ctx, int slot);

/* ---- support planes, masked fusion and sequence fusion (csrc/fuse.hip, csrc/fuse_sequence.hip, csrc/tsdf.hip) ----
 * A support plane is H * W bytes of u8 per depth slot: how many neighbour maps confirm the depth each pixel of the stored map holds, e.g.
 * the propagation's support map (mvs_propagate_support_device).  All planes live in one buffer of `capacity` planes, allocated by the first
 * support upload after mvs_depth_store and freed by mvs_depth_store (re-sizing empties the store).  Uploads are stream-ordered like
 * mvs_depth_upload*; mvs_depth_support_fetch synchronises.  mvs_depth_upload / mvs_depth_upload_device into a slot drop that slot's plane
 * (a flag, not a copy: a new map is not described by the old bytes).  MVS_EINVAL: NULL argument, slot outside the store; MVS_ESTATE: upload
 * into a slot without a depth map, fetch from a slot without a plane; MVS_ENOMEM.  A refused call leaves the context usable.
 *
 * Rule 1s replaces fusion rule 1 wherever a min_support (0..255) is given: a stored pixel p is valid when rule 1 holds and, for
 * min_support > 0, support[p] >= min_support.  With min_support > 0 every slot involved must have a plane (else MVS_ESTATE); with
 * min_support = 0 planes are not read and need not exist.  Rule 1s is the same as overwriting the stored depth with the empty value 1.0
 * wherever the support is too low.
 *
 * mvs_fuse_depth_masked is mvs_fuse_depth with rule 1s in the three places it reads a stored depth: the reference pixel, its four tangent
 * neighbours, and the neighbour map's pixel of rule 3.  It fills the same buffers (mvs_fuse_points_device returns its rows).
 * mvs_tsdf_integrate_masked is mvs_tsdf_integrate (frame_slots NULL) or mvs_tsdf_integrate_frames with rule 1s in the w-map pass: a masked
 * pixel's w is NaN.  With min_support = 0 both write the bytes of the calls they extend.
 *
 * mvs_fuse_sequence fuses a list of references into one cloud in which every surface point appears once:
 *   S1 Every distinct slot named in the call has a claim plane of H * W bytes, all zero when the call starts.
 *   S2 References are taken in list order.  For reference i, rules 1s-5 of mvs_fuse_depth_masked run with its row of neighbours
 *      (neighbour_slots[i * nneighbours ...]); a -1 entry is skipped, a neighbour listed twice votes twice.  A pixel p is KEPT when those
 *      rules keep it and claim_ref[p] == 0.  Claims gate nothing else: a claimed pixel is still a tangent neighbour and still votes in
 *      other references' rule 3 -- it is surface, only not a new point.
 *   S3 For every kept pixel and every neighbour j that agreed in rule 3: claim_j[(r_j, c_j)] = 1, at the pixel rule 3 read.  Dropped
 *      pixels claim nothing.
 *   S4 Rows are (x, y, z, 1, nx, ny, nz); reference i's rows come in ascending pixel index, behind reference i - 1's.  A row whose index
 *      is >= max_rows is not written; *out_count is the total either way and out_ref_counts[i] reference i's count.  Claims are made
 *      whether or not the row fitted: calling again with a larger max_rows gives the same rows, because S1 clears the planes.
 *      max_rows = 0 with a NULL out_points7 is a counting call.
 *   S5 The result is determinate: the launches of reference i read only claim plane ref_i and write only planes of slots other than
 *      ref_i (a neighbour equal to its reference is refused, as in mvs_fuse_depth), every write stores the value 1, and the launches are
 *      stream-ordered.
 * The host does not wait between references: the running total lives in device memory and the call synchronises once (totals and
 * per-reference counts) plus once for the optional row download; row offsets are 64-bit.  out_points7 NULL with max_rows > 0 leaves the
 * rows on the device (mvs_fuse_sequence_points_device).  Errors beside mvs_fuse_depth's: nrefs outside 1..capacity, a reference listed
 * twice, nneighbours outside 0..16, min_support outside 0..255, negative max_rows; MVS_ENOMEM.
 * Out of scope: weights in the TSDF sum, a per-row view count, the propagation's geometric term reading the neighbours' planes, batching
 * references that share no slot into one launch. */
int mvs_depth_support_upload(mvs_ctx *ctx, int slot, const uint8_t *support_hw);
int mvs_depth_support_upload_device(mvs_ctx *ctx, int slot, const void *support_dev); /* e.g. mvs_propagate_support_device(ctx) */
int mvs_depth_support_fetch(mvs_ctx *ctx, int slot, uint8_t *support_hw);
int mvs_depth_support_drop(mvs_ctx *ctx, int slot);
int mvs_fuse_depth_masked(mvs_ctx *ctx, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px,
                          float max_rel_depth, float max_cost, int min_support, float *out_points7, int *out_count);
int mvs_tsdf_integrate_masked(mvs_ctx *ctx, int n, const int *depth_slots, const int *frame_slots /* nullable: no appearance */, float max_cost,
                              int min_support);
int mvs_fuse_sequence(mvs_ctx *ctx, int nrefs, const int *ref_slots, int nneighbours, const int *neighbour_slots /* nrefs x nneighbours, -1 = none */,
                      int min_consistent, float max_reproj_px, float max_rel_depth, float max_cost, int min_support, long long max_rows,
                      float *out_points7 /* nullable: max_rows x 7 */, int *out_ref_counts /* nullable: nrefs */, long long *out_count);
void *mvs_fuse_sequence_points_device(mvs_ctx *ctx); /* the rows of the last call, min(total, max_rows) of them; NULL before the first */

/* ---- normals: from the propagation's slopes, per depth slot, in the fusion (csrc/normals.hip) ----------------
 * A normal map is H * W * 3 f32, interleaved, unit; (0, 0, 0) means none -- the layout of mvs_tsdf_raycast_normals_device.  All
 * arithmetic is f32 with one rounding per operation, `/` and sqrt correctly rounded, no FMA but the pixel centres'.
 *
 * Rule N1 (mvs_propagate_normals).  cam is the main camera P (row-major, clip = P X) as given to mvs_depth_upload; its centre C is derived
 * as mvs_depth_slot_matrices derives it.  For pixel (row, col) holding the hypothesis (z, gx, gy) with -1 < z < 1:
 *   xn, yn   the sweep's pixel centres, fmaf(2 col + 1, 1/W, -1) and fmaf(-(2 row + 1), 1/H, 1)
 *   a = -gx (W 0.5),  b = gy (H 0.5),  d = -((z + a xn) + b yn)                 the NDC plane a x + b y + z + d = 0
 *   m_k = ((a P[0][k] + b P[1][k]) + P[2][k]) + d P[3][k],  k = 0..3            its world plane, the row vector times P
 *   n = m.xyz / sqrt((m0 m0 + m1 m1) + m2 m2)                                    zeros when the length is 0, infinite or NaN
 *   n is negated when ((m0 C0 + m1 C1) + m2 C2) + m3 < 0                         the normal points to the camera's side of the plane
 * A pixel without a hypothesis (z outside (-1, 1), NaN) gives zeros.  The call reads the stage's maps as they are at that point of the
 * stream (after any mvs_propagate_run), is asynchronous and touches no other state; the map is made by the first call, behind every check.
 * MVS_EINVAL: NULL argument, a camera with a non-finite entry, singular or without a finite centre; MVS_ESTATE: before mvs_propagate_init
 * (mvs_propagate_normals), before the first mvs_propagate_normals (the fetch; the pointer is NULL then).
 *
 * Normal planes.  One plane per depth slot in one buffer of `capacity` planes, made by the first normals upload after mvs_depth_store and
 * freed by mvs_depth_store.  Uploads are stream-ordered like mvs_depth_upload*; the fetch synchronises.  mvs_depth_upload* into a slot drops
 * that slot's plane (a flag), so a plane always describes the stored map.  The device form takes mvs_propagate_normals_device(ctx) or
 * mvs_tsdf_raycast_normals_device(ctx) unchanged.  Errors are the support planes': MVS_EINVAL for a NULL argument or a slot outside the
 * store, MVS_ESTATE for an upload into a slot without a depth map or a fetch from a slot without a plane, MVS_ENOMEM.
 * A stored normal is USABLE when 0.5 < (nx nx + ny ny) + nz nz < 2: false for zeros, NaN and infinities.
 *
 * mvs_fuse_depth_normals is mvs_fuse_depth_masked (rules 1s-5) with two changes; n_r is the reference slot's stored normal at the pixel,
 * n_j voter j's stored normal at the pixel (r, c) rule 3 read it at.
 *   3n  A voter that passes every test of rule 3 must also satisfy (n_r.x n_j.x + n_r.y n_j.y) + n_r.z n_j.z >= min_normal_cos whenever
 *       both normals are usable; the test passes when either is missing (no plane on that slot, or an unusable value).
 *       min_normal_cos <= 1; -INFINITY turns the test off; NaN or a value above 1 is MVS_EINVAL.
 *   5n  When n_r is usable the pixel is not subject to the tangent rule (it is not dropped for lacking neighbours); the row's normal is
 *       n_r plus the usable n_j of the agreeing voters, added componentwise in listed order, divided by its length
 *       sqrt((sx sx + sy sy) + sz sz) (0 or infinite: the pixel is dropped) and turned toward C_r by rule 5's own test.  Otherwise rule 5
 *       stands as it is.
 * No plane in the store and -INFINITY give mvs_fuse_depth_masked's bytes, planes of zeros too, and with min_support = 0 mvs_fuse_depth's.
 * Rows land in the buffer mvs_fuse_points_device returns.
 * Out of scope: mvs_fuse_sequence with normals, TSDF weights from normals, normals for the band and plane-table sweeps, the exact sampler,
 * the C++ seam (host/recon.hpp). */
int mvs_propagate_normals(mvs_ctx *ctx, const float cam[16]);
void *mvs_propagate_normals_device(mvs_ctx *ctx); /* H*W*3 f32; NULL before the first mvs_propagate_normals */
int mvs_propagate_normals_fetch(mvs_ctx *ctx, float *normals_hw3);
int mvs_depth_normals_upload(mvs_ctx *ctx, int slot, const float *normals_hw3);
int mvs_depth_normals_upload_device(mvs_ctx *ctx, int slot, const void *normals_dev);
int mvs_depth_normals_fetch(mvs_ctx *ctx, int slot, float *normals_hw3);
int mvs_depth_normals_drop(mvs_ctx *ctx, int slot);
int mvs_fuse_depth_normals(mvs_ctx *ctx, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px,
                           float max_rel_depth, float max_cost, int min_support, float min_normal_cos, float *out_points7, int *out_count);

/* ---- depth-map plane fit: gated least-squares slopes, a fitted depth, normals and slope seeds (csrc/depth_fit.hip)
 * A least-squares plane through the (2 radius + 1)^2 window of every pixel of a depth map, gated like mvs_depth_filter's window: what a
 * sweep's refined map, a band run's resolved map, a filtered map or a depth-store slot lacks to get normals (their cells hold no slopes),
 * and a better slope seed for the propagation than MVS_PROPAGATE_SLOPES' one-pixel differences.  All arithmetic is f32 with one rounding
 * per operation, no contraction and no FMA; sums run in window (row-major) order and start from 0.0f; bit-identical to
 * tests/depth_fit_mirror.py.
 *   F1. Valid: -1 < z < 1, read as z + 0.0f (rule 1 of mvs_depth_filter).
 *   F2. Window and guide gate: rule 2 of mvs_depth_filter; radius 1..4, |G(q) - G(p)| <= tau in integers, tau = 255 reads no guide.
 *   F3. Members of a valid p: the valid q of the frame that pass the guide gate and whose t(q) = z(q) - z(p) (one rounding) satisfies
 *       fabsf(t) <= max_step (+inf: no depth gate, 0: equal values only).  p is a member.
 *   F4. Moments over the members, dc = q.col - p.col, dr = q.row - p.row: n, Sx = sum dc, Sy = sum dr, Sxx, Sxy, Syy exact in int32;
 *       St = sum t, Sxt = sum (float)dc t, Syt = sum (float)dr t in f32, each product rounded, then added.
 *   F5. The integer adjugate: A00 = Sxx Syy - Sxy^2, A01 = Sy Sxy - Sx Syy, A02 = Sx Sxy - Sy Sxx, A11 = n Syy - Sy^2,
 *       A12 = Sx Sy - n Sxy, A22 = n Sxx - Sx^2, D = n A00 + Sx A01 + Sy A02: exact in int32, every |Aij| < 2^24 (exact as a float),
 *       (float)D one round-to-nearest-even conversion.  p is FITTED when n >= min_members (3..81) and D != 0 (D = 0: the members are
 *       collinear).  Then c = ((A00 St + A01 Sxt) + A02 Syt) / D, gx = ((A01 St + A11 Sxt) + A12 Syt) / D,
 *       gy = ((A02 St + A12 Sxt) + A22 Syt) / D, the division correctly rounded.
 *   F6. Outputs, context-owned: z = z(p) + 0.0f or MVS_BACKGROUND_DEPTH; gx, gy (the depth's change per column and per row, the
 *       propagation's convention), 0 unless fitted; zfit = z(p) + c when p is fitted and the sum is inside (-1, 1), else z; members = n
 *       of a fitted pixel, else 0 (u8).  The report: out[0..3] = valid centres, fitted, refused for n < min_members, refused for D = 0.
 * max_step is in depth units, a few plane steps; the gate keeps the plane from straddling a depth step.  The fit has been measured on
 * smooth maps with bounded noise and on swept maps: outliers inside the gate pull the plane as they pull a mean.
 *   depth_dev: every map mvs_depth_filter accepts, and mvs_depth_fit_depth_device itself: a launch never reads the map it writes (an
 * input that is zfit is fitted into a spare map that is copied over zfit behind the kernel).  guide_dev: H * W u8, NULL = the staged
 * main image.  mvs_depth_fit_device: z, gx, gy, H * W f32 each, one behind the other, in the layout of mvs_propagate_depth_device;
 * mvs_depth_fit_depth_device: zfit, a depth map in the library's convention; mvs_depth_fit_members_device: H * W u8.  All are NULL
 * before the first call and do not change afterwards.  The fetch (each pointer may be NULL) and the report synchronise.  One allocation
 * (33 H W + 8192 bytes) made by the first mvs_depth_fit behind every check; a context that never calls it allocates nothing.  Asynchronous
 * on the context's stream, timed under MVS_K_ARGMIN; the call touches no other state.
 *   mvs_depth_fit_normals: rule N1 (above) on (z, gx, gy) of the last fit for the main camera cam, bit for bit, but a pixel that is not
 * fitted gets (0, 0, 0) and not the fronto-parallel plane rule N1 gives zero slopes.  mvs_depth_fit_normals_device goes into
 * mvs_depth_normals_upload_device unchanged (NULL before the first mvs_depth_fit_normals).
 *   mvs_propagate_set_slopes only records two device pointers (H * W f32 each, e.g. mvs_depth_fit_device + H W and + 2 H W; not the
 * propagation's own slope maps).  The NEXT mvs_propagate_init that passes its checks consumes them: behind rule 5's copy a pixel with a
 * hypothesis takes gx(p), gy(p) from them (a non-finite value as 0), a pixel without one keeps 0; then the cells are evaluated as always
 * and the record is cleared, so the maps must be valid from this call to the end of that init and not longer.  One-shot on purpose: a
 * later init never reads a map the caller may have freed.  Both NULL clears the record.  Recorded slopes together with
 * MVS_PROPAGATE_SLOPES are MVS_EINVAL at init (the record stays).  With nothing recorded init writes the bytes it wrote before.
 * Errors: MVS_EINVAL for a NULL ctx, depth_dev, cam, out or normals array, a radius outside 1..4, tau outside 0..255, a negative or NaN
 * max_step, min_members outside 3..81, a camera mvs_propagate_normals refuses, gx_dev / gy_dev with only one of them NULL; MVS_ESTATE
 * for tau < 255 with a NULL guide and no staged main image, for the fetch, the report and mvs_depth_fit_normals before the first fit, for
 * mvs_depth_fit_normals_fetch before the first mvs_depth_fit_normals; MVS_ENOMEM.  All checks come before the first allocation; after an
 * error nothing is written and the context stays usable.
 * Out of scope: a residual-gated refit, hole filling from the fitted plane, normals in mvs_fuse_sequence and TSDF weights from normals,
 * the exact sampler, the C++ seam (host/recon.hpp). */
int mvs_depth_fit(mvs_ctx *ctx, const void *depth_dev, const void *guide_dev /* NULL: the staged main image */, int radius, int tau, float max_step, int min_members);
void *mvs_depth_fit_device(mvs_ctx *ctx);         /* z, gx, gy: 3 * H*W f32 */
void *mvs_depth_fit_depth_device(mvs_ctx *ctx);   /* zfit: H*W f32 */
void *mvs_depth_fit_members_device(mvs_ctx *ctx); /* H*W u8 */
int mvs_depth_fit_fetch(mvs_ctx *ctx, float *z_hw, float *gx_hw, float *gy_hw, float *zfit_hw, uint8_t *members_hw);
int mvs_depth_fit_report(mvs_ctx *ctx, long long out[4]);
int mvs_depth_fit_normals(mvs_ctx *ctx, const float cam[16]);
void *mvs_depth_fit_normals_device(mvs_ctx *ctx); /* H*W*3 f32 */
int mvs_depth_fit_normals_fetch(mvs_ctx *ctx, float *normals_hw3);
int mvs_propagate_set_slopes(mvs_ctx *ctx, const void *gx_dev, const void *gy_dev /* both NULL: clear */);

/* ---- one main view on several GPUs of one node (SURVEY.md section 8b "multi-GPU", 8e, north_star) -----------------------------
 * A communicator owns one context per listed device and one RCCL communicator across them (librccl is loaded when the first
 * communicator is created; the library has no link dependency on it).  mvs_sweep_sharded runs ONE main view on all of them, one host
 * thread per GPU, and returns the depth map (and best cost) of the whole view -- bit-identical to mvs_sweep on one GPU in every mode
 * (cells are integers, sums are exact):
 *   MVS_SHARD_ROWS (default)  every GPU holds all side views and sweeps a band of the main view's pixel rows, depth selected inside
 *                             the kernel; each band is copied from its GPU into depth_hw / cost_hw.  4 bytes per pixel and map, no
 *                             collective: the split that scales.
 *   MVS_SHARD_VIEWS           the north_star's split: the side views are dealt to the GPUs, every GPU builds the packed volume of its
 *                             views, the volumes are all-reduced over xGMI per plane group (mvs_comm_set_plane_groups, default 4) on
 *                             a second stream while the next group is swept, depth is selected from the sum.  2 (n-1)/n x 4 P D
 *                             bytes per GPU on the links: cannot scale at the BASELINE sizes, built because
 *                             the north_star names it.
 *   MVS_SHARD_VIEWS_SCATTER   the same split, half the bytes, no overlap: reduce-scatter by plane slices + partial selection +
 *                             all-gather of 8-byte partials (nplanes a multiple of the GPU count; otherwise as MVS_SHARD_VIEWS).
 * A rank that fails before the exchange makes every rank skip it (host barrier + shared error flag); a failure inside the exchange
 * aborts all communicators (ncclCommAbort) so that no rank is left waiting; mvs_sweep_sharded then returns MVS_ESTATE until a new
 * communicator is created.  The sampler of a communicator's contexts is set through mvs_comm_context(). */
#define MVS_SHARD_ROWS 0
#define MVS_SHARD_VIEWS 1
#define MVS_SHARD_VIEWS_SCATTER 2
typedef struct mvs_comm mvs_comm;
mvs_comm *mvs_comm_create(const int *devices, int n, int width, int height); /* NULL on error: mvs_comm_last_error(NULL) */
void mvs_comm_destroy(mvs_comm *comm);
int mvs_comm_size(const mvs_comm *comm);
mvs_ctx *mvs_comm_context(mvs_comm *comm, int rank); /* borrowed; NULL if rank is out of range */
const char *mvs_comm_last_error(const mvs_comm *comm);
int mvs_comm_set_mode(mvs_comm *comm, int mode);   /* MVS_SHARD_* */
int mvs_comm_mode(const mvs_comm *comm);
int mvs_comm_set_plane_groups(mvs_comm *comm, int groups); /* MVS_SHARD_VIEWS: plane groups of the all-reduce pipeline, 1..64 */
int mvs_sweep_sharded(mvs_comm *comm, const float main_cam[16], const uint8_t *main_hw, int nviews, const float *side_cams /* nviews*16 */,
                      const uint8_t *const *side_frames, int nplanes, float z_lo, float z_hi, float *depth_hw, float *cost_hw /* nullable */);
/* The RESIDENT form (the staged mvs_sweep_set_* / mvs_sweep_run of one context, for a communicator): a sequence's caller -- the loop of
 * recon.cpp:65-117 over main frames -- uploads once and sweeps many times; nothing crosses PCIe, is re-planned or re-prepared between runs.
 *   mvs_comm_set_planes / _set_main / _set_views   upload to EVERY rank (each keeps all side views and the plan, so any mode can run on them;
 *                        host pointers are not retained: the calls return when the copies have landed).  Like a context, a new main view
 *                        invalidates the side views (their matrices depend on the main camera): set planes, then main, then views.
 *   mvs_comm_run(flags)  one sweep of what is resident, in the current mode; returns when every rank has finished.  The depth and best-cost
 *                        maps of the WHOLE view are left on rank 0's GPU (mvs_sweep_depth_device / _cost_device of mvs_comm_context(comm, 0);
 *                        not the index map): MVS_SHARD_ROWS copies each rank's band there by peer copies over xGMI behind the rank's sweep
 *                        (4 bytes per pixel and map in total, no collective, no host memory); the views modes end with the selection on
 *                        every rank.  flags: 0, or MVS_SWEEP_VOLUME to make MVS_SHARD_ROWS materialise each rank's band of the packed
 *                        volume as well (the views modes always build it).  The persistent rank threads do the work: no thread is created,
 *                        no frame uploaded and no plan made per call.
 *   mvs_comm_fetch       download rank 0's maps (either pointer may be NULL).
 * mvs_sweep_sharded = set_planes + set_main + set_views + run + fetch in one pass over the ranks (in a views mode each rank uploads only its
 * own views, and in rows mode the bands go straight to the caller's host maps); what it uploaded stays resident for mvs_comm_run in the same mode. */
int mvs_comm_set_planes(mvs_comm *comm, int nplanes, float z_lo, float z_hi);
int mvs_comm_set_main(mvs_comm *comm, const float main_cam[16], const uint8_t *main_hw);
int mvs_comm_set_views(mvs_comm *comm, int nviews, const float *side_cams /* nviews*16 */, const uint8_t *const *side_frames);
int mvs_comm_run(mvs_comm *comm, unsigned flags);
int mvs_comm_fetch(mvs_comm *comm, float *depth_hw /* nullable */, float *cost_hw /* nullable */);
/* Two calls in flight (the loop of recon.cpp:65-117 over main views, or a fixed rig's next frames: the gather of view k beside the sweep of
 * view k + 1).  mvs_comm_run_async(comm, 0) QUEUES one sweep of what is resident and returns when every rank's launches are queued -- nobody
 * waits for a GPU: in MVS_SHARD_ROWS each rank's band leaves its context's maps by a device copy behind the sweep and travels to rank 0 on a
 * second stream, into one of two (depth, cost) result pairs on rank 0's device, so the next call's sweep runs beside it; at most two calls are
 * in flight (a third is refused with MVS_ESTATE until mvs_comm_wait).  mvs_comm_wait(comm) waits for the OLDEST call in flight and makes its
 * maps the ones mvs_comm_fetch downloads; they stay valid until the second mvs_comm_run_async after that call.  The view-sharded modes end in
 * collectives that every rank thread drives: there mvs_comm_run_async completes the call before it returns (one in flight at most) and
 * mvs_comm_wait only publishes it.  While calls are in flight mvs_comm_run, mvs_comm_set_* and mvs_sweep_sharded return MVS_ESTATE.
 * Launch failures are returned by mvs_comm_run_async, failures on a GPU by mvs_comm_wait.  mvs_comm_pending: calls in flight (0..2). */
int mvs_comm_run_async(mvs_comm *comm, unsigned flags /* 0 */);
int mvs_comm_wait(mvs_comm *comm);
int mvs_comm_pending(const mvs_comm *comm);
/* Where a rank's band copies travel (the resident MVS_SHARD_ROWS gather: rank r -> rank 0).  mvs_comm_create enables peer access between
 * every rank's device and rank 0's in both directions (hipDeviceCanAccessPeer + hipDeviceEnablePeerAccess; "already enabled" accepted) and
 * keeps the outcome: mvs_comm_peer_access(comm, r) = 1 when rank r's copies go GPU to GPU (xGMI, or r shares rank 0's device; rank 0 itself:
 * 1), 0 when the runtime stages them through host memory -- nothing is refused, a staged band is slow, not wrong; right after creation
 * mvs_comm_last_error(comm) names the ranks concerned ("note: ...").  mvs_comm_device(comm, r): the HIP device ordinal of rank r. */
int mvs_comm_peer_access(const mvs_comm *comm, int rank);
int mvs_comm_device(const mvs_comm *comm, int rank);

/* ---- kernel timing (HIP events on the context's stream) ---------------------------------------- */
#define MVS_K_SWEEP 0
#define MVS_K_ARGMIN 1
#define MVS_K_PLAN 2
#define MVS_K_RASTER 3
#define MVS_K_PROJECT 4 /* Render::projected; the lens launches (mvs_undistort, _device, _map, mvs_frame_upload_lens*) */
#define MVS_K_FLOW 5
#define MVS_K_FUSE 6 /* mvs_fuse_depth: count pass, scan, row pass */
#define MVS_K_TSDF 7 /* mvs_tsdf_integrate: w-map passes and integration launches; mvs_tsdf_raycast: field, brick mask, ray kernel; mvs_tsdf_integrate_frames, _shade, _sample_appearance */
#define MVS_K_COUNT 8
int mvs_profile_enable(mvs_ctx *ctx, int on);
/* synchronises, then returns summed elapsed ms and launch count per kernel class since the last reset */
int mvs_profile_read(mvs_ctx *ctx, float ms_sum[MVS_K_COUNT], int launches[MVS_K_COUNT], int reset);

/* ---- surface meshing: replaces poissonSurface (recon.hpp:37, cgal_poisson.cpp:47-136, pcl.cpp:193-228) ----
 * Poisson reconstruction of oriented samples on a regular grid (csrc/poisson.hip): normals splatted with 64-bit fixed-point atomics,
 * laplace(chi) = div V solved with hipFFT, level set through the samples meshed by surface nets.  Context-free: runs on the calling
 * thread's current HIP device (device 0 unless the caller has set another), on a stream of its own; no CPU path.
 *   points     n rows x, y, z, w (homogeneous, as recon.cpp:121 hands them over);  normals  n rows nx, ny, nz (pointing out of the solid;
 *              a component that is NaN or beyond 1e4 in magnitude makes the sample vote for nothing).  Their lengths act as confidences,
 *              as given -- the reference's semantics on both of its backends (cgal_poisson.cpp:58-69; pcl.cpp:23, 198-202).  The wrappers
 *              with the reference's signature, poissonSurface (host/poisson.cpp) and mvs_amd.poisson_surface, normalise them first BY
 *              DEFAULT: a deliberate divergence (see there for what the pdf lengths of triangulatePixels do to this solver), switchable.
 *              The level is the median of chi over the samples (CGAL's Poisson_reconstruction_function: median value at the input points)
 *   grid_log2  log2 of the nodes per axis, 4..9; 0 = from the samples' average 6-nearest-neighbour spacing, the reference's own
 *              yardstick (CGAL::compute_average_spacing(points, 6), cgal_poisson.cpp:77): the coarsest of 32..512 nodes per axis whose
 *              node spacing is at most 0.75 x that spacing, which keeps the surface within the reference's approximation bound of
 *              0.375 x average spacing (cgal_poisson.cpp:52) on the analytic test surfaces; mvs_surface_spacing reports the average
 *              spacing, the node spacing and whether the ratio could be kept (512 nodes per axis may still be too coarse)
 *   smooth_cells  standard deviation (grid cells) of the Gaussian low-pass applied to chi; 1.0 is a good default
 *   keep_fields  non-zero: keep chi and the splatted integer fields for mvs_surface_grid (tests)
 * The alpha shape of the first iteration (alphaShapeFaces, recon.hpp:33-34) is host-only code: libmvs_host.so, host/alpha_shapes.cpp.
 *   support_spacings (mvs_poisson_surface_ex)  the level set is meshed only in cells within this many average spacings (rounded up to whole
 *              nodes, Chebyshev distance) of a grid node that collected sample weight; 0 = everywhere.  Away from the samples the solved
 *              field is flat and hovers around the level: on open or noisy clouds (what recon.cpp:121 collects from the flows) the level
 *              set there is a closing sheet no sample supports plus numerical fuzz -- 97 % of 16 M vertices on the config-5 cloud of
 *              tests/test_meshing_gpu.py.  The reference's mesher returns such sheets too (coarse ones: its Delaunay refinement has no
 *              resolution where there are no points); this grid would return them at full resolution, so it does not return them at
 *              all.  Closed, evenly sampled surfaces are not affected (every cell of the surface is next to a sample).
 *              mvs_poisson_surface uses MVS_POISSON_SUPPORT_DEFAULT. */
#define MVS_POISSON_SUPPORT_DEFAULT 8.0f
typedef struct mvs_surface mvs_surface;
/* The first hipFFT plan of a grid size in a process costs about 2 s (rocFFT compiles its kernels for the size at run time); every
 * later call of that size finds the plans cached.  mvs_poisson_warmup(grid_log2) pays that cost when the caller chooses -- at start-up,
 * beside mvs_create -- instead of inside the first poissonSurface of a reconstruction: it builds and keeps the two plans of a
 * 2^grid_log2 grid (5..9) on the calling thread's current device.  Optional; returns 0, or a negative MVS_E* code. */
int mvs_poisson_warmup(int grid_log2);
int mvs_poisson_surface(const float *points, const float *normals, int n, int grid_log2, float smooth_cells, int keep_fields, mvs_surface **out);
int mvs_poisson_surface_ex(const float *points, const float *normals, int n, int grid_log2, float smooth_cells, float support_spacings, int keep_fields,
                           mvs_surface **out);
int mvs_surface_support(const mvs_surface *s, int *support_nodes /* the radius used, in nodes; 0: no trimming */);
/* The normals' lengths are confidences (triangulatePixels scales them by a pdf, util.cpp:322-327: 1e-6 .. 1e-4 on real frames) and only
 * their ratios matter; before the fixed-point splat they are multiplied by the power of two that brings their median size into [0.5, 1)
 * (exact; 2^0 for unit normals).  chi and the level of mvs_surface_grid carry that factor. */
int mvs_surface_normal_scale(const mvs_surface *s, int *scale_log2);
int mvs_surface_counts(const mvs_surface *s, int *vertices, int *faces);
int mvs_surface_fetch(const mvs_surface *s, float *vertices /* V x 4, w = 1 */, int32_t *faces /* F x 3, normals along the samples' */);
int mvs_surface_grid(const mvs_surface *s, int *nodes_per_axis, float origin3[3], float *spacing, float *level, float *chi /* G^3, nullable */,
                     int64_t *splat /* 4 G^3: vx, vy, vz, weight in units of 2^-16; nullable */);
int mvs_surface_spacing(const mvs_surface *s, float *average_spacing /* of the samples, 6 nearest neighbours */, float *node_spacing, int *ratio_kept);
/* The facet criteria the reference hands its mesher (cgal_poisson.cpp:50-52, 95-97: CGAL::Surface_mesh_default_criteria_3(sm_angle = 20
 * degrees, sm_radius = 300 x average spacing, sm_distance = 0.375 x average spacing)), as a pass over the surface's triangles
 * (csrc/surface_criteria.cpp; host code, like the reference's mesher): facets whose smallest angle is below min_angle_deg are removed by
 * edge collapses and edge flips between the vertices the mesher placed (no vertex moves, none is added; the link condition keeps the
 * surface a manifold wherever it was one), each guarded so that the surface moves by at most a quarter of max_distance; facets whose
 * circumradius exceeds max_radius are counted (the grid rule of mvs_poisson_surface keeps every facet two orders of magnitude below the
 * reference's bound, so nothing is done about them).  Vertices that lose all their facets are dropped; the order of the others, and of
 * the facets, is kept.  Last, facets that are still below the angle bound and lie on the BORDER of an open surface (where the samples'
 * support cut the level set) are removed when that only moves the border: a facet with two or three border edges, or with one and an
 * interior opposite vertex.  report (nullable) says what was done and what is left.  poissonSurface (host/poisson.cpp) and
 * mvs_amd.poisson_surface apply it with the reference's three numbers. */
typedef struct mvs_criteria_report {
    int collapses, flips;          /* operations applied */
    int facets_below_angle;        /* facets still below min_angle_deg afterwards */
    int facets_above_radius;       /* facets whose circumradius exceeds max_radius */
    float min_angle_deg;           /* smallest facet angle of the result (180 for an empty mesh) */
    float max_circumradius;        /* largest facet circumradius of the result */
    int facets_trimmed;            /* facets below min_angle_deg ON THE BORDER of an open surface that were removed (the border moved; see below) */
} mvs_criteria_report;
int mvs_surface_enforce_criteria(mvs_surface *s, float min_angle_deg /* [0, 60) */, float max_radius, float max_distance, mvs_criteria_report *report);
/* The other half of what those criteria mean: they bound a facet's angles from below and its distance from the surface from above -- NOT
 * its size (sm_radius = 300 spacings) -- so the reference's mesher returns as few facets as the curvature allows, where the grid mesher
 * returns the grid's density.  mvs_surface_simplify removes the vertices the criteria do not need: edge collapses u -> v, shortest edge
 * first, under the guards of mvs_surface_enforce_criteria (link condition, no facet turning over) with every rewritten facet keeping
 * min_angle_deg and every vertex keeping an ACCUMULATED displacement of at most max_distance (a vertex inherits what was merged into it);
 * no vertex moves, none is added, vertices on a border or on a non-manifold edge stay.  Apply after mvs_surface_enforce_criteria.
 * poissonSurface (host/poisson.cpp) and mvs_amd.poisson_surface run it with sm_angle and sm_distance. */
typedef struct mvs_simplify_report {
    int collapses;
    int vertices_before, vertices_after, facets_before, facets_after;
    float max_accumulated_distance;
} mvs_simplify_report;
int mvs_surface_simplify(mvs_surface *s, float min_angle_deg /* [0, 60) */, float max_distance, mvs_simplify_report *report);
/* a surface object over a caller's triangle mesh (vertices V x 4 with w = 1, faces F x 3), e.g. to apply the criteria to it; needs no GPU */
int mvs_surface_from_mesh(const float *vertices, int vertex_count, const int32_t *faces, int face_count, float average_spacing, mvs_surface **out);
void mvs_surface_free(mvs_surface *s);
const char *mvs_surface_last_error(void); /* of the calling thread */

/* library / device info string, e.g. "libmvs_hip gfx950 AMD Instinct MI355X" */
const char *mvs_device_info(mvs_ctx *ctx);

#ifdef __cplusplus
}
#endif
#endif /* MVS_H */
