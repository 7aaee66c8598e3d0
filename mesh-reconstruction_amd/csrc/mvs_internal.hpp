// mvs_internal.hpp -- context layout and helpers shared by the HIP translation units of libmvs_hip.so.
// Not part of the ABI (include/mvs.h is).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <array>
#include <vector>

#include "../../include/mvs.h"
#include "hooks.hpp"

namespace mvs {

// Device buffer that only ever grows; freed with the context.
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
};

// The table of the propagation's geometric term (propagate.hip) as the kernel reads it: per camera P then P^-1,
// row-major -- the main camera first, then the neighbours --, each neighbour's depth map in the depth store, weight * 255 and the cap
struct alignas(16) PropGeo {
    float cam[9][32];
    const float *map[8];
    float w255, max_px;
    int pad[2];
};
static_assert(sizeof(PropGeo) == 1232, "PropGeo is copied to the device and into LDS as 308 words");

struct ProfileSlot {
    hipEvent_t start = nullptr, stop = nullptr;
    int kind = -1;
};

}  // namespace mvs

struct mvs_ctx {
    int device = 0;
    int W = 0, H = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;  // the stream work is queued on (own_stream unless mvs_set_stream)
    char err[512] = {0};
    char info[256] = {0};
    int num_cus = 0;
    mvs::Hooks hooks;                // environment switches as read by mvs_create (all defaults unless MVS_TEST_HOOKS=1: hooks.hpp)
    bool plan_cache = true;          // mvs_sweep_set_plan_cache

    // ---- sweep state (HBM resident) -------------------------------------------------------------
    // main image: H*W u8 tight.  side images: V slabs of (H+2) rows x pad_pitch bytes, 1-pixel
    // GL_REPEAT wrap padding so the sampler never needs wrap logic.
    mvs::DevBuf main_img, side_pads, qmats, ztab, plan, upload;
    mvs::DevBuf volume_own;          // packed (cnt<<16 | sum) cells, [D][H][W] u32
    uint32_t *volume = nullptr;      // volume_own.ptr or caller memory (mvs_sweep_use_volume)
    size_t volume_bytes = 0;
    bool volume_external = false;
    mvs::DevBuf depth, cost, index;  // H*W each
    int sel_planes = 0;              // plane count EVERY row of the index map was last selected over (0: no depth selection); set by the note_*
                                     // transitions below only, compared with D by the readers of the index map (selection_current)
    int sel_band_planes = 0;         // fused row-band runs over a plane count other than sel_planes: that count and the rows [lo, hi) the
    int sel_band_lo = 0, sel_band_hi = 0;  // bands cover so far; sel_planes follows when they cover all rows (note_rows_selected)
    int pad_pitch = 0;
    size_t pad_slab = 0;             // bytes per padded side image
    int V = 0, D = 0;
    float main_cam[16] = {0};
    bool have_main = false, have_views = false, have_planes = false;
    bool plan_valid = false;         // region plan matches current (views, planes)
    int sampler = MVS_SAMPLER_FIXED;  // arithmetic contract of the sweep's texture fetch (mvs_sweep_set_sampler)
    // the sampler whose cell layout the library last wrote the current packed volume / Wv in (-1: unknown -- nothing written yet, or a
    // caller's volume the library has not written since mvs_sweep_use_volume); own_cells_sampler keeps the own volume's while a caller's
    // is in use.  A reader under another sampler would decode the cells wrongly and refuses (mvs::cells_readable)
    // CELLS_MIXED: a row band or plane group was written under another sampler than the rest: no reader until a sweep writes all of it
    static constexpr int CELLS_MIXED = -2;
    int vol_cells_sampler = -1, own_cells_sampler = -1, win_cells_sampler = -1;
    mvs::DevBuf side_quads;          // fixed sampler: quad image of every padded side view (4 bytes per texel), built by mvs_sweep_set_views
    mvs::DevBuf side_quads16;        // exact sampler: f16 quad image (8 bytes per texel), built on demand by ensure_quads16
    bool quads16_valid = false;
    bool pads_valid = false;         // side_pads (wrap-padded u8 frames) matches the current quad images: rebuilt on demand by ensure_pads
    mvs::DevBuf frame_ptrs;          // mvs_sweep_set_views_device: device table of the caller's frame pointers
    std::vector<const uint8_t *> frame_ptrs_host;
    // mvs_sweep_handles: the current main / side views are slots of the frame store (no copies: the kernels read the store)
    bool views_in_store = false;
    int main_store_slot = -1;
    mvs::DevBuf view_slots;          // device: slot of view v
    std::vector<int> view_slots_host;
    mvs::DevBuf fx_lut;              // fixed sampler: 32 x 32 table of packed 8-bit bilinear weights
    int plan_shape = 2;              // what the plan was made for: 1 = exact sampler, 2 px x 32 planes; 2 = exact, 4 px x 16 planes; 3 = fixed sampler
    bool plan_forced = false;        // plan made with the 4 x 16 shape forced (timing experiments)
    mvs::DevBuf plan_stats;          // planner counters (oversize regions, regions not skipped, widest / tallest staged region)
    // rectified fast path of the fixed sampler (sweep_rect.hip): per (tile column | tile row, view, plane) texel + phase + certificates
    mvs::DevBuf rect_tab;
    bool rect_ok = false;            // the current plan can be served by sweep_fx_rect
    // rectified path of the exact sampler (sweep_xrect.hip): box tables, LDS row stride and slot size of the current plan
    mvs::DevBuf xrect_tab;
    bool xrect_ok = false;
    int xrect_rs = 0, xrect_slot_bytes = 0;
    bool exact_tiled_planned = false;  // sweep_tiled's region plan exists for the current (views, planes) (made on demand when xrect_ok)
    int exact_last_shape = 0;          // what served the exact sampler's last run: 1 / 2 (sweep_tiled's thread shapes) or 5 (sweep_exact_rect)
    // what the fixed sampler's plan in memory (rectified tables, general plan) was made for: a new set of views with the SAME view matrices,
    // planes and slots -- a fixed camera rig delivering its next frames -- reuses it instead of planning again
    bool snap_valid = false, snap_in_store = false;
    std::vector<float> snap_q, snap_z;
    std::vector<int> snap_slots;
    mvs::DevBuf sep_tab;             // the separable path's tables for the current (views, planes): sweep_fx.hip, plan_sep_tables
    bool sep_ok = false;
    int sep_dpad = 0;
    size_t sep_r_offset = 0;
    bool fx_general_planned = false; // the general tiled kernel's plan exists for the current (views, planes) (made on demand when rect_ok)
    int rect_rs = 0, rect_slot_dw = 0, rect_dpad = 0;
    std::vector<unsigned char> rect_cold_host;  // host copy of the kernel's cold block (sweep_rect.hip: RectCold)
    bool rect_cold_sent = false;
    std::array<int, 5> rect_order{};  // the region order the X / Y records are packed for: view range, chunk range, chunks per workgroup (sweep_rect.hip: RectOrder)
    hipEvent_t plan_event = nullptr;  // the rectified planner's read-back has landed (the host waits for this, not for the whole stream)
    mvs::DevBuf probe_buf;           // mvs_depth_probe: pixel coordinates in, depths out
    mvs::DevBuf raster_bins;         // face binning of large meshes: per-bin counts / offsets / lists, shared list of large faces
    mvs::DevBuf filter_sort;         // mvs_filter_points, dense clouds: keys and a second copy of the upper lists for the global sorts
    double *filter_pinned = nullptr; // mvs_filter_points: pinned host slots for the convergence value of two iterations in flight
    hipEvent_t filter_ev[2] = {nullptr, nullptr};
    mvs::DevBuf filter_density;      // mvs_filter_points: the two density buffers of the power iteration (no other stage touches them);
    int filter_density_n = 0;        // mvs_filter_density_fetch: N of the last successful call (0: nothing to fetch) and the byte offset of
    size_t filter_density_off = 0;   // the buffer its greedy pass ranked by
    std::vector<float> q_host;       // V*12
    std::vector<float> side_cams_host;  // V*16: the side cameras the current views were staged with (mvs_pyramid_stage hands them to the coarser level)
    std::vector<float> z_host;       // D

    // ---- renderer state -----------------------------------------------------------------------------
    mvs::DevBuf soup;                // 9 floats per face, dehomogenised triangle soup
    int nfaces = 0;
    mvs::DevBuf r_zbuf, r_shadow, r_frame, r_out3, r_tmp0, r_tmp1, r_tmp2, r_mips;
    mvs::DevBuf r_tris_main;         // Render::projected's main pass: the main camera's triangle records (raster.hip: projected_main_pass)
    // Render::projected's frame textures as raster.hip last made them (projected_textures): bytes per frame in r_frame / r_mips, how many frames were
    // prepared up front (mvs_process_frame: all side views at once), and the mip-chain description of one frame (raster.hip's MipArgs, opaque here)
    size_t tex_frame_bytes = 0, tex_mips_bytes = 0;
    int tex_prepared = 0;
    unsigned char tex_mip[256] = {0};
    int texture_filter = MVS_FILTER_MIPMAP;  // Render::projected's frame texture: mip chain + trilinear (the reference's request) or level 0 only
    mvs::DevBuf cubic_tab;           // Q15 bicubic weights for remap (32*32*16 shorts)
    mvs::DevBuf flow_arena;          // optical-flow pyramids and work buffers
    mvs::DevBuf flow_batch_arena;    // the same for the batched Farneback of mvs_process_frame (all side views of a main frame per launch)
    mvs::DevBuf frame_buf;           // mvs_process_frame: frames, depth, warped image, flows of one main frame
    mvs::DevBuf best_parts;          // plane-split sweeps: partial (best cell, best index) per split and pixel
    // frame store (mvs_frame_store / mvs_frame_upload / mvs_sweep_batch): the frames of a sequence, uploaded once, each as raw frame,
    // quad image (5 bytes per pixel); main and side views of the batched sweep are slots of it
    mvs::DevBuf store_raw, store_quads;
    // mvs_sweep_batch_async: two batches in flight, each with its own device block and host staging; the results of a batch travel on
    // the copy stream while the next batch is planned and swept on the context's stream
    struct BatchSlot {
        mvs::DevBuf buf;
        std::vector<char> host;
        hipEvent_t swept = nullptr, landed = nullptr;  // kernel done (copy stream waits for it) / results in the caller's memory
        bool busy = false;
    } batch_slot[2];
    int batch_next = 0;
    hipStream_t copy_stream = nullptr;
    int onecall_bands_last = 0;           // row bands of the last mvs_sweep (test hook mvs_test_onecall_bands)
    std::vector<hipEvent_t> band_events;  // mvs_sweep's band pipeline: rows uploaded / band swept, per band
    int store_cap = 0;
    std::vector<unsigned char> store_have;
    // lens (lens.hip: mvs_set_lens / mvs_undistort* / mvs_frame_upload_lens): the radial coefficients and the centre in pixels (y from the
    // bottom) while lens_set; lens_stage is the W*H staging frame of mvs_frame_upload_lens, allocated by its first use
    bool lens_set = false;
    float lens_k[3] = {0.f, 0.f, 0.f};
    float lens_cx = 0.f, lens_cy = 0.f;
    mvs::DevBuf lens_stage;
    // mvs_process_frame runs the flows of one main frame's side views concurrently, one lane each:
    // A lane: the stream one side view's flow runs on, a SHADOW context that stands for this context on that stream (device, size, hooks; its own flow
    // arena; nothing else is used through it) and a host thread that queues the flow's launches while the calling thread goes on with the next side
    // view (pipeline.hip: a main frame is ~150 launches at ~6 us of host time each, the calling thread alone was the bottleneck).
    struct FlowLane {
        hipStream_t stream = nullptr;
        mvs_ctx *shadow = nullptr;
        void *worker = nullptr;   // pipeline.hip: LaneWorker
    };
    static constexpr int kFlowLanes = 4;
    FlowLane lanes[kFlowLanes];
    std::vector<hipEvent_t> lane_events;  // 2 per side view: inputs ready, flow done

    // depth store (fuse.hip: mvs_depth_store / mvs_depth_upload / mvs_fuse_depth): per slot an H*W f32 depth map, an H*W f32 cost map
    // and the camera's matrices as the fusion kernels use them (host copy; they travel as kernel arguments)
    struct DepthSlot {
        bool have = false, have_cost = false;
        bool have_support = false;  // the slot's plane of dstore_support describes the stored map (mvs_depth_support_upload; a depth upload clears it)
        bool have_normals = false;  // the slot's plane of store_normals describes the stored map (mvs_depth_normals_upload; a depth upload clears it)
        float P[16], Pi[16], C[4];
    };
    mvs::DevBuf dstore_depth, dstore_cost;
    mvs::DevBuf dstore_support;  // support planes (section 28): capacity planes of H*W u8, made by the first support upload, freed by mvs_depth_store
    // normals (normals.hip, section 31): capacity planes of H*W*3 f32 beside the depth store, made by the first normals upload and freed by
    // mvs_depth_store; the H*W*3 f32 map of the last mvs_propagate_normals, made by its first call (hyp_normals_have: one has run)
    mvs::DevBuf store_normals, hyp_normals;
    bool hyp_normals_have = false;
    std::vector<DepthSlot> dstore;
    mvs::DevBuf fuse_rows, fuse_counts, fuse_scan;  // rows of the last mvs_fuse_depth; per-segment keep counts and their offsets; scan scratch
    bool fuse_have_rows = false;
    // sequence fusion (fuse_sequence.hip: mvs_fuse_sequence, section 28): the rows of the last call; one H*W u8 claim plane per distinct slot
    // it named; the running total (i64) followed by the per-reference counts (i32).  All three are made by the first call that needs them.
    mvs::DevBuf fuse_seq_rows, fuse_seq_claims, fuse_seq_state;
    bool fuse_seq_have_rows = false;
    // TSDF volume (tsdf.hip: mvs_tsdf_volume / mvs_tsdf_integrate / mvs_tsdf_surface): G^3 f32 sums then G^3 i32 counts; the w-maps of one
    // integration launch; the field and support mask mvs_tsdf_surface meshes.  tsdf_G = 0: no volume yet.
    mvs::DevBuf tsdf_vol, tsdf_wmaps, tsdf_work;
    int tsdf_G = 0;
    float tsdf_origin[3] = {0.f, 0.f, 0.f};
    float tsdf_h = 0.f, tsdf_inv_tau = 0.f;
    // ray-cast of the volume (raycast.hip: mvs_tsdf_raycast): tsdf_work holds the field F and cell mask of tsdf_field_key's min_observations
    // (0: stale; mvs_tsdf_surface writes it too), tsdf_bricks the brick bitmask made from that field for tsdf_brick_key (0: stale);
    // the W x H depth map and normal map of the last raycast
    int tsdf_field_key = 0, tsdf_brick_key = 0;
    mvs::DevBuf tsdf_bricks, ray_depth, ray_normals;
    bool ray_have = false;
    bool ray_plain = false;          // test hook mvs_test_raycast_plain: march without the brick mask (timing A/B, tests)
    // appearance of the volume (tsdf.hip: mvs_tsdf_integrate_frames; appearance.hip: mvs_tsdf_shade / mvs_tsdf_sample_appearance): one packed
    // u32 cell per node (count << 24 | sum of u8 intensities), there only while tsdf_app_have (mvs_tsdf_volume drops it; the first
    // mvs_tsdf_integrate_frames or mvs_tsdf_appearance_upload after it makes a zeroed one); the W x H map of u8 pairs of the last shade; the
    // points and values of one mvs_tsdf_sample_appearance
    mvs::DevBuf tsdf_app, shade_map, app_points;
    bool tsdf_app_have = false, shade_have = false;
    // semi-global aggregation (aggregate.hip: mvs_sweep_aggregate): the capped matching costs C and the path sums S, u16 [D][H][W] each;
    // agg_planes = D of the last call (0: nothing aggregated yet)
    mvs::DevBuf agg_cost, agg_sum;
    int agg_planes = 0;
    // cleaning of the selected maps (clean.hip: mvs_sweep_clean): H*W i32 labels followed by H*W i32 roots, the H*W i32 component sizes
    // (valid while clean_have_sizes: the last clean ran the speckle filter) and the report's four counters (valid once clean_done).
    // Allocated by the first call that needs them.
    mvs::DevBuf clean_labels, clean_sizes, clean_counters;
    bool clean_done = false, clean_have_sizes = false;
    // windowed matching cost (window.hip: mvs_sweep_window): Wv, packed cells [D][H][W] u32, allocated by the first call; win_planes = D of
    // the last call (0: no Wv yet); volume_source = which packed volume argmin / refine / aggregate / clean read (mvs::reader_volume)
    mvs::DevBuf win_vol;
    int win_planes = 0;
    int volume_source = MVS_VOLUME_RAW;
    // band sweep (band.hip: mvs_sweep_run_band): the context's copy of the prior, the absolute depths of the last mvs_sweep_band_resolve and
    // its report's four counters, H*W f32 / H*W f32 / 4 i32, each allocated by the first call that needs it.  band_planes = D of the last
    // band run while the maps are still its (0: none yet, or an ordinary sweep ran since); band_resolved: band_depth belongs to that run
    mvs::DevBuf band_prior, band_depth, band_counters;
    int band_planes = 0;
    bool band_resolved = false;
    // resolution pyramid (pyramid.hip): as the COARSE level of mvs_pyramid_stage, the (V + 1) half-resolution frames (main, then the side
    // views) its staged state was made from, allocated by the first call; the two events that order this context's stream against the
    // other level's ([0]: recorded when another stream is about to read this context's buffers, [1]: behind a kernel this context's
    // stream ran on the other level's buffers), created by the first pyramid call, without timing
    mvs::DevBuf pyr_frames;
    hipEvent_t pyr_events[2] = {nullptr, nullptr};
    // depth-map filter (depth_filter.hip: mvs_depth_filter): the filtered map followed by the intermediate map of a two-stage call, H*W f32
    // each, one allocation made by the first call; dfilter_have: a call has written the filtered map
    mvs::DevBuf dfilter_maps;
    bool dfilter_have = false;
    // depth-map plane fit (depth_fit.hip: mvs_depth_fit): z, gx, gy, zfit, a spare map and the normals (8 H*W f32), the report's
    // 64-bit counters (64 stripes of four) and the members' bytes in one allocation made by the first call; dfit_have: a fit has run, dfit_normals_have:
    // mvs_depth_fit_normals has.  dfit_seed_gx / _gy: what mvs_propagate_set_slopes recorded for the next mvs_propagate_init (NULL: nothing)
    mvs::DevBuf dfit_maps;
    bool dfit_have = false, dfit_normals_have = false;
    const void *dfit_seed_gx = nullptr, *dfit_seed_gy = nullptr;
    // hypothesis propagation (propagate.hip: mvs_propagate_init / mvs_propagate_run): z, gx, gy (H*W f32 each), the packed cells (H*W u32)
    // and the cost map (H*W f32) in one allocation, and the report's four 64-bit counters, both made by the first init; prop_have: an init
    // has run; what it recorded (cost, radius, keep, the view range) and the iterations run since
    mvs::DevBuf prop_maps, prop_counters;
    bool prop_have = false;
    int prop_cost = 0, prop_radius = 0, prop_keep = 0, prop_view_first = 0, prop_view_count = 0;
    long long prop_iter = 0;
    // its guide gate (section 26): what mvs_propagate_set_gate recorded for the next init, and what the last init took -- tau and whether
    // the guide is the stage's own copy (H*W u8 behind the five maps) or the main image
    int prop_gate_tau = 255;
    const void *prop_gate_guide = nullptr;
    int prop_tau = 255;
    bool prop_guide_own = false;
    // its geometric term (section 27): what mvs_propagate_set_consistency recorded for the next init (prop_cons_n = 0: off), and what
    // the last init took -- how many neighbours, their slots, the depth store's capacity then, and the host copy of the table the
    // kernel reads, which sits behind the guide bytes and the H*W support bytes of prop_maps
    int prop_cons_n = 0, prop_cons_slots[8] = {0};
    float prop_cons_weight = 0.f, prop_cons_max_px = 0.f;
    int prop_geo_n = 0, prop_geo_slots[8] = {0};
    size_t prop_geo_cap = 0;
    mvs::PropGeo prop_geo = {};

    // ---- profiling -----------------------------------------------------------------------------------
    bool profiling = false;
    std::vector<mvs::ProfileSlot> slots;
    size_t slots_used = 0;
};

namespace mvs {

int fail(mvs_ctx *ctx, int code, const char *fmt, ...);
void set_global_error(const char *msg);

#define MVS_HIP(ctx, call)                                                                         \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return mvs::fail((ctx), MVS_EHIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                             __FILE__, __LINE__);                                                  \
    } while (0)

// grow-only device allocation
int ensure(mvs_ctx *ctx, DevBuf &b, size_t bytes);

// bracket a kernel launch with events when profiling is on
struct ProfileScope {
    mvs_ctx *ctx;
    int slot;
    ProfileScope(mvs_ctx *c, int kind);
    ~ProfileScope();
};

// host camera math (double precision; order of operations is part of the parity contract)
void invert4(const double m[16], double out[16]);
void view_matrix(const float main_cam[16], const float side_cam[16], int W, int H, float Q[12]);
void plane_table(int D, float z_lo, float z_hi, float *z);
// fuse.hip: the matrices of a depth slot from its camera (P, P^-1 and the centre); false for a camera with a
// non-finite entry, a singular one, or one without a finite centre.  mvs_tsdf_raycast takes its camera through it too.
bool slot_matrices(const float cam[16], mvs_ctx::DepthSlot &s);
// depth_fit.hip: behind mvs_propagate_init's seed kernel, the slope maps mvs_propagate_set_slopes recorded go into gx, gy at the pixels
// whose z holds a hypothesis, and the record is cleared (nothing recorded: nothing happens)
void dfit_seed_slopes(mvs_ctx *ctx, const float *z, float *gx, float *gy);
// tsdf.hip: F and the cell mask of the volume for min_obs into ctx->tsdf_work, unless they are there already (launches on ctx->stream)
int tsdf_ensure_field(mvs_ctx *ctx, int min_obs);
// tsdf.hip: the appearance volume, allocated and zeroed unless it is there (ctx->tsdf_app_have)
int tsdf_ensure_appearance(mvs_ctx *ctx);

inline int div_up(int a, int b) { return (a + b - 1) / b; }

// select.hip: the packed volume the readers of mvs_sweep_set_volume_source read -- the raw volume as the context holds it (pointer and size
// may be null / short: the reader's own checks apply), or Wv; MVS_ESTATE under MVS_VOLUME_WINDOWED without a Wv of the current planes
int reader_volume(mvs_ctx *ctx, const char *who, const uint32_t *&vol, size_t &bytes);

// what the readers test next, each with its own refusal: the bytes a packed volume of the current planes takes, whether (vol, bytes) is
// one, and whether the index map is a selection over the current planes
inline size_t volume_need(const mvs_ctx *ctx) { return (size_t)ctx->W * ctx->H * (size_t)ctx->D * sizeof(uint32_t); }
inline bool volume_holds_planes(const mvs_ctx *ctx, const uint32_t *vol, size_t bytes) { return ctx->have_planes && vol && bytes >= volume_need(ctx); }
inline bool selection_current(const mvs_ctx *ctx) { return ctx->sel_planes == ctx->D; }

// The state DESIGN.md section 30 tabulates (sel_planes, sel_band_*, band_planes, band_resolved, the three *_cells_sampler, win_planes;
// section 13 for the selection) changes through these transitions only; tests/test_shadow_cpu.py holds that over the sources.
// A writer of every row of ctx->index has been launched over the current planes:
inline void note_full_selection(mvs_ctx *ctx)
{
    ctx->sel_planes = ctx->D;
    ctx->sel_band_planes = 0;
}
// a fused run has rewritten rows [r0, r1) of the index map over the current planes (select.hip):
void note_rows_selected(mvs_ctx *ctx, int r0, int r1);
// the volume was rewritten without a selection on it: refinement, cleaning and the band resolve wait for one (mvs_sweep_argmin, ...)
inline void note_no_selection(mvs_ctx *ctx) { ctx->sel_planes = ctx->sel_band_planes = 0; }
// an ordinary sweep has run: the volume and the maps stop being a band run's (mvs_sweep_band_resolve refuses from here on)
inline void note_ordinary_sweep(mvs_ctx *ctx) { ctx->band_planes = 0; }
// the prior buffer was rewritten behind a band run (mvs_pyramid_prior): the offsets in the depth map were measured from the old prior
inline void note_new_prior(mvs_ctx *ctx) { ctx->band_planes = 0; }
// a sweep has written cells into the current packed volume: they have the layout of the current sampler
inline void note_volume_written(mvs_ctx *ctx) { ctx->vol_cells_sampler = ctx->sampler; }
// a band run has been launched: the volume and the maps are its, and no resolve of it has run yet
inline void note_band_run(mvs_ctx *ctx)
{
    ctx->band_planes = ctx->D;
    ctx->band_resolved = false;
}
// mvs_sweep_band_resolve has been launched: band_depth belongs to the last band run
inline void note_band_resolved(mvs_ctx *ctx) { ctx->band_resolved = true; }
// the epilogue of a fixed-sampler sweep entry (sweep_shared.hpp: fx_sweep_run) that wrote all rows and planes: a band run or an ordinary
// one, with or without the volume, with or without a depth selection
inline void note_fx_sweep(mvs_ctx *ctx, bool band, bool vol, bool fused)
{
    band ? note_band_run(ctx) : note_ordinary_sweep(ctx);
    if (vol) note_volume_written(ctx);
    fused ? note_full_selection(ctx) : note_no_selection(ctx);
}
// mvs_sweep_run has written the whole volume or a row band / plane group of it: a part written under another sampler than the rest was
// written with leaves cells of both layouts until a sweep writes all of it
inline void note_volume_part_written(mvs_ctx *ctx, bool whole)
{
    if (whole || ctx->vol_cells_sampler == -1 || ctx->vol_cells_sampler == ctx->sampler)
        note_volume_written(ctx);
    else
        ctx->vol_cells_sampler = mvs_ctx::CELLS_MIXED;
}
// mvs_sweep_window has been launched over the current planes / has replaced Wv's buffer and not yet launched
inline void note_window_written(mvs_ctx *ctx)
{
    ctx->win_planes = ctx->D;
    ctx->win_cells_sampler = ctx->sampler;
}
inline void note_no_window(mvs_ctx *ctx) { ctx->win_planes = 0; }
// mvs_sweep_use_volume is about to hand the packed volume over (ctx->volume_external still says whose it was): the own volume's layout is
// kept while a caller's is in use and comes back with it; the library has not written the caller's cells
inline void note_volume_swapped(mvs_ctx *ctx, bool to_external)
{
    if (to_external) {
        if (!ctx->volume_external) ctx->own_cells_sampler = ctx->vol_cells_sampler;
        ctx->vol_cells_sampler = -1;
    } else if (ctx->volume_external) {
        ctx->vol_cells_sampler = ctx->own_cells_sampler;
    }
}
// select.hip: MVS_ESTATE when cells written under `cells_sampler` (-1: unknown, readable) would be decoded in the current sampler's layout,
// or when they are a mixture of both layouts (CELLS_MIXED)
int cells_readable(mvs_ctx *ctx, const char *who, const char *what, int cells_sampler);

// the sweep's input setters with the final synchronisation optional (context.hip; mvs_sweep queues all of them and waits once)
int sweep_set_main_impl(mvs_ctx *ctx, const float main_cam[16], const uint8_t *main_hw, bool sync, bool device = false);
int sweep_set_views_impl(mvs_ctx *ctx, int nviews, const float *side_cams, const uint8_t *const *side_frames, bool sync, bool defer_frames = false, bool device = false);
int sweep_upload_frames_impl(mvs_ctx *ctx, const uint8_t *const *side_frames, bool device = false);
struct PlanHook {  // work a caller wants queued between the planner's launches and the planner's one host read-back (it then runs while the host waits)
    virtual int run() = 0;
    virtual ~PlanHook() = default;
};
int sweep_fx_plan(mvs_ctx *ctx, PlanHook *between = nullptr);  // sweep_fx.hip: the fixed sampler's region plan (rectified tables or the general plan)
int ensure_pads(mvs_ctx *ctx);     // wrap-padded u8 frames of the current side views, rebuilt from the quad images when a path needs them
int sweep_upload_rows_impl(mvs_ctx *ctx, const uint8_t *const *side_frames, int r0, int r1, hipStream_t s);  // context.hip: band pipeline of mvs_sweep
int sweep_build_quads_impl(mvs_ctx *ctx, int q0, int q1);
int sweep_rect_plan(mvs_ctx *ctx, PlanHook *between = nullptr);   // sweep_rect.hip: tables + eligibility of the rectified kernel for the current fixed-sampler plan
struct SweepParams;
int ensure_quads16(mvs_ctx *ctx);  // exact sampler's f16 quad image of the current side views  // the deferred half of sweep_set_views_impl
int sweep_set_planes_impl(mvs_ctx *ctx, int nplanes, float z_lo, float z_hi, bool sync);

// device-buffer forms used by the flow stage (photometric.hip)
int compare_device(mvs_ctx *ctx, const uint8_t *prev8, const uint8_t *next8, float *out);
int remap_device(mvs_ctx *ctx, const float *flow, int stride, const uint8_t *img, uint8_t *out);
// the same for B pairs per launch (photometric.hip): compare(prev, next_i), flowRemap(flow_i, img_i)
int compare_batch_device(mvs_ctx *ctx, const uint8_t *prev8, const uint8_t *next8, int B, float *out);
int remap_batch_device(mvs_ctx *ctx, const float *flow, int stride, ptrdiff_t flow_z, const uint8_t *img, int B, uint8_t *out);
int ensure_cubic_table(mvs_ctx *ctx);
// lens.hip: nframes tightly packed W*H frames through the context's lens in one launch on ctx->stream (lens set, ranges disjoint: the caller checks)
int undistort_launch(mvs_ctx *ctx, const uint8_t *src_dev, uint8_t *dst_dev, int nframes);
// raster.hip / flow.hip / triangulate.hip on device buffers (pipeline.hip strings them together)
int depth_device(mvs_ctx *ctx, const float cam[16], float *out_dev);
int projected_device(mvs_ctx *ctx, const float cam[16], const uint8_t *frame_dev, const float projector[16], uint8_t *out3_dev);
int projected_main_pass(mvs_ctx *ctx, const float cam[16]);   // the half of projected() that does not depend on the side view ...
int projected_side_pass(mvs_ctx *ctx, const uint8_t *frame_dev, const float projector[16], uint8_t *out3_dev, int prepared_view = -1, const uint8_t *mix_bg = nullptr,
                        float *mix_depth = nullptr, uint8_t *mix_out = nullptr);   // ... and the half that does
int projected_prepare_views(mvs_ctx *ctx, const uint8_t *const *frames_dev, int nframes);   // the frame textures (wrap padding + mip chain) of nframes (<= 32) side frames, a device pointer each, per launch
int mix_background_device(mvs_ctx *ctx, const uint8_t *img3_dev, const uint8_t *bg_dev, float *depth_dev, uint8_t *out_dev);
// calculateFlow's Farneback window is (H + W) / 100 (flow.cpp:24): 0 below H + W = 100, where the box scale 1 / window^2 is infinite and every flow NaN.
// MVS_EINVAL with a message that names the window; checked by every entry point before it queues anything.  The variational form has no window.
int flow_check_window(mvs_ctx *ctx, int use_farneback, const char *who);
int flow_device(mvs_ctx *ctx, const uint8_t *prev_dev, const uint8_t *next_dev, int use_farneback, float *out4_dev);
int flow_only_device(mvs_ctx *ctx, const uint8_t *prev_dev, const uint8_t *next_dev, int use_farneback, float *flow2_dev);  // without the variance channel ...
int flow_variance_batch_device(mvs_ctx *ctx, const uint8_t *prev8, const uint8_t *next8, const float *flow2, int B, uint8_t *r8, float *var, float *out4);  // ... which this adds for B flows per launch
int flow_farneback_batch_device(mvs_ctx *ctx, const uint8_t *prev_dev, const uint8_t *next_dev, int B, float *out4_dev);  // next: B frames, W*H bytes apart
int triangulate_impl(mvs_ctx *ctx, int nviews, const float *const *flows, bool on_device, const float main_cam[16],
                     const float *side_cams, const float *depth, float *out_points7, int *out_count);
void lanes_shutdown(mvs_ctx *ctx);   // pipeline.hip: joins the lane threads, frees the shadows' arenas (mvs_destroy)
int compare_prepare(mvs_ctx *ctx, int pairs = 1);  // allocates compare_device's arena (for `pairs` image pairs per launch: compare_batch_device)

}  // namespace mvs
