// sweep_shared.hpp -- what the two sweep samplers (sweep.hip: exact f32, contract v1; sweep_fx.hip: fixed point, contract v2)
// have in common: launch parameters, the projective arithmetic up to s and r = RN(1/s.w), the XCD-aware tile order, and the host-side
// decisions every sweep entry makes alike (outputs, cell layout) and the one body of the fixed-point entries beside mvs_sweep_run --
// the ZNCC, best-K, band, band best-K and gated sweeps: fx_sweep_run, with their preconditions and the sampler's limits.  The packed cells
// and the rules of depth selection are select_rules.hpp's; the state the body leaves is mvs_internal.hpp's note_fx_sweep.
#pragma once
#include "mvs_internal.hpp"
#include "select_rules.hpp"

#include <climits>
#include <type_traits>

namespace mvs {

typedef _Float16 half4_t __attribute__((ext_vector_type(4)));

constexpr int TILE_W = 64;   // one wavefront spans a tile row
// sweep_tiled is instantiated for two thread shapes with 64 accumulators each (NPX pixels x PC planes per thread, tile
// height 4 * NPX): 2 x 32 amortises the per-(pixel, view) set-up and the staged texels over twice as many planes
// (c3: 2.20 -> 2.09 ms) but needs the warped footprint of 32 consecutive planes to fit the LDS region; 4 x 16 is the
// fallback when the planner reports oversize regions (wide baselines with few planes).  Chosen per plan, see sweep_run_exact.
constexpr int PCG = 16;          // planes per accumulator batch of the un-tiled generic kernel
constexpr int ROW_GRAN = 16;     // public row granularity: a multiple of both tile heights
constexpr int PLANE_GRAN = 32;   // public plane granularity: a multiple of both chunk sizes
constexpr int LDS_QUADS = 5120;  // 40 KiB of 8-byte quads per staging buffer
constexpr int MAX_RW = 192;
constexpr float PLAN_MARGIN = 0.0625f;

enum RegionMode : unsigned { R_SKIP = 0, R_FAST = 1, R_BORDER = 2, R_GENERIC = 3 };

// The timing-experiment switches: bits 8-15 of mvs_sweep_run's flags, honoured only under MVS_DEBUG_FLAGS=1 (sweep_run_impl) and handed to
// the kernels in SweepParams::debug.  Tests and tools pass them as numbers, so the values stay.  Results are bit-identical with any of
// them set, DBG_NO_STAGING excepted.
enum SweepDebug : int {
    DBG_NO_STAGING = 1,       // sweep_tiled: skip the LDS staging of the side regions (wrong results; times everything else)
    DBG_LINEAR_TILES = 2,     // sweep_tiled, sweep_fx_tiled: block id = tile id instead of the XCD-aware grouped order
    DBG_NO_CONST_W = 4,       // sweep_tiled, sweep_fx_tiled: never take the plane-independent-w path
    DBG_FORCE_4X16 = 8,       // exact sampler, host side: sweep_tiled in its 4 x 16 shape, never 2 x 32 or sweep_exact_rect
    DBG_FX_NO_HALF_COL = 8,   // the same bit in sweep_fx_tiled: no half-column path (the next region is not staged ahead)
    DBG_NO_PAIRED_READS = 16  // sweep_tiled<2, 32>: general cameras take the plain sample loop, not the hand-pipelined one
};

// mvs_sweep_run's `flags`, decoded once by sweep_run_impl
struct SweepFlags {
    bool vol, fused, generic, no_rect;  // MVS_SWEEP_VOLUME, _FUSED_ARGMIN, _FORCE_GENERIC, _NO_RECT
    int debug;                          // SweepDebug bits
    int forced_split;                   // plane-split count forced by a timing experiment; 0: the launcher's target decides
};

struct SweepParams {
    const uint8_t *__restrict__ main_img;
    const uint8_t *__restrict__ pads;
    size_t pad_slab;
    int pitch;
    const uint32_t *__restrict__ quads;  // fixed sampler: per view (H+2) x pitch packed bilinear footprints (t00, t01, t10, t11); pad_slab dwords per view
    const uint2 *__restrict__ quads16;   // exact sampler: per view (H+2) x pitch f16 quads {t00 + 0.5, t01 - t00, t10 - t00, dxy}; pad_slab quads per view
    int W, H, D, V;
    int v0, vcount;
    const float *__restrict__ Q;  // V * 12
    const float *__restrict__ z;  // D
    uint32_t *__restrict__ volume;
    float *__restrict__ depth;
    float *__restrict__ cost;
    int *__restrict__ index;
    float invW, invH;
    float Wp, Hp;  // W + 0.5, H + 0.5
    const uint2 *__restrict__ plan;
    int tiles_x, tiles_y, nchunks;
    int chunk0, chunk1;  // plane chunks [chunk0, chunk1) processed by this launch
    int ty0, tyn;        // tile rows [ty0, ty0 + tyn) processed by this launch (row-band sharding)
    int tile_h, pc;      // shape of the tiled kernel this plan was made for (tile height, planes per chunk)
    int row_begin, row_end, plane_begin, plane_end;  // the same ranges in pixels / planes (generic kernel)
    int *__restrict__ plan_stats;  // [0] regions too large for LDS, [1] regions not skipped (planner output)
    int cps;             // plane chunks per workgroup: blockIdx.y selects chunks [chunk0 + y*cps, +cps) of a tile
    uint2 *__restrict__ part;  // plane-split launches with fused depth selection: [gridDim.y][P] partial bests
    const int *__restrict__ view_slot;  // nullable: slab of view v's padded / quad image (frame store slots, mvs_sweep_batch); null = slab v
    // separable path of the fixed sampler's general kernel (sweep_fx.hip: plan_sep_tables; null = not available): for views whose matrix has
    // q1 = q4 = q8 = q9 = 0 (a camera with the main camera's orientation, anywhere), RN(1 / s.w) per (view, plane) and the row part of both LDS
    // addresses per (view, image row, plane)
    const float *__restrict__ sep_r;   // [V][sep_dpad]
    const uint2 *__restrict__ sep_y;   // [V][H][sep_dpad]: (ky << 10, iy << 10)
    int sep_dpad, sep_reserved;
    int debug;  // timing experiments only: SweepDebug bits
};

// ------------------------------------------------------------------------------------------------------
// shared sample arithmetic
// ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float rcp_rn(float w)
{
    // v_rcp_f32 is accurate to 1 ulp; one Newton step with FMA yields the correctly rounded
    // reciprocal (Markstein) for every w whose significand is not all ones -- verified
    // exhaustively on the device by tests/test_sweep_gpu.py::test_rcp_newton_exact.
    const float r0 = __builtin_amdgcn_rcpf(w);
    const float e = __builtin_fmaf(-w, r0, 1.0f);
    return __builtin_fmaf(e, r0, r0);
}

struct Affine {
    float ax, ay, aw;
};

__device__ __forceinline__ Affine view_affine(const float *__restrict__ q, float xn, float yn)
{
    Affine a;
    a.ax = __builtin_fmaf(q[0], xn, __builtin_fmaf(q[1], yn, q[3]));
    a.ay = __builtin_fmaf(q[4], xn, __builtin_fmaf(q[5], yn, q[7]));
    a.aw = __builtin_fmaf(q[8], xn, __builtin_fmaf(q[9], yn, q[11]));
    return a;
}

template <int CS = CS_EXACT>
__device__ __forceinline__ void store_best(const SweepParams &p, size_t pix, uint32_t bs, uint32_t bc, int bi)
{
    p.depth[pix] = bi >= 0 ? p.z[bi] : MVS_BACKGROUND_DEPTH;
    p.cost[pix] = bi >= 0 ? cell_cost<CS>(bs, bc) : __builtin_inff();
    p.index[pix] = bi;
}


// ------------------------------------------------------------------------------------------------------
// the windowed sweeps' tile (zncc.hip: sweep_fx_zncc, bestk.hip: sweep_fx_bestk) and the two window elements
// ------------------------------------------------------------------------------------------------------
constexpr int ZN_TW = 32, ZN_TH = 16;    // pixels per tile
constexpr int ZN_THREADS = 256;          // two pixels each
constexpr int ZN_PC = 2;                 // planes per accumulator chunk (4 and 8 spill scalar registers: DESIGN.md section 21)
constexpr float ZN_MAGIC = 12582912.0f;  // 1.5 * 2^23, as sweep_fx.hip's FX_MAGIC

template <int R>
struct ZnShape {
    static constexpr int HW = ZN_TW + 2 * R, HH = ZN_TH + 2 * R;               // tile + halo
    static constexpr int SAMPLES = HW * HH, ROWSUMS = HH * ZN_TW;              // elements of the two LDS buffers
    static constexpr int NS = (SAMPLES + ZN_THREADS - 1) / ZN_THREADS;         // samples per thread (3 or 4)
    static constexpr int NR = (ROWSUMS + ZN_THREADS - 1) / ZN_THREADS;         // row sums per thread (3)
};

__device__ __forceinline__ uint4 add4(uint4 a, uint4 b) { return make_uint4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// band.hip's sample (sweep_fx.hip: sample_global_fx) -> the window element of the position: a = A(q), aa = a a.  A position outside the
// main frame carries NaN in its affine part, which fails the sampler's own s.w > 0 test like a sample outside the view's frame
__device__ __forceinline__ uint4 zncc_sample(const Affine &A, float bx, float by, float bw, float z, const uint32_t *__restrict__ quads, uint32_t pitch, float hix, float hiy,
                                             const uint32_t *__restrict__ lut, uint32_t a, uint32_t aa)
{
    const float sx = __builtin_fmaf(z, bx, A.ax), sy = __builtin_fmaf(z, by, A.ay), sw = __builtin_fmaf(z, bw, A.aw);
    const float r256 = rcp_rn(sw) * 256.0f;
    const float tx = __builtin_fmaf(sx, r256, ZN_MAGIC + 4.0f), ty = __builtin_fmaf(sy, r256, ZN_MAGIC + 4.0f);
    const bool ok = sw > 0.0f && tx > ZN_MAGIC + 132.0f && tx < hix && ty > ZN_MAGIC + 132.0f && ty < hiy;  // false for NaN
    const uint32_t ux = __builtin_bit_cast(uint32_t, tx) & 0x3fffffu, uy = __builtin_bit_cast(uint32_t, ty) & 0x3fffffu;  // t - magic
    const uint32_t quad = quads[ok ? (uy >> 8) * pitch + (ux >> 8) : 0u];   // in frame: column <= W, row <= H of the (H + 2) x pitch quad image
    const uint32_t w = lut[(((uy >> 3) & 31u) << 5) | ((ux >> 3) & 31u)];
    const uint32_t dot = __builtin_amdgcn_udot4(quad, w, 0u, false);   // <= 65025
    const uint32_t b = (dot + 127u) / 255u;                            // rule 1: the grey level mvs_warp_by_depth returns
    return ok ? make_uint4(a | (b << 16), umul24u(a, b) | (1u << 24), aa, umul24u(b, b)) : make_uint4(0u, 0u, 0u, 0u);
}

// band.hip's sample (sweep_fx.hip: sample_global_fx) -> the absolute difference's window element e | ok << 24; a position outside the main
// frame carries NaN in its affine part (zncc_sample)
__device__ __forceinline__ uint32_t absdiff_sample(const Affine &A, float bx, float by, float bw, float z, const uint32_t *__restrict__ quads, uint32_t pitch, float hix,
                                                   float hiy, const uint32_t *__restrict__ lut, uint32_t Im255)
{
    const float sx = __builtin_fmaf(z, bx, A.ax), sy = __builtin_fmaf(z, by, A.ay), sw = __builtin_fmaf(z, bw, A.aw);
    const float r256 = rcp_rn(sw) * 256.0f;
    const float tx = __builtin_fmaf(sx, r256, ZN_MAGIC + 4.0f), ty = __builtin_fmaf(sy, r256, ZN_MAGIC + 4.0f);
    const bool ok = sw > 0.0f && tx > ZN_MAGIC + 132.0f && tx < hix && ty > ZN_MAGIC + 132.0f && ty < hiy;  // false for NaN
    const uint32_t ux = __builtin_bit_cast(uint32_t, tx) & 0x3fffffu, uy = __builtin_bit_cast(uint32_t, ty) & 0x3fffffu;  // t - magic
    const uint32_t quad = quads[ok ? (uy >> 8) * pitch + (ux >> 8) : 0u];   // in frame: column <= W, row <= H of the (H + 2) x pitch quad image
    const uint32_t w = lut[(((uy >> 3) & 31u) << 5) | ((ux >> 3) & 31u)];
    // (the builtin, not inline asm: sweep_fx.hip, sad_u16)
    const uint32_t cell = __builtin_amdgcn_sad_u16(__builtin_amdgcn_udot4(quad, w, 0u, false), Im255, 1u << 24);
    return ok ? cell : 0u;
}

// rules 3-5: the window's sums -> the view's contribution to the cell
__device__ __forceinline__ uint32_t zncc_cell(uint4 s, uint32_t centre_ok)
{
    const int N = (int)(s.y >> 24), Sab = (int)(s.y & 0xffffffu), Sa = (int)(s.x & 0xffffu), Sb = (int)(s.x >> 16), Saa = (int)s.z, Sbb = (int)s.w;
    const int cov = N * Sab - Sa * Sb, va = N * Saa - Sa * Sa, vb = N * Sbb - Sb * Sb;   // all below 2^31 (81 * 81 * 65025)
    const bool counted = centre_ok != 0u && va > 0 && vb > 0;
    const float den = sqrtf((float)max(va, 1) * (float)max(vb, 1));   // (the max: no 0 / 0 in a lane that is dropped anyway)
    float ncc = (float)cov / den;
    ncc = fminf(fmaxf(ncc, -1.0f), 1.0f);
    const uint32_t c = (uint32_t)floorf(32512.0f * (1.0f - ncc));     // 0 .. 65024
    return counted ? (1u << 24) + c : 0u;
}

// wave-uniform value -> SGPR
__device__ __forceinline__ float uniform_f(float x)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, x)));
}

// Workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 shares an XCD, MI355X_MICROARCH.md), each with
// its own 4 MiB L2.  Tiles are grouped 2 wide x 4 tall (128 x 64 pixels); the 8 tiles of a group get block ids
// with equal (id % 8), so a group's overlapping side-image regions share one L2, and consecutive groups go to
// consecutive XCDs, so border tiles (which take the slower per-sample-test path) spread evenly over the chip
// (a contiguous band per XCD cut HBM fetches 3.2x but ran 5 % slower: profiles/r01).  Bijective onto the padded
// group grid; ids that fall outside the image exit.  Placement affects speed and traffic only.
constexpr int GROUP_W = 2, GROUP_H = 4;

__device__ __forceinline__ int grouped_tile(int bid, int tiles_x, int tiles_y)
{
    const int gx = (tiles_x + GROUP_W - 1) / GROUP_W;
    const int sb = bid >> 6, x = bid & 7, m = (bid >> 3) & 7;
    const int g = sb * 8 + x;
    const int tx = (g % gx) * GROUP_W + (m & (GROUP_W - 1));
    const int ty = (g / gx) * GROUP_H + (m >> 1);
    return (tx < tiles_x && ty < tiles_y) ? ty * tiles_x + tx : -1;
}

// the main view: the context's own copy, or a slot of the frame store (mvs_sweep_handles)
inline const uint8_t *main_image_ptr(const mvs_ctx *ctx)
{
    return ctx->main_store_slot >= 0 ? (const uint8_t *)ctx->store_raw.ptr + (size_t)ctx->W * ctx->H * (size_t)ctx->main_store_slot : (const uint8_t *)ctx->main_img.ptr;
}

// host: launch parameters of the whole image / all planes; callers narrow the ranges
inline int fill_params(mvs_ctx *ctx, SweepParams &p, int v0, int vcount, int tile_h, int pc)
{
    p.main_img = main_image_ptr(ctx);
    p.pads = ctx->pads_valid ? (const uint8_t *)ctx->side_pads.ptr : nullptr;  // rebuilt on demand (ensure_pads) by the paths that gather single texels
    p.pad_slab = ctx->pad_slab;
    p.quads = ctx->views_in_store ? (const uint32_t *)ctx->store_quads.ptr : (const uint32_t *)ctx->side_quads.ptr;
    p.quads16 = (const uint2 *)ctx->side_quads16.ptr;
    p.pitch = ctx->pad_pitch;
    p.W = ctx->W;
    p.H = ctx->H;
    p.D = ctx->D;
    p.V = ctx->V;
    p.v0 = v0;
    p.vcount = vcount;
    p.Q = (const float *)ctx->qmats.ptr;
    p.z = (const float *)ctx->ztab.ptr;
    p.volume = ctx->volume;
    p.depth = (float *)ctx->depth.ptr;
    p.cost = (float *)ctx->cost.ptr;
    p.index = (int *)ctx->index.ptr;
    p.invW = 1.0f / (float)ctx->W;
    p.invH = 1.0f / (float)ctx->H;
    p.Wp = (float)ctx->W + 0.5f;
    p.Hp = (float)ctx->H + 0.5f;
    p.plan = (const uint2 *)ctx->plan.ptr;
    p.tiles_x = div_up(ctx->W, TILE_W);
    p.tile_h = tile_h;
    p.pc = pc;
    p.tiles_y = div_up(ctx->H, tile_h);
    p.nchunks = div_up(ctx->D, pc);
    p.chunk0 = 0;
    p.chunk1 = p.nchunks;
    p.ty0 = 0;
    p.tyn = p.tiles_y;
    p.row_begin = 0;
    p.row_end = ctx->H;
    p.plane_begin = 0;
    p.plane_end = ctx->D;
    p.cps = p.nchunks;
    p.part = nullptr;
    p.plan_stats = nullptr;
    p.view_slot = ctx->views_in_store ? (const int *)ctx->view_slots.ptr : nullptr;  // mvs_sweep_handles: view v is slot view_slot[v] of the frame store
    p.sep_r = nullptr;
    p.sep_y = nullptr;
    p.sep_dpad = 0;
    p.sep_reserved = 0;
    p.debug = 0;
    return MVS_OK;
}

// host: the depth / cost / index maps every writer of a selection needs
inline int ensure_maps(mvs_ctx *ctx)
{
    const size_t P = (size_t)ctx->W * ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->depth, P * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->cost, P * sizeof(float)))) return rc;
    return ensure(ctx, ctx->index, P * sizeof(int));
}

// host: the maps and, for a volume run, the packed volume of the current planes; a caller's volume that is too small is refused before
// anything is allocated
inline int sweep_outputs(mvs_ctx *ctx, bool need_volume, const char *who)
{
    const size_t need = volume_need(ctx);
    int rc;
    if (need_volume && ctx->volume_external && ctx->volume_bytes < need)
        return fail(ctx, MVS_EINVAL, "%s: caller volume is %zu bytes, need %zu", who, ctx->volume_bytes, need);
    if ((rc = ensure_maps(ctx))) return rc;
    if (need_volume && !ctx->volume_external) {
        if ((rc = ensure(ctx, ctx->volume_own, need))) return rc;
        ctx->volume = (uint32_t *)ctx->volume_own.ptr;
        ctx->volume_bytes = ctx->volume_own.bytes;
    }
    return MVS_OK;
}

// host: the fixed sampler's limits as every stage that samples with it (`who`) refuses them: the view range, the views a cell counts, the
// image size its addresses reach
inline int fx_sampler_limits(mvs_ctx *ctx, const char *who, int view_first, int view_count)
{
    if (view_first < 0 || view_count < 0 || view_first + view_count > ctx->V)
        return fail(ctx, MVS_EINVAL, "%s: view range [%d,%d) outside 0..%d", who, view_first, view_first + view_count, ctx->V);
    if (ctx->V > 255) return fail(ctx, MVS_EINVAL, "%s: the fixed sampler's cells hold at most 255 views (have %d)", who, ctx->V);
    if (ctx->W > 16383 || ctx->H > 16383) return fail(ctx, MVS_EINVAL, "%s: the fixed sampler addresses images of up to 16383 x 16383", who);
    return MVS_OK;
}

// host: what the fixed-sampler sweep entries (`who`) check alike before they touch anything: the flag bits, the inputs, the sampler and
// its limits.  Decodes the two output flags.
inline int fx_sweep_preconditions(mvs_ctx *ctx, const char *who, int view_first, int view_count, unsigned flags, bool &vol, bool &fused)
{
    if (flags & ~(MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN))
        return fail(ctx, MVS_EINVAL, "%s: unknown flag bits 0x%x (MVS_SWEEP_VOLUME and MVS_SWEEP_FUSED_ARGMIN only)", who,
                    flags & ~(MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN));
    vol = (flags & MVS_SWEEP_VOLUME) != 0;
    fused = (flags & MVS_SWEEP_FUSED_ARGMIN) != 0;
    if (!vol && !fused) return fail(ctx, MVS_EINVAL, "%s: flags select neither volume nor fused argmin", who);
    if (!ctx->have_main || !ctx->have_views || !ctx->have_planes) return fail(ctx, MVS_ESTATE, "%s: set main view, side views and planes first", who);
    if (ctx->sampler != MVS_SAMPLER_FIXED) return fail(ctx, MVS_ESTATE, "%s: implemented for MVS_SAMPLER_FIXED (the library default)", who);
    return fx_sampler_limits(ctx, who, view_first, view_count);
}

// host: narrows filled parameters to planes [plane_first, +plane_count) and rows [row_first, +row_count), in the units of the shape
// they were filled for (p.pc planes per chunk, tiles of p.tile_h rows) and in planes / pixels
inline void narrow_params(SweepParams &p, int plane_first, int plane_count, int row_first, int row_count)
{
    p.chunk0 = plane_first / p.pc;
    p.chunk1 = div_up(plane_first + plane_count, p.pc);
    p.ty0 = row_first / p.tile_h;
    p.tyn = div_up(row_first + row_count, p.tile_h) - p.ty0;
    p.row_begin = row_first;
    p.row_end = min(p.H, row_first + row_count);
    p.plane_begin = plane_first;
    p.plane_end = min(p.D, plane_first + plane_count);
}

// host: plane splits of a launch = gridDim.y
inline int split_count(const SweepParams &p) { return div_up(p.chunk1 - p.chunk0, p.cps); }

// host: the plane split of a tiled launch whose ranges are set.  A launch with too few tiles to fill the chip hands each workgroup
// p.cps of a tile's plane chunks (blockIdx.y selects them), aiming at `wgs_per_cu` workgroups per CU unless an experiment forces the
// split count; `max_cps` bounds what one workgroup can take.  With a fused depth selection the splits' partial bests go to p.part,
// for merge_split_bests.
inline int choose_split(mvs_ctx *ctx, SweepParams &p, int tiles, int wgs_per_cu, const SweepFlags &f, int max_cps = INT_MAX)
{
    const int nch = p.chunk1 - p.chunk0;
    const int want = f.forced_split ? f.forced_split : div_up(wgs_per_cu * ctx->num_cus, tiles);
    p.cps = max(1, min(div_up(nch, max(1, min(want, nch))), max_cps));
    if (f.fused && split_count(p) > 1) {
        int rc = ensure(ctx, ctx->best_parts, (size_t)split_count(p) * p.W * p.H * sizeof(uint2));
        if (rc) return rc;
        p.part = (uint2 *)ctx->best_parts.ptr;
    }
    return MVS_OK;
}

// host: calls f(std::bool_constant<VOL>, std::bool_constant<FUSED>) for the outputs a launch writes, so that a launcher names its kernel
// once.  Neither output is rejected by sweep_run_impl and is never instantiated.
template <class F>
inline auto with_outputs(bool vol, bool fused, F &&f)
{
    if (vol && fused) return f(std::true_type{}, std::true_type{});
    if (vol) return f(std::true_type{}, std::false_type{});
    return f(std::false_type{}, std::true_type{});
}

// host: calls f(std::integral_constant<int, CS>) for the cell layout of the context's sampler, so that a launch names its kernel once
template <class F>
inline auto with_cells(const mvs_ctx *ctx, F &&f)
{
    if (ctx->sampler == MVS_SAMPLER_FIXED) return f(std::integral_constant<int, CS_FIXED>{});
    return f(std::integral_constant<int, CS_EXACT>{});
}

int ensure_fx_lut(mvs_ctx *ctx);  // sweep_fx.hip: the fixed sampler's 32 x 32 weight table on the device (ctx->fx_lut)

// One call of a fixed-sampler sweep entry (the ZNCC, best-K, band, band best-K and gated sweeps) whose own arguments are checked
struct FxSweepCall {
    const char *who;
    int view_first, view_count;
    unsigned flags;
    const void *prior_dev;  // non-null: a band run, plane d of pixel p is prior(p) + the plane table's delta_d
    int tile_h, pc;         // the kernel's tile height and planes per chunk (fill_params)
};

// host: the body of those entries, what tests/shadow_context.py states as _fx_sweep: refusals, then allocations, then the band's copy of
// the prior, then launch(p, lut, prior, vol, fused) -- `prior` the context's copy, null without a band --, then the state (note_fx_sweep)
template <class F>
inline int fx_sweep_run(mvs_ctx *ctx, const FxSweepCall &c, F &&launch)
{
    const bool band = c.prior_dev != nullptr;
    bool vol, fused;
    int rc;
    if ((rc = fx_sweep_preconditions(ctx, c.who, c.view_first, c.view_count, c.flags, vol, fused))) return rc;
    for (int d = 0; band && d < ctx->D; d++)
        if (!(ctx->z_host[d] > -1.0f && ctx->z_host[d] < 1.0f))
            return fail(ctx, MVS_ESTATE, "%s: the plane table holds the band's offsets and must lie inside (-1, 1): offset %d is %g", c.who, d, ctx->z_host[d]);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    if ((rc = sweep_outputs(ctx, vol, c.who))) return rc;
    if (band && (rc = ensure(ctx, ctx->band_prior, P * sizeof(float)))) return rc;
    if ((rc = ensure_fx_lut(ctx))) return rc;
    // the context's own copy: the caller's map may be the depth map this run overwrites (stream order puts the copy first)
    if (band && c.prior_dev != ctx->band_prior.ptr)
        MVS_HIP(ctx, hipMemcpyAsync(ctx->band_prior.ptr, c.prior_dev, P * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    SweepParams p;
    fill_params(ctx, p, c.view_first, c.view_count, c.tile_h, c.pc);
    {
        ProfileScope ps(ctx, MVS_K_SWEEP);
        launch(p, (const uint32_t *)ctx->fx_lut.ptr, band ? (const float *)ctx->band_prior.ptr : nullptr, vol, fused);
    }
    MVS_HIP(ctx, hipGetLastError());
    note_fx_sweep(ctx, band, vol, fused);
    return MVS_OK;
}

// the launchers: `p` carries the view / plane / row ranges; each chooses its plane split; the caller merges the partial bests
// (merge_split_bests)
int sweep_fx_plan_general(mvs_ctx *ctx);                                    // sweep_fx.hip: the fixed-point sampler (contract v2)
int sweep_fx_launch(mvs_ctx *ctx, SweepParams &p, const SweepFlags &f);
int sweep_rect_launch(mvs_ctx *ctx, SweepParams &p, const SweepFlags &f);   // sweep_rect.hip: the fixed sampler on rectified views
int sweep_xrect_plan(mvs_ctx *ctx);                                         // sweep_xrect.hip: the exact sampler on rectified views
int sweep_xrect_launch(mvs_ctx *ctx, SweepParams &p, const SweepFlags &f);
int warp_by_depth_fx_launch(mvs_ctx *ctx, const float *depth_dev, const float *q_dev, const uint8_t *pad_dev, int pitch, uint8_t *out2_dev);
// select.hip: the merge of the partial bests choose_split's splits left in p.part, over the launch's rows; n packed cells as mean costs
int merge_split_bests(mvs_ctx *ctx, const SweepParams &p);
int unpack_volume_launch(mvs_ctx *ctx, const uint32_t *vol, float *out, size_t n);


// Planner counters: every thread of a launch used to hit the same two or three addresses with an atomic (0.2-0.3 ms of serialised L2
// atomics for a 0.01 ms kernel); one atomic per wavefront instead.  All 64 lanes must call (inactive contributions: the identity).
__device__ __forceinline__ int wave_max_i32(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, 64));
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

}  // namespace mvs
