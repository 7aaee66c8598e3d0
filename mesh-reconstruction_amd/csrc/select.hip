// select.hip -- depth selection over a packed cost volume, whichever sampler or stage wrote it: argmin_volume (also over the slice of
// planes a rank owns), combine_best (merge of partial selections), refine_depth and unpack_volume, with their entry points; the one place
// that decides which packed volume the readers read (reader_volume, mvs_sweep_set_volume_source); the row-band transition of the selection
// state (note_rows_selected).  The rules themselves are select_rules.hpp's device functions.
#include "sweep_shared.hpp"

namespace mvs {

template <int CS>
__global__ __launch_bounds__(256) void refine_depth(const uint32_t *__restrict__ vol, size_t P, int D, const float *__restrict__ z, const int *__restrict__ index,
                                                    float *__restrict__ depth)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    const int i = index[p];
    if (i < 0) {
        depth[p] = MVS_BACKGROUND_DEPTH;
        return;
    }
    float zr = z[i];
    if (i > 0 && i < D - 1) {
        const uint32_t a = vol[(size_t)(i - 1) * P + p], b = vol[(size_t)i * P + p], c = vol[(size_t)(i + 1) * P + p];
        if ((a >> CS) != 0u && (c >> CS) != 0u && (b >> CS) != 0u) zr = refine_parabola(cell_mean<CS>(a), cell_mean<CS>(b), cell_mean<CS>(c), z, i, D);
    }
    depth[p] = zr;
}

// merge of the partial bests of a plane-split launch: splits are in ascending plane order and a later split wins only
// if strictly better, so ties still go to the lowest plane
template <int CS>
__global__ __launch_bounds__(256) void combine_best(SweepParams p, int nsplit, size_t pix_first, size_t pix_count)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= pix_count) return;
    const size_t pix = pix_first + i, P = (size_t)p.W * p.H;
    uint32_t best = 0u;
    int bi = -1;
    for (int s = 0; s < nsplit; s++) {
        const uint2 st = p.part[(size_t)s * P + pix];
        argmin_update_packed<CS>(st.x, (int)st.y, best, bi);
    }
    store_best<CS>(p, pix, best & ((1u << CS) - 1u), best >> CS, bi);
}

static int launch_combine(mvs_ctx *ctx, const SweepParams &p, int nsplit, size_t pix_first, size_t pix_count)
{
    with_cells(ctx, [&](auto cs) {
        combine_best<decltype(cs)::value><<<(unsigned)((pix_count + 255) / 256), 256, 0, ctx->stream>>>(p, nsplit, pix_first, pix_count);
    });
    MVS_HIP(ctx, hipGetLastError());
    return MVS_OK;
}

int merge_split_bests(mvs_ctx *ctx, const SweepParams &p)
{
    if (!p.part) return MVS_OK;
    return launch_combine(ctx, p, split_count(p), (size_t)p.row_begin * p.W, (size_t)(p.row_end - p.row_begin) * p.W);
}

// Layout [D][P] keeps a pixel on a lane, so the reduction over planes runs in registers; each thread
// streams 16-byte loads of 4 consecutive pixels per plane (P % 4 == 0) or single cells otherwise.
// part != nullptr: `vol` holds planes [d_first, d_first + D) only (the slice a rank owns after a reduce-scatter) and the result
// is the partial selection (best packed cell, best ABSOLUTE plane index) per pixel, to be merged by combine_best
template <int VEC, int CS>
__global__ __launch_bounds__(256) void argmin_volume(const uint32_t *__restrict__ vol, size_t P, int D,
                                                     const float *__restrict__ z, float *__restrict__ depth,
                                                     float *__restrict__ cost, int *__restrict__ index,
                                                     uint2 *__restrict__ part = nullptr, int d_first = 0)
{
    const size_t base = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * VEC;
    if (base >= P) return;
    uint32_t bs[VEC], bc[VEC];
    int bi[VEC];
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        bs[i] = 0u;
        bc[i] = 0u;
        bi[i] = -1;
    }
    int d = 0;
    constexpr int UNR = 8;  // planes in flight per thread: 8 x 16 B, non-temporal (the stream is read once): 4.75 -> 5.64 TB/s at c3
    for (; d + UNR <= D; d += UNR) {
        uint32_t c[UNR][VEC];
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            if (VEC == 4) {
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                const u32x4 t = __builtin_nontemporal_load((const u32x4 *)(vol + (size_t)(d + u) * P + base));
                c[u][0] = t.x;
                c[u][1 % VEC] = t.y;
                c[u][2 % VEC] = t.z;
                c[u][3 % VEC] = t.w;
            } else {
                c[u][0] = vol[(size_t)(d + u) * P + base];
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; u++)
#pragma unroll
            for (int i = 0; i < VEC; i++) argmin_update<CS>(c[u][i], d + u, bs[i], bc[i], bi[i]);
    }
    for (; d < D; d++) {
#pragma unroll
        for (int i = 0; i < VEC; i++) argmin_update<CS>(vol[(size_t)d * P + base + i], d, bs[i], bc[i], bi[i]);
    }
    if (part) {
#pragma unroll
        for (int i = 0; i < VEC; i++)
            part[base + i] = bi[i] >= 0 ? make_uint2((bc[i] << CS) | bs[i], (uint32_t)(bi[i] + d_first)) : make_uint2(0u, 0xffffffffu);
        return;
    }
#pragma unroll
    for (int i = 0; i < VEC; i++) {
        depth[base + i] = bi[i] >= 0 ? z[bi[i]] : MVS_BACKGROUND_DEPTH;
        cost[base + i] = bi[i] >= 0 ? cell_cost<CS>(bs[i], bc[i]) : __builtin_inff();
        index[base + i] = bi[i];
    }
}

// depth selection over `vol` with the cell layout of the context's sampler; 16-byte loads when the pixel count and the pointer allow
static void launch_argmin(mvs_ctx *ctx, const uint32_t *vol, size_t P, int D, const float *z, float *depth, float *cost, int *index, uint2 *part,
                          int d_first)
{
    const bool wide = P % 4 == 0 && ((uintptr_t)vol % 16) == 0;
    const unsigned blocks = (unsigned)(((wide ? P / 4 : P) + 255) / 256);
    with_cells(ctx, [&](auto cs) {
        constexpr int CS = decltype(cs)::value;
        if (wide)
            argmin_volume<4, CS><<<blocks, 256, 0, ctx->stream>>>(vol, P, D, z, depth, cost, index, part, d_first);
        else
            argmin_volume<1, CS><<<blocks, 256, 0, ctx->stream>>>(vol, P, D, z, depth, cost, index, part, d_first);
    });
}

template <int CS>
__global__ void unpack_volume(const uint32_t *__restrict__ vol, float *__restrict__ out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t cell = vol[i];
    const uint32_t s = cell & ((1u << CS) - 1u), c = cell >> CS;
    out[i] = c ? cell_cost<CS>(s, c) : __builtin_inff();
}

int unpack_volume_launch(mvs_ctx *ctx, const uint32_t *vol, float *out, size_t n)
{
    with_cells(ctx, [&](auto cs) { unpack_volume<decltype(cs)::value><<<(unsigned)((n + 255) / 256), 256, 0, ctx->stream>>>(vol, out, n); });
    MVS_HIP(ctx, hipGetLastError());
    return MVS_OK;
}

int cells_readable(mvs_ctx *ctx, const char *who, const char *what, int cells_sampler)
{
    static const char *const names[2] = {"MVS_SAMPLER_FIXED", "MVS_SAMPLER_EXACT_F32"};
    if (cells_sampler == mvs_ctx::CELLS_MIXED)
        return fail(ctx, MVS_ESTATE, "%s: %s holds cells of both samplers' layouts (a row band or plane group swept after a sampler switch): sweep all of it first", who,
                    what);
    if (cells_sampler < 0 || cells_sampler == ctx->sampler) return MVS_OK;
    return fail(ctx, MVS_ESTATE, "%s: %s was written under %s and the context's sampler now is %s, whose cells have another layout (sweep again, or switch back)", who,
                what, names[cells_sampler == MVS_SAMPLER_FIXED ? 0 : 1], names[ctx->sampler == MVS_SAMPLER_FIXED ? 0 : 1]);
}

int reader_volume(mvs_ctx *ctx, const char *who, const uint32_t *&vol, size_t &bytes)
{
    vol = nullptr;
    bytes = 0;
    if (ctx->volume_source != MVS_VOLUME_WINDOWED) {
        if (int rc = cells_readable(ctx, who, "the packed volume", ctx->vol_cells_sampler)) return rc;
        vol = ctx->volume;
        bytes = ctx->volume_bytes;
        return MVS_OK;
    }
    if (!ctx->have_planes || !ctx->win_planes || ctx->win_planes != ctx->D)
        return fail(ctx, MVS_ESTATE, "%s: the volume source is MVS_VOLUME_WINDOWED and there is no windowed volume of the current %d planes (mvs_sweep_window first)", who,
                    ctx->D);
    if (int rc = cells_readable(ctx, who, "the windowed volume", ctx->win_cells_sampler)) return rc;
    vol = (const uint32_t *)ctx->win_vol.ptr;
    bytes = (size_t)ctx->win_planes * ctx->W * ctx->H * sizeof(uint32_t);
    return MVS_OK;
}

// The whole image, or bands over the plane count the map already has, leave a selection over D planes; bands over another count leave
// one only once they -- each overlapping or touching what the earlier ones covered -- reach every row: until then the other rows hold
// planes of the old count and there is no selection
void note_rows_selected(mvs_ctx *ctx, int r0, int r1)
{
    const int D = ctx->D;
    if (r0 <= 0 && r1 >= ctx->H) return note_full_selection(ctx);
    if (ctx->sel_planes == D) return;
    ctx->sel_planes = 0;  // rows of two plane counts: no selection until the bands are through
    if (ctx->sel_band_planes != D || r0 > ctx->sel_band_hi || r1 < ctx->sel_band_lo) {
        ctx->sel_band_planes = D;
        ctx->sel_band_lo = r0;
        ctx->sel_band_hi = r1;
    } else {
        ctx->sel_band_lo = r0 < ctx->sel_band_lo ? r0 : ctx->sel_band_lo;
        ctx->sel_band_hi = r1 > ctx->sel_band_hi ? r1 : ctx->sel_band_hi;
    }
    if (ctx->sel_band_lo <= 0 && ctx->sel_band_hi >= ctx->H) note_full_selection(ctx);
}

}  // namespace mvs

using namespace mvs;

int mvs_sweep_argmin(mvs_ctx *ctx)
{
    if (!ctx) return MVS_EINVAL;
    const uint32_t *vol;
    size_t vol_bytes;
    int rc = reader_volume(ctx, "mvs_sweep_argmin", vol, vol_bytes);   // refuses before anything is allocated
    if (rc) return rc;
    const bool raw = ctx->volume_source == MVS_VOLUME_RAW;
    if (raw && (!ctx->have_planes || !ctx->volume))
        return fail(ctx, MVS_ESTATE, "mvs_sweep_argmin: no cost volume (run mvs_sweep_run with MVS_SWEEP_VOLUME)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = sweep_outputs(ctx, raw, "mvs_sweep_argmin"))) return rc;
    if (raw) vol = ctx->volume;   // (sweep_outputs may have re-made the context's own)
    const size_t P = (size_t)ctx->W * ctx->H;
    ProfileScope ps(ctx, MVS_K_ARGMIN);
    launch_argmin(ctx, vol, P, ctx->D, (const float *)ctx->ztab.ptr, (float *)ctx->depth.ptr, (float *)ctx->cost.ptr, (int *)ctx->index.ptr,
                  nullptr, 0);
    MVS_HIP(ctx, hipGetLastError());
    note_full_selection(ctx);
    return MVS_OK;
}

int mvs_sweep_refine_depth(mvs_ctx *ctx)
{
    if (!ctx) return MVS_EINVAL;
    const uint32_t *vol;
    size_t vol_bytes;
    if (int rc = reader_volume(ctx, "mvs_sweep_refine_depth", vol, vol_bytes)) return rc;
    if (!ctx->have_planes || !vol || !ctx->index.ptr || !ctx->sel_planes)
        return fail(ctx, MVS_ESTATE, "mvs_sweep_refine_depth: needs the packed volume and a depth selection (MVS_SWEEP_VOLUME | MVS_SWEEP_FUSED_ARGMIN, or mvs_sweep_argmin)");
    // the kernel reads z[index] and the cells of planes index - 1 .. index + 1: the index map must be one over the current planes ...
    if (!selection_current(ctx))
        return fail(ctx, MVS_ESTATE, "mvs_sweep_refine_depth: the depth selection was made over %d planes, the context now has %d (select again)", ctx->sel_planes, ctx->D);
    // ... and the volume must hold them
    const size_t P = (size_t)ctx->W * ctx->H, need = volume_need(ctx);
    if (vol_bytes < need) {
        if (ctx->volume_external) return fail(ctx, MVS_EINVAL, "mvs_sweep_refine_depth: caller volume is %zu bytes, %d planes need %zu", vol_bytes, ctx->D, need);
        return fail(ctx, MVS_ESTATE, "mvs_sweep_refine_depth: the context's volume is %zu bytes, %d planes need %zu (mvs_sweep_run with MVS_SWEEP_VOLUME)", vol_bytes, ctx->D, need);
    }
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    with_cells(ctx, [&](auto cs) {
        refine_depth<decltype(cs)::value><<<(unsigned)((P + 255) / 256), 256, 0, ctx->stream>>>(vol, P, ctx->D, (const float *)ctx->ztab.ptr, (const int *)ctx->index.ptr,
                                                                                            (float *)ctx->depth.ptr);
    });
    MVS_HIP(ctx, hipGetLastError());
    return MVS_OK;
}

int mvs_sweep_argmin_partial(mvs_ctx *ctx, const void *volume_slice_dev, int plane_first, int plane_count, void *partial_out_dev)
{
    if (!ctx || !volume_slice_dev || !partial_out_dev) return fail(ctx, MVS_EINVAL, "mvs_sweep_argmin_partial: null argument");
    if (!ctx->have_planes) return fail(ctx, MVS_ESTATE, "mvs_sweep_argmin_partial: set the planes first");
    if (plane_first < 0 || plane_count <= 0 || plane_first + plane_count > ctx->D)
        return fail(ctx, MVS_EINVAL, "mvs_sweep_argmin_partial: planes [%d,%d) outside 0..%d", plane_first, plane_first + plane_count, ctx->D);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    ProfileScope ps(ctx, MVS_K_ARGMIN);
    launch_argmin(ctx, (const uint32_t *)volume_slice_dev, P, plane_count, nullptr, nullptr, nullptr, nullptr, (uint2 *)partial_out_dev, plane_first);
    MVS_HIP(ctx, hipGetLastError());
    return MVS_OK;
}

int mvs_sweep_combine_partials(mvs_ctx *ctx, const void *partials_dev, int nparts)
{
    if (!ctx || !partials_dev || nparts <= 0) return fail(ctx, MVS_EINVAL, "mvs_sweep_combine_partials: bad argument");
    if (!ctx->have_planes) return fail(ctx, MVS_ESTATE, "mvs_sweep_combine_partials: set the planes first");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    int rc = sweep_outputs(ctx, false, "mvs_sweep_combine_partials");
    if (rc) return rc;
    SweepParams p;
    fill_params(ctx, p, 0, 0, 16, 16);
    p.part = (uint2 *)partials_dev;  // read-only here
    ProfileScope ps(ctx, MVS_K_ARGMIN);
    if ((rc = launch_combine(ctx, p, nparts, 0, (size_t)ctx->W * ctx->H))) return rc;
    note_full_selection(ctx);
    return MVS_OK;
}

int mvs_sweep_set_volume_source(mvs_ctx *ctx, int source)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_set_volume_source: null context");
    if (source != MVS_VOLUME_RAW && source != MVS_VOLUME_WINDOWED) return fail(ctx, MVS_EINVAL, "mvs_sweep_set_volume_source: unknown source %d", source);
    ctx->volume_source = source;
    return MVS_OK;
}

int mvs_sweep_volume_source(const mvs_ctx *ctx) { return ctx ? ctx->volume_source : MVS_EINVAL; }
