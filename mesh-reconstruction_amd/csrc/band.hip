// band.hip -- band sweep: the fixed sampler's planes in a per-pixel band around a depth prior (DESIGN.md section 19 is the arithmetic
// contract; tests/band_mirror.py states it a sample at a time).
//
// Plane d of pixel p is  z = prior(p) + delta_d  with delta the context's plane table, so the D planes of a sweep are spent where a
// coarser result says the surface is instead of on the whole depth range.  The volume is the packed volume of the ordinary sweep (cells
// count << 24 | sum, [D][H][W]) and the maps are the ordinary maps, so everything behind the volume -- argmin, refinement, window,
// aggregation, cleaning -- runs on it unchanged, in the index domain.  The depth map holds OFFSETS delta[index] until mvs_sweep_band_resolve
// adds the prior back into a map of its own.
//
// sweep_fx_band: the un-tiled kernel's arithmetic (sweep_fx.hip: sample_global_fx) with a per-pixel z.  A workgroup is a 32 x 8-pixel tile,
// one pixel per thread; a wavefront covers 2 rows x 32 columns, so a plane's volume store is two full 128-byte segments.  The 4 KiB weight
// table sits in LDS (the kernel's only LDS); the texel quad is ONE dword of the view's quad image, read without a branch: a sample that is
// out of frame or on a dead plane reads quad 0 and is dropped by a select.  A dead plane (no prior, or prior + delta outside (-1, 1))
// carries z = NaN, which fails the sampler's own s.w > 0 test, so it costs no mask register.  The sample is absdiff_sample
// (sweep_shared.hpp), the one the windowed sweeps take: its e | ok << 24 is this sweep's cell of one view.
#include "sweep_shared.hpp"

#include <climits>

namespace mvs {

namespace {

constexpr int BAND_TW = 32, BAND_TH = 8;   // pixels per tile: 256 threads
constexpr int BAND_PC = 16;                // planes per accumulator chunk

// one chunk of up to BAND_PC planes from d0: the cells of the listed views into acc.  TAIL: the chunk has n < BAND_PC planes
template <bool TAIL>
__device__ __forceinline__ void band_chunk(const SweepParams &p, const uint32_t *__restrict__ lut, float xn, float yn, float z0, bool has, uint32_t Im255, float hix, float hiy,
                                           int d0, int n, uint32_t (&acc)[BAND_PC])
{
    float zc[BAND_PC];
#pragma unroll
    for (int k = 0; k < BAND_PC; k++) {
        acc[k] = 0u;
        const float z = z0 + p.z[TAIL ? min(d0 + k, p.D - 1) : d0 + k];   // one add (rule 2)
        zc[k] = (has && z > -1.0f && z < 1.0f) ? z : __builtin_nanf("");
    }
    for (int v = p.v0; v < p.v0 + p.vcount; v++) {
        const float *q = p.Q + 12 * v;
        const Affine A = view_affine(q, xn, yn);
        const uint32_t *qv = p.quads + p.pad_slab * (size_t)(p.view_slot ? p.view_slot[v] : v);
#pragma unroll
        for (int k = 0; k < BAND_PC; k++)
            if (!TAIL || k < n) acc[k] += absdiff_sample(A, q[2], q[6], q[10], zc[k], qv, (uint32_t)p.pitch, hix, hiy, lut, Im255);
    }
}

template <bool WRITE_VOLUME, bool FUSED>
__global__ __launch_bounds__(256) void sweep_fx_band(SweepParams p, const uint32_t *__restrict__ lut_g, const float *__restrict__ prior)
{
    __shared__ uint32_t lut[1024];
#pragma unroll
    for (int i = 0; i < 4; i++) lut[threadIdx.x + 256 * i] = lut_g[threadIdx.x + 256 * i];
    __syncthreads();
    const int col = blockIdx.x * BAND_TW + (threadIdx.x & (BAND_TW - 1));
    const int row = blockIdx.y * BAND_TH + (threadIdx.x / BAND_TW);
    if (col >= p.W || row >= p.H) return;   // (no barrier below)
    const size_t P = (size_t)p.W * p.H;
    const size_t pix = (size_t)row * p.W + col;
    const float xn = __builtin_fmaf((float)(2 * col + 1), p.invW, -1.0f);
    const float yn = __builtin_fmaf(-(float)(2 * row + 1), p.invH, 1.0f);
    const uint32_t Im255 = 255u * p.main_img[pix];
    const float hix = ZN_MAGIC + 132.0f + 256.0f * (float)p.W, hiy = ZN_MAGIC + 132.0f + 256.0f * (float)p.H;
    const float z0 = prior[pix];
    const bool has = z0 > -1.0f && z0 < 1.0f;   // rule 1 (false for NaN)
    uint32_t best = 0;
    int bi = -1;
    for (int d0 = 0; d0 < p.D; d0 += BAND_PC) {
        const int n = min(BAND_PC, p.D - d0);
        uint32_t acc[BAND_PC];
        if (n == BAND_PC)
            band_chunk<false>(p, lut, xn, yn, z0, has, Im255, hix, hiy, d0, n, acc);
        else
            band_chunk<true>(p, lut, xn, yn, z0, has, Im255, hix, hiy, d0, n, acc);
#pragma unroll
        for (int k = 0; k < BAND_PC; k++)
            if (k < n) {
                if (WRITE_VOLUME) __builtin_nontemporal_store(acc[k], p.volume + (size_t)(d0 + k) * P + pix);  // written once, read by a later kernel
                if (FUSED) argmin_update_packed<CS_FIXED>(acc[k], d0 + k, best, bi);
            }
    }
    if (FUSED) store_best<CS_FIXED>(p, pix, best & 0xffffffu, best >> 24, bi);   // depth = delta[index]: an offset
}

// rule 5: band_depth = prior + offset where there is an index and the sum stays inside (-1, 1), else the background depth; the report's
// four counters, one atomic per wavefront and counter
__global__ __launch_bounds__(256) void band_resolve(const float *__restrict__ prior, const float *__restrict__ offset, const int *__restrict__ index,
                                                    float *__restrict__ out, int *__restrict__ counters, size_t P, int D)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    int with_prior = 0, with_index = 0, at_edge = 0, emptied = 0;
    if (i < P) {
        const float z0 = prior[i];
        const int ix = index[i];
        with_prior = (z0 > -1.0f && z0 < 1.0f) ? 1 : 0;
        float r = MVS_BACKGROUND_DEPTH;
        if (ix >= 0) {
            with_index = 1;
            at_edge = (ix == 0 || ix == D - 1) ? 1 : 0;
            const float z = z0 + offset[i];
            if (z > -1.0f && z < 1.0f)
                r = z;
            else
                emptied = 1;
        }
        out[i] = r;
    }
    const int sums[4] = {wave_sum_i32(with_prior), wave_sum_i32(with_index), wave_sum_i32(at_edge), wave_sum_i32(emptied)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (sums[k]) atomicAdd(counters + k, sums[k]);
    }
}

// resolve, fetch and report work on the maps of a band run: one happened, no ordinary sweep since, and the index map is a selection over
// the planes the band run had
int band_state(mvs_ctx *ctx, const char *who)
{
    if (!ctx->band_planes) return fail(ctx, MVS_ESTATE, "%s: no band run yet, or an ordinary sweep or a new prior (mvs_pyramid_prior) since (mvs_sweep_run_band first)", who);
    if (!ctx->have_planes || ctx->D != ctx->band_planes)
        return fail(ctx, MVS_ESTATE, "%s: the band run had %d planes, the context now has %d (run the band again)", who, ctx->band_planes, ctx->D);
    if (!selection_current(ctx) || !ctx->index.ptr)
        return fail(ctx, MVS_ESTATE, "%s: no depth selection over the current %d planes (MVS_SWEEP_FUSED_ARGMIN, or mvs_sweep_argmin)", who, ctx->D);
    return MVS_OK;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_run_band(mvs_ctx *ctx, int view_first, int view_count, const void *prior_dev, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_run_band: null context");
    if (!prior_dev) return fail(ctx, MVS_EINVAL, "mvs_sweep_run_band: prior_dev is null");
    return fx_sweep_run(ctx, {"mvs_sweep_run_band", view_first, view_count, flags, prior_dev, BAND_TH, BAND_PC},
                        [&](const SweepParams &p, const uint32_t *lut, const float *prior, bool vol, bool fused) {
                            const dim3 grid((unsigned)div_up(ctx->W, BAND_TW), (unsigned)div_up(ctx->H, BAND_TH));
                            with_outputs(vol, fused, [&](auto v, auto f) { sweep_fx_band<decltype(v)::value, decltype(f)::value><<<grid, 256, 0, ctx->stream>>>(p, lut, prior); });
                        });
}

int mvs_sweep_band_resolve(mvs_ctx *ctx)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_band_resolve: null context");
    int rc;
    if ((rc = band_state(ctx, "mvs_sweep_band_resolve"))) return rc;
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    if ((rc = ensure(ctx, ctx->band_depth, P * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->band_counters, 4 * sizeof(int)))) return rc;
    MVS_HIP(ctx, hipMemsetAsync(ctx->band_counters.ptr, 0, 4 * sizeof(int), ctx->stream));
    {
        ProfileScope ps(ctx, MVS_K_ARGMIN);
        band_resolve<<<(unsigned)((P + 255) / 256), 256, 0, ctx->stream>>>((const float *)ctx->band_prior.ptr, (const float *)ctx->depth.ptr, (const int *)ctx->index.ptr,
                                                                         (float *)ctx->band_depth.ptr, (int *)ctx->band_counters.ptr, P, ctx->D);
    }
    MVS_HIP(ctx, hipGetLastError());
    note_band_resolved(ctx);
    return MVS_OK;
}

void *mvs_sweep_band_depth_device(mvs_ctx *ctx) { return ctx ? ctx->band_depth.ptr : nullptr; }
void *mvs_sweep_band_prior_device(mvs_ctx *ctx) { return ctx ? ctx->band_prior.ptr : nullptr; }

int mvs_sweep_band_fetch(mvs_ctx *ctx, float *depth_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_band_fetch: null context");
    if (!depth_hw) return fail(ctx, MVS_EINVAL, "mvs_sweep_band_fetch: depth_hw is null");
    if (int rc = band_state(ctx, "mvs_sweep_band_fetch")) return rc;
    if (!ctx->band_resolved) return fail(ctx, MVS_ESTATE, "mvs_sweep_band_fetch: the last band run is not resolved (mvs_sweep_band_resolve first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(depth_hw, ctx->band_depth.ptr, (size_t)ctx->W * ctx->H * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_sweep_band_report(mvs_ctx *ctx, int out[4])
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_band_report: null context");
    if (!out) return fail(ctx, MVS_EINVAL, "mvs_sweep_band_report: out is null");
    if (int rc = band_state(ctx, "mvs_sweep_band_report")) return rc;
    if (!ctx->band_resolved) return fail(ctx, MVS_ESTATE, "mvs_sweep_band_report: the last band run is not resolved (mvs_sweep_band_resolve first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(out, ctx->band_counters.ptr, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}
