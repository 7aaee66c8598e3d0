// depth_filter.hip -- depth-map filter: gated median and gated mean of a selected depth map (include/mvs.h "mvs_depth_filter", DESIGN.md
// section 23 holds the contract; tests/depth_filter_mirror.py restates it in numpy, bit for bit).
//
// The median stage does no arithmetic at all (its output is one of its inputs) and the mean stage adds its members one at a time in window
// order, one f32 rounding per operation, so nothing below depends on the order in which the hardware runs it.
//   depth_filter_median<R, GATED>   a workgroup of 256 threads owns a 32 x 8 pixel tile, a thread one pixel.  The tile plus an R-wide halo
//                        ((32 + 2R) x (8 + 2R) elements) is staged in LDS once: the depth as an order-preserving u32 key (sign bit flipped
//                        for z >= 0, all bits for z < 0, of z + 0.0f), 0xffffffff for a pixel that is invalid or outside the frame -- no
//                        valid key has that value, and it is above every valid key -- and, GATED, the guide byte beside it.  A thread
//                        gathers the (2R + 1)^2 keys of its window into registers, the ones the guide gate refuses replaced by 0xffffffff,
//                        and counts the n that are left.  The key of rank k = (n - 1) / 2 is the largest T with fewer than k + 1 keys below
//                        it; T is found a bit at a time from the top, 32 rounds of (2R + 1)^2 compare-and-count on registers: no sort, no
//                        indexed register array, no scratch.  The round loop is a real loop, its body the unrolled window.
//   depth_filter_mean<R, GATED>     the same tile and staging with the map's values themselves (z + 0.0f, NaN for a pixel that is invalid
//                        or outside the frame: NaN fails the depth gate's comparison, so it needs no flag).  A thread walks its window in
//                        row-major order: member = guide gate and fabsf(m(q) - m(p)) <= max_step, sum += m(q), n += 1, then sum / (float)n
//                        in correctly rounded f32 division.
// Not GATED (tau = 255): the guide is neither staged nor read.  With both stages the median writes the context's intermediate map and the
// mean reads it: two launches, the second over a map that is L2-resident at every size the sweep runs at.
// No atomics, no scalar memory writes.
#include "sweep_shared.hpp"

namespace mvs {

namespace {

constexpr int DF_TW = 32, DF_TH = 8, DF_THREADS = DF_TW * DF_TH;   // pixels per tile, one per thread
constexpr int DF_MAX_RADIUS = 4;
constexpr uint32_t DF_NONE = 0xffffffffu;   // the key of a pixel that is no member: above every valid key

struct FilterArgs {
    const float *__restrict__ src;
    float *__restrict__ dst;
    const uint8_t *__restrict__ guide;   // GATED only
    int W, H, tau, fill, min_members;
    float max_step;
};

__device__ __forceinline__ bool df_valid(float z) { return z > -1.0f && z < 1.0f; }   // rule 1 (false for NaN)

// valid z -> a key that orders as the floats do
__device__ __forceinline__ uint32_t df_key(float z)
{
    const uint32_t b = __builtin_bit_cast(uint32_t, z + 0.0f);   // -0.0 -> +0.0
    return df_valid(z) ? b ^ ((uint32_t)((int32_t)b >> 31) | 0x80000000u) : DF_NONE;
}

__device__ __forceinline__ float df_unkey(uint32_t k) { return __builtin_bit_cast(float, k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu)); }

template <int R, bool GATED>
__global__ __launch_bounds__(DF_THREADS) void depth_filter_median(const FilterArgs a)
{
    constexpr int K = 2 * R + 1, LW = DF_TW + 2 * R, LH = DF_TH + 2 * R, CELLS = LW * LH;
    __shared__ uint32_t keys[CELLS];
    __shared__ uint8_t gd[GATED ? CELLS : 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DF_TW, y0 = blockIdx.y * DF_TH;
    for (int e = tid; e < CELLS; e += DF_THREADS) {
        const int ly = e / LW, lx = e - ly * LW;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        const bool inside = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
        const size_t pix = inside ? (size_t)gy * a.W + gx : 0;
        keys[e] = inside ? df_key(a.src[pix]) : DF_NONE;
        if (GATED) gd[e] = inside ? a.guide[pix] : (uint8_t)0;   // (outside the frame: any value, the key there is DF_NONE)
    }
    __syncthreads();
    const int tx = tid & (DF_TW - 1), ty = tid / DF_TW;
    const int col = x0 + tx, row = y0 + ty;
    if (col >= a.W || row >= a.H) return;   // (no barrier below)
    uint32_t k[K * K];
    const uint32_t g0 = GATED ? (uint32_t)gd[(ty + R) * LW + tx + R] : 0u, tau = (uint32_t)a.tau;
    int n = 0;
#pragma unroll
    for (int dy = 0; dy < K; dy++)
#pragma unroll
        for (int dx = 0; dx < K; dx++) {
            const int e = (ty + dy) * LW + tx + dx;
            uint32_t key = keys[e];
            if (GATED) {
                const uint32_t g = gd[e], diff = max(g, g0) - min(g, g0);
                key |= (~(tau - diff) >> 31) - 1u;   // diff <= tau (both below 256): as it is, else DF_NONE
            }
            k[dy * K + dx] = key;
            n += key != DF_NONE ? 1 : 0;
        }
    const uint32_t own = k[R * K + R];
    const int rank = (n - 1) >> 1;   // the lower median; n = 0: -1, nothing is below it and the result is not used
    uint32_t T = 0u;
#pragma unroll 1
    for (int bit = 31; bit >= 0; bit--) {
        const uint32_t cand = T | (1u << bit);
        int below = 0;
#pragma unroll
        for (int j = 0; j < K * K; j++) below += k[j] < cand ? 1 : 0;
        T = below <= rank ? cand : T;
    }
    const bool take = own != DF_NONE || (a.fill && n >= a.min_members);   // min_members >= 1
    a.dst[(size_t)row * a.W + col] = take ? df_unkey(T) : MVS_BACKGROUND_DEPTH;
}

template <int R, bool GATED>
__global__ __launch_bounds__(DF_THREADS) void depth_filter_mean(const FilterArgs a)
{
    constexpr int K = 2 * R + 1, LW = DF_TW + 2 * R, LH = DF_TH + 2 * R, CELLS = LW * LH;
    __shared__ float vals[CELLS];
    __shared__ uint8_t gd[GATED ? CELLS : 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * DF_TW, y0 = blockIdx.y * DF_TH;
    for (int e = tid; e < CELLS; e += DF_THREADS) {
        const int ly = e / LW, lx = e - ly * LW;
        const int gx = x0 - R + lx, gy = y0 - R + ly;
        const bool inside = gx >= 0 && gx < a.W && gy >= 0 && gy < a.H;
        const size_t pix = inside ? (size_t)gy * a.W + gx : 0;
        const float z = a.src[pix];
        vals[e] = inside && df_valid(z) ? z + 0.0f : __builtin_nanf("");
        if (GATED) gd[e] = inside ? a.guide[pix] : (uint8_t)0;
    }
    __syncthreads();
    const int tx = tid & (DF_TW - 1), ty = tid / DF_TW;
    const int col = x0 + tx, row = y0 + ty;
    if (col >= a.W || row >= a.H) return;   // (no barrier below)
    const float c = vals[(ty + R) * LW + tx + R];
    const uint32_t g0 = GATED ? (uint32_t)gd[(ty + R) * LW + tx + R] : 0u, tau = (uint32_t)a.tau;
    float sum = 0.0f;
    int n = 0;
#pragma unroll
    for (int dy = 0; dy < K; dy++)
#pragma unroll
        for (int dx = 0; dx < K; dx++) {
            const int e = (ty + dy) * LW + tx + dx;
            float v = vals[e];
            if (GATED) {
                // a pixel the guide gate refuses becomes NaN, in integer arithmetic: one condition per neighbour, used at once (two of
                // them, combined, are kept in scalar registers for the whole window and spill those)
                const uint32_t g = gd[e], diff = max(g, g0) - min(g, g0);
                const uint32_t pass = ~(tau - diff) >> 31;   // diff <= tau, both below 256
                v = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | (pass - 1u));
            }
            const bool in = __builtin_fabsf(v - c) <= a.max_step;   // false for a NaN on either side
            sum += in ? v : 0.0f;   // (sum + 0.0f is sum: a sum that starts at +0.0f and adds no -0.0f never is -0.0f)
            n += in ? 1 : 0;
        }
    // a valid centre is a member of its own window: n >= 1
    a.dst[(size_t)row * a.W + col] = c == c ? sum / (float)n : MVS_BACKGROUND_DEPTH;
}

template <int R>
void launch_stage(mvs_ctx *ctx, bool mean, bool gated, const FilterArgs &a)
{
    const dim3 grid((unsigned)div_up(a.W, DF_TW), (unsigned)div_up(a.H, DF_TH));
    if (mean) {
        if (gated)
            depth_filter_mean<R, true><<<grid, DF_THREADS, 0, ctx->stream>>>(a);
        else
            depth_filter_mean<R, false><<<grid, DF_THREADS, 0, ctx->stream>>>(a);
    } else {
        if (gated)
            depth_filter_median<R, true><<<grid, DF_THREADS, 0, ctx->stream>>>(a);
        else
            depth_filter_median<R, false><<<grid, DF_THREADS, 0, ctx->stream>>>(a);
    }
}

void launch_stage(mvs_ctx *ctx, int radius, bool mean, bool gated, const FilterArgs &a)
{
    switch (radius) {
    case 1: launch_stage<1>(ctx, mean, gated, a); break;
    case 2: launch_stage<2>(ctx, mean, gated, a); break;
    case 3: launch_stage<3>(ctx, mean, gated, a); break;
    default: launch_stage<4>(ctx, mean, gated, a); break;
    }
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_depth_filter(mvs_ctx *ctx, const void *depth_dev, const void *guide_dev, int radius, int tau, float max_step, int min_members, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_filter: null context");
    if (!depth_dev) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: depth_dev is null");
    if (radius < 1 || radius > DF_MAX_RADIUS) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: radius %d outside 1..%d", radius, DF_MAX_RADIUS);
    if (tau < 0 || tau > 255) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: tau %d outside 0..255", tau);
    if (!(max_step >= 0.0f)) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: max_step %g is negative or NaN", (double)max_step);
    const unsigned known = MVS_FILTER_MEDIAN | MVS_FILTER_MEAN | MVS_FILTER_FILL;
    if (flags & ~known) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: unknown flag bits 0x%x", flags & ~known);
    const bool median = (flags & MVS_FILTER_MEDIAN) != 0, mean = (flags & MVS_FILTER_MEAN) != 0, fill = (flags & MVS_FILTER_FILL) != 0;
    if (!median && !mean) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: flags select neither MVS_FILTER_MEDIAN nor MVS_FILTER_MEAN");
    if (fill && !median) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: MVS_FILTER_FILL without MVS_FILTER_MEDIAN");
    if (fill && (min_members < 1 || min_members > 81)) return fail(ctx, MVS_EINVAL, "mvs_depth_filter: min_members %d outside 1..81", min_members);
    const bool gated = tau < 255;
    const uint8_t *guide = guide_dev ? (const uint8_t *)guide_dev : (ctx->have_main ? main_image_ptr(ctx) : nullptr);
    if (gated && !guide) return fail(ctx, MVS_ESTATE, "mvs_depth_filter: tau %d needs a guide image: pass one, or stage a main image (mvs_sweep_set_main)", tau);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->dfilter_maps, 2 * P * sizeof(float)))) return rc;   // the filtered map, then the intermediate map
    float *out = (float *)ctx->dfilter_maps.ptr, *mid = out + P;
    FilterArgs a;
    a.guide = gated ? guide : nullptr;
    a.W = ctx->W;
    a.H = ctx->H;
    a.tau = tau;
    a.fill = fill ? 1 : 0;
    a.min_members = fill ? min_members : 1;
    a.max_step = max_step;
    const bool in_place = depth_dev == (const void *)out;   // the filtered map of an earlier call, filtered again
    {
        ProfileScope ps(ctx, MVS_K_ARGMIN);
        if (median && mean) {
            // (an input that is the filtered map itself is read by the median only, which writes the intermediate map)
            a.src = (const float *)depth_dev;
            a.dst = mid;
            launch_stage(ctx, radius, false, gated, a);
            a.src = mid;
            a.dst = out;
            launch_stage(ctx, radius, true, gated, a);
        } else {
            a.src = (const float *)depth_dev;
            a.dst = in_place ? mid : out;   // a stage never reads the map it writes
            launch_stage(ctx, radius, mean, gated, a);
        }
    }
    MVS_HIP(ctx, hipGetLastError());
    if (in_place && !(median && mean)) MVS_HIP(ctx, hipMemcpyAsync(out, mid, P * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->dfilter_have = true;
    return MVS_OK;
}

void *mvs_depth_filtered_device(mvs_ctx *ctx) { return ctx && ctx->dfilter_have ? ctx->dfilter_maps.ptr : nullptr; }

int mvs_depth_filter_fetch(mvs_ctx *ctx, float *depth_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_filter_fetch: null context");
    if (!depth_hw) return fail(ctx, MVS_EINVAL, "mvs_depth_filter_fetch: depth_hw is null");
    if (!ctx->dfilter_have) return fail(ctx, MVS_ESTATE, "mvs_depth_filter_fetch: no filtered map yet (mvs_depth_filter first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(depth_hw, ctx->dfilter_maps.ptr, (size_t)ctx->W * ctx->H * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}
