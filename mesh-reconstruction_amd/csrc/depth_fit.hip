// depth_fit.hip -- depth-map plane fit: a gated least-squares plane through the window of every pixel of a depth map -> slopes, a fitted
// depth, normals, and slope seeds for the propagation (include/mvs.h "mvs_depth_fit", DESIGN.md section 32 holds the contract;
// tests/depth_fit_mirror.py restates it in numpy, bit for bit).
//
//   depth_fit_plane<R, GATED>   depth_filter_mean's shape: a workgroup of 256 threads owns a 32 x 8 pixel tile, a thread one pixel.  The tile
//                        plus an R-wide halo is staged in LDS once: the map's values (z + 0.0f, NaN for a pixel that is invalid or outside
//                        the frame: NaN fails the depth gate's comparison, so validity needs no flag) and, GATED, the guide byte beside
//                        them.  A thread walks its window in row-major order.  The differences t = z(q) - z(p) of the members feed three
//                        f32 sums, one rounding per operation; the six position moments are integers, masked adds of compile-time
//                        constants (a row's three first, then the row's share of the others), so no indexed register array and no scratch.
//                        The 3 x 3 normal equations are solved by the integer adjugate; every cofactor is below 2^24, exact as a float.
//                        The report's four counters take one ballot and one vector atomic per wave and class, into one of 64 stripes.
//   depth_fit_normals_kernel    rule N1 (normals_rules.hpp) on the fit's (z, gx, gy); a pixel that is not fitted gets zeros.
//   depth_fit_seed_kernel       the recorded slope maps of mvs_propagate_set_slopes into the propagation's gx, gy behind its seed kernel.
// Nothing below depends on the order in which the hardware runs it.  No scalar memory writes.
#include "normals_rules.hpp"
#include "sweep_shared.hpp"

namespace mvs {

namespace {

constexpr int FT_TW = 32, FT_TH = 8, FT_THREADS = FT_TW * FT_TH;   // pixels per tile, one per thread
constexpr int FT_MAX_RADIUS = 4;
// the report's counters: 64 stripes of four 64-bit counters, 128 bytes apart (a cache line each); the report adds the stripes up
constexpr int FT_STRIPES = 64, FT_STRIPE_WORDS = 16;
constexpr size_t FT_COUNTER_BYTES = (size_t)FT_STRIPES * FT_STRIPE_WORDS * sizeof(unsigned long long);

struct FitArgs {
    const float *__restrict__ src;
    float *__restrict__ z, *__restrict__ gx, *__restrict__ gy, *__restrict__ zfit;
    uint8_t *__restrict__ members;
    const uint8_t *__restrict__ guide;   // GATED only
    unsigned long long *__restrict__ counters;
    int W, H, tau, min_members;
    float max_step;
};

__device__ __forceinline__ bool ft_valid(float z) { return z > -1.0f && z < 1.0f; }   // rule F1 (false for NaN)

template <int R, bool GATED>
__global__ __launch_bounds__(FT_THREADS) void depth_fit_plane(const FitArgs a)
{
    constexpr int K = 2 * R + 1, LW = FT_TW + 2 * R, LH = FT_TH + 2 * R, CELLS = LW * LH;
    __shared__ float vals[CELLS];
    __shared__ uint8_t gd[GATED ? CELLS : 1];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * FT_TW, y0 = blockIdx.y * FT_TH;
    for (int e = tid; e < CELLS; e += FT_THREADS) {
        const int ly = e / LW, lx = e - ly * LW;
        const int px = x0 - R + lx, py = y0 - R + ly;
        const bool inside = px >= 0 && px < a.W && py >= 0 && py < a.H;
        const size_t pix = inside ? (size_t)py * a.W + px : 0;
        const float z = a.src[pix];
        vals[e] = inside && ft_valid(z) ? z + 0.0f : __builtin_nanf("");
        if (GATED) gd[e] = inside ? a.guide[pix] : (uint8_t)0;   // (outside the frame: any value, the depth there is NaN)
    }
    __syncthreads();
    const int tx = tid & (FT_TW - 1), ty = tid / FT_TW;
    const int col = x0 + tx, row = y0 + ty;
    const bool live = col < a.W && row < a.H;   // (no early return: every lane of a wave takes part in the ballots below)
    const float c = vals[(ty + R) * LW + tx + R];
    const uint32_t g0 = GATED ? (uint32_t)gd[(ty + R) * LW + tx + R] : 0u, tau = (uint32_t)a.tau;
    int n = 0, Sx = 0, Sy = 0, Sxx = 0, Sxy = 0, Syy = 0;
    float St = 0.0f, Sxt = 0.0f, Syt = 0.0f;
#pragma unroll
    for (int dy = 0; dy < K; dy++) {
        const int dr = dy - R;
        int rn = 0, rx = 0, rxx = 0;   // the row's members, their dc and dc^2
#pragma unroll
        for (int dx = 0; dx < K; dx++) {
            const int dc = dx - R;
            const int e = (ty + dy) * LW + tx + dx;
            float v = vals[e];
            if (GATED) {
                // a pixel the guide gate refuses becomes NaN, in integer arithmetic (as in depth_filter_mean)
                const uint32_t g = gd[e], diff = max(g, g0) - min(g, g0);
                const uint32_t pass = ~(tau - diff) >> 31;   // diff <= tau, both below 256
                v = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, v) | (pass - 1u));
            }
            const float t = v - c;
            const bool in = __builtin_fabsf(t) <= a.max_step;   // rule F3; false for a NaN on either side
            // a pixel that is no member adds (+-0.0f) to sums that start at +0.0f and therefore never are -0.0f: it leaves them as they
            // are, and so does the product of a member's t with dc = 0 or dr = 0.  The condition becomes a register mask at once and is
            // used as one: kept as conditions, a window's worth of them lives in scalar registers and spills those
            uint32_t mask = in ? 0xffffffffu : 0u;
            asm volatile("" : "+v"(mask));   // (opaque: the compiler turns a mask it can see through back into its condition)
            const float tm = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, t) & mask);
            St += tm;
            if (dc != 0) Sxt += (float)dc * tm;
            if (dr != 0) Syt += (float)dr * tm;
            rn -= (int)mask;
            rx += (int)(mask & (uint32_t)dc);
            rxx += (int)(mask & (uint32_t)(dc * dc));
        }
        // a window row at a time: the f32 sums are used only by the lanes that store, and left alone the compiler sinks all of them behind
        // that test and holds the window's differences and masks, 180 vector registers at R = 4, until then
        asm volatile("" : "+v"(St), "+v"(Sxt), "+v"(Syt));
        n += rn;
        Sx += rx;
        Sxx += rxx;
        Sy += dr * rn;
        Syy += (dr * dr) * rn;
        Sxy += dr * rx;
    }
    // rule F5: the adjugate of [[n, Sx, Sy], [Sx, Sxx, Sxy], [Sy, Sxy, Syy]], exact in int32
    const int A00 = Sxx * Syy - Sxy * Sxy, A01 = Sy * Sxy - Sx * Syy, A02 = Sx * Sxy - Sy * Sxx;
    const int A11 = n * Syy - Sy * Sy, A12 = Sx * Sy - n * Sxy, A22 = n * Sxx - Sx * Sx;
    const int D = n * A00 + Sx * A01 + Sy * A02;
    const bool valid = live && c == c, enough = n >= a.min_members;
    const bool fitted = valid && enough && D != 0;
    const float Df = (float)D;   // up to 23 619 600: one round-to-nearest-even conversion
    const float pc = (((float)A00 * St + (float)A01 * Sxt) + (float)A02 * Syt) / Df;
    const float px = (((float)A01 * St + (float)A11 * Sxt) + (float)A12 * Syt) / Df;
    const float py = (((float)A02 * St + (float)A12 * Sxt) + (float)A22 * Syt) / Df;
    if (live) {
        const size_t pix = (size_t)row * a.W + col;
        const float zc = valid ? c : MVS_BACKGROUND_DEPTH;
        const float moved = c + pc;
        a.z[pix] = zc;
        a.gx[pix] = fitted ? px : 0.0f;
        a.gy[pix] = fitted ? py : 0.0f;
        a.zfit[pix] = fitted && ft_valid(moved) ? moved : zc;
        a.members[pix] = fitted ? (uint8_t)n : (uint8_t)0;
    }
    // the report: valid centres, fitted, refused for n < min_members, refused for D = 0.  One ballot and one atomic per wave and class,
    // into the workgroup's stripe of the counters: on four addresses for the whole grid the atomics queue up behind each other and take
    // longer than the fit (0.87 ms of a 1080p call)
    const int cls = !valid ? -1 : fitted ? 1 : !enough ? 2 : 3;
    unsigned long long *stripe = a.counters + (size_t)((blockIdx.y * gridDim.x + blockIdx.x) & (FT_STRIPES - 1)) * FT_STRIPE_WORDS;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long m = __ballot(k == 0 ? valid : cls == k);
        if (m != 0ull && (tid & 63) == 0) atomicAdd(stripe + k, (unsigned long long)__popcll(m));
    }
}

__global__ __launch_bounds__(256) void depth_fit_normals_kernel(const NormalCam k, const float *__restrict__ zmap, const float *__restrict__ gxmap,
                                                                 const float *__restrict__ gymap, const uint8_t *__restrict__ members, float *__restrict__ out, int W,
                                                                 int H, float invW, float invH, float halfW, float halfH)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int row = (int)(p / W), col = (int)(p - (size_t)row * W);
    float nx = 0.f, ny = 0.f, nz = 0.f;
    if (members[p] != 0) rule_n1(k, row, col, zmap[p], gxmap[p], gymap[p], invW, invH, halfW, halfH, nx, ny, nz);
    out[3 * p] = nx;
    out[3 * p + 1] = ny;
    out[3 * p + 2] = nz;
}

// behind propagate_seed: a pixel with a hypothesis takes the caller's slopes, a non-finite one as 0; one without keeps the 0 it got
__global__ __launch_bounds__(256) void depth_fit_seed_kernel(const float *__restrict__ z, float *__restrict__ gx, float *__restrict__ gy,
                                                              const float *__restrict__ seed_gx, const float *__restrict__ seed_gy, size_t P)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P || !ft_valid(z[p])) return;
    const float sx = seed_gx[p], sy = seed_gy[p];
    gx[p] = __builtin_fabsf(sx) < INFINITY ? sx : 0.0f;   // (false for NaN)
    gy[p] = __builtin_fabsf(sy) < INFINITY ? sy : 0.0f;
}

template <int R>
void launch_fit(mvs_ctx *ctx, bool gated, const FitArgs &a)
{
    const dim3 grid((unsigned)div_up(a.W, FT_TW), (unsigned)div_up(a.H, FT_TH));
    if (gated)
        depth_fit_plane<R, true><<<grid, FT_THREADS, 0, ctx->stream>>>(a);
    else
        depth_fit_plane<R, false><<<grid, FT_THREADS, 0, ctx->stream>>>(a);
}

// the stage's one buffer: z, gx, gy, zfit, a spare map (the output of a call whose input is zfit itself), the normals (8 P f32 in all), the
// report's 64-bit counters in their stripes and the members' bytes
struct FitLayout {
    float *maps, *zfit, *spare, *normals;
    unsigned long long *counters;
    uint8_t *members;
};

size_t fit_bytes(size_t P) { return 8 * P * sizeof(float) + FT_COUNTER_BYTES + P; }

FitLayout fit_layout(const mvs_ctx *ctx)
{
    const size_t P = (size_t)ctx->W * ctx->H;
    FitLayout l;
    l.maps = (float *)ctx->dfit_maps.ptr;
    l.zfit = l.maps + 3 * P;
    l.spare = l.maps + 4 * P;
    l.normals = l.maps + 5 * P;
    l.counters = (unsigned long long *)(l.maps + 8 * P);   // 32 P bytes in: 8-byte aligned
    l.members = (uint8_t *)(l.counters + FT_STRIPES * FT_STRIPE_WORDS);
    return l;
}

}  // namespace

// mvs_propagate_init, behind its seed kernel: consumes what mvs_propagate_set_slopes recorded (nothing recorded: nothing is launched)
void dfit_seed_slopes(mvs_ctx *ctx, const float *z, float *gx, float *gy)
{
    if (!ctx->dfit_seed_gx) return;
    const size_t P = (size_t)ctx->W * ctx->H;
    depth_fit_seed_kernel<<<(unsigned)((P + 255) / 256), 256, 0, ctx->stream>>>(z, gx, gy, (const float *)ctx->dfit_seed_gx, (const float *)ctx->dfit_seed_gy, P);
    ctx->dfit_seed_gx = ctx->dfit_seed_gy = nullptr;   // one-shot: a later init must not read a map the caller may have freed
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_depth_fit(mvs_ctx *ctx, const void *depth_dev, const void *guide_dev, int radius, int tau, float max_step, int min_members)
{
    static const char who[] = "mvs_depth_fit";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!depth_dev) return fail(ctx, MVS_EINVAL, "%s: depth_dev is null", who);
    if (radius < 1 || radius > FT_MAX_RADIUS) return fail(ctx, MVS_EINVAL, "%s: radius %d outside 1..%d", who, radius, FT_MAX_RADIUS);
    if (tau < 0 || tau > 255) return fail(ctx, MVS_EINVAL, "%s: tau %d outside 0..255", who, tau);
    if (!(max_step >= 0.0f)) return fail(ctx, MVS_EINVAL, "%s: max_step %g is negative or NaN", who, (double)max_step);
    if (min_members < 3 || min_members > 81) return fail(ctx, MVS_EINVAL, "%s: min_members %d outside 3..81", who, min_members);
    const bool gated = tau < 255;
    const uint8_t *guide = guide_dev ? (const uint8_t *)guide_dev : (ctx->have_main ? main_image_ptr(ctx) : nullptr);
    if (gated && !guide) return fail(ctx, MVS_ESTATE, "%s: tau %d needs a guide image: pass one, or stage a main image (mvs_sweep_set_main)", who, tau);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->dfit_maps, fit_bytes(P)))) return rc;
    const FitLayout l = fit_layout(ctx);
    // a launch never reads the map it writes: an input that is zfit itself (the fitted map of an earlier call) is fitted into the spare
    // map, which is copied over zfit behind the kernel.  (An input that is the stage's z map is rewritten pixel by pixel with the value it
    // is read as, or an invalid one with another invalid one: what a neighbour reads of it means the same before and after.)
    const bool in_place = depth_dev == (const void *)l.zfit;
    FitArgs a;
    a.src = (const float *)depth_dev;
    a.z = l.maps;
    a.gx = l.maps + P;
    a.gy = l.maps + 2 * P;
    a.zfit = in_place ? l.spare : l.zfit;
    a.members = l.members;
    a.guide = gated ? guide : nullptr;
    a.counters = l.counters;
    a.W = ctx->W;
    a.H = ctx->H;
    a.tau = tau;
    a.min_members = min_members;
    a.max_step = max_step;
    MVS_HIP(ctx, hipMemsetAsync(l.counters, 0, FT_COUNTER_BYTES, ctx->stream));
    {
        ProfileScope ps(ctx, MVS_K_ARGMIN);
        switch (radius) {
        case 1: launch_fit<1>(ctx, gated, a); break;
        case 2: launch_fit<2>(ctx, gated, a); break;
        case 3: launch_fit<3>(ctx, gated, a); break;
        default: launch_fit<4>(ctx, gated, a); break;
        }
    }
    MVS_HIP(ctx, hipGetLastError());
    if (in_place) MVS_HIP(ctx, hipMemcpyAsync(l.zfit, l.spare, P * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    ctx->dfit_have = true;
    return MVS_OK;
}

void *mvs_depth_fit_device(mvs_ctx *ctx) { return ctx && ctx->dfit_have ? ctx->dfit_maps.ptr : nullptr; }

void *mvs_depth_fit_depth_device(mvs_ctx *ctx) { return ctx && ctx->dfit_have ? fit_layout(ctx).zfit : nullptr; }

void *mvs_depth_fit_members_device(mvs_ctx *ctx) { return ctx && ctx->dfit_have ? fit_layout(ctx).members : nullptr; }

int mvs_depth_fit_fetch(mvs_ctx *ctx, float *z_hw, float *gx_hw, float *gy_hw, float *zfit_hw, uint8_t *members_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_fit_fetch: null context");
    if (!ctx->dfit_have) return fail(ctx, MVS_ESTATE, "mvs_depth_fit_fetch: no fitted maps yet (mvs_depth_fit first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    const FitLayout l = fit_layout(ctx);
    float *host[4] = {z_hw, gx_hw, gy_hw, zfit_hw};
    for (int k = 0; k < 4; k++)
        if (host[k]) MVS_HIP(ctx, hipMemcpyAsync(host[k], l.maps + k * P, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (members_hw) MVS_HIP(ctx, hipMemcpyAsync(members_hw, l.members, P, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_depth_fit_report(mvs_ctx *ctx, long long out[4])
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_fit_report: null context");
    if (!out) return fail(ctx, MVS_EINVAL, "mvs_depth_fit_report: out is null");
    if (!ctx->dfit_have) return fail(ctx, MVS_ESTATE, "mvs_depth_fit_report: no fitted maps yet (mvs_depth_fit first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    unsigned long long c[FT_STRIPES * FT_STRIPE_WORDS];
    MVS_HIP(ctx, hipMemcpyAsync(c, fit_layout(ctx).counters, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++) {
        out[k] = 0;
        for (int s = 0; s < FT_STRIPES; s++) out[k] += (long long)c[s * FT_STRIPE_WORDS + k];
    }
    return MVS_OK;
}

int mvs_depth_fit_normals(mvs_ctx *ctx, const float cam[16])
{
    static const char who[] = "mvs_depth_fit_normals";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!cam) return fail(ctx, MVS_EINVAL, "%s: cam is null", who);
    if (!ctx->dfit_have) return fail(ctx, MVS_ESTATE, "%s: no fitted maps yet (mvs_depth_fit first)", who);
    mvs_ctx::DepthSlot s;
    if (!slot_matrices(cam, s)) return fail(ctx, MVS_EINVAL, "%s: the camera has a non-finite entry, is singular or has no finite centre", who);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    const FitLayout l = fit_layout(ctx);
    NormalCam k;
    memcpy(k.P, s.P, sizeof(k.P));
    memcpy(k.C, s.C, sizeof(k.C));
    {
        ProfileScope ps(ctx, MVS_K_FUSE);
        depth_fit_normals_kernel<<<(unsigned)((P + 255) / 256), 256, 0, ctx->stream>>>(k, l.maps, l.maps + P, l.maps + 2 * P, l.members, l.normals, ctx->W, ctx->H,
                                                                                    1.0f / (float)ctx->W, 1.0f / (float)ctx->H, (float)ctx->W * 0.5f,
                                                                                    (float)ctx->H * 0.5f);
        MVS_HIP(ctx, hipGetLastError());
    }
    ctx->dfit_normals_have = true;
    return MVS_OK;
}

void *mvs_depth_fit_normals_device(mvs_ctx *ctx) { return ctx && ctx->dfit_normals_have ? fit_layout(ctx).normals : nullptr; }

int mvs_depth_fit_normals_fetch(mvs_ctx *ctx, float *normals_hw3)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_fit_normals_fetch: null context");
    if (!normals_hw3) return fail(ctx, MVS_EINVAL, "mvs_depth_fit_normals_fetch: normals_hw3 is null");
    if (!ctx->dfit_normals_have) return fail(ctx, MVS_ESTATE, "mvs_depth_fit_normals_fetch: no normals yet (mvs_depth_fit_normals first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(normals_hw3, fit_layout(ctx).normals, (size_t)ctx->W * ctx->H * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_propagate_set_slopes(mvs_ctx *ctx, const void *gx_dev, const void *gy_dev)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_set_slopes: null context");
    if ((gx_dev == nullptr) != (gy_dev == nullptr)) return fail(ctx, MVS_EINVAL, "mvs_propagate_set_slopes: one of gx_dev and gy_dev is null (both, or neither to clear)");
    ctx->dfit_seed_gx = gx_dev;
    ctx->dfit_seed_gy = gy_dev;
    return MVS_OK;
}

}  // extern "C"
