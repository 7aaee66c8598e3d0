// propagate.hip -- hypothesis propagation: PatchMatch refinement of a depth map (DESIGN.md section 25 is the contract;
// tests/propagate_mirror.py states it in numpy float32 and integer arrays).
//
// Every pixel holds a hypothesis (z, gx, gy) -- the NDC depth at its centre and its change per column and per row, a slanted plane -- and
// the packed cell k << 24 | sum (section 22) of that hypothesis.  An iteration is two checkerboard half-passes; an active pixel tests the
// planes of its neighbours at distance 1 and 5 extended to its own position, then `nrandom` perturbations of what it holds by then, and
// keeps whatever is better by the rule of the depth selection (strict, so ties keep the earlier one).  Neighbours at odd Manhattan
// distance are inactive in the half-pass, so it runs in place without a race.  The per-view windowed cost is section 22's on the fixed
// sampler, with window member q of pixel p sampled at z + gx dc + gy dr; no plane table and no D x H x W volume exist.
//
// propagate_pass<COST, R, KMAX>: a 32 x 16 tile per workgroup, 256 threads, one ACTIVE pixel per thread (col = 2 j + ((row + h) & 1)), so
// all lanes work in a checkerboard pass; the init pass is the same kernel with both colours (two pixels per thread, one after the other)
// and the pixel's own hypothesis as its only candidate.  The main image of tile + halo sits in LDS.  Per candidate the thread loops over
// views and window members, adds the window element of zncc_sample / absdiff_sample in registers (no sums are shared between pixels:
// every pixel has its own plane) and merges the views through BkList<KMAX>.  A member's affine part is computed per member (six FMAs;
// staging it per view in LDS was not tried).  One candidate loop with one call site keeps the code of an instantiation at one window
// loop, and the two window loops are NOT unrolled: unrolled, the samples' frame-test masks of a whole window row are live at once and
// every instantiation with a window spilled 3 to 79 scalar registers (ZNCC at radius 2 took 230 vector registers); as loops none
// spills and the vector registers stay at 54 to 78.  36 instantiations as in bestk.hip.
// The guide gate of DESIGN.md section 26 (mvs_propagate_set_gate) is two kernel arguments, not a template parameter: a member is live only
// if its guide value is within tau of the centre's, read from a second byte tile in LDS (the main image again, or the stage's copy of the
// caller's guide); tau = 255, the default, passes every member, so an ungated run computes what it computed without the gate.
#include "bestk_rules.hpp"

#include <cmath>

namespace mvs {

int ensure_fx_lut(mvs_ctx *ctx);  // sweep_fx.hip: the 32 x 32 weight table on the device

namespace {

constexpr int PR_KEPT = 0, PR_NEAR = 1, PR_FAR = 2, PR_RANDOM = 3;

struct PropArgs {
    float *z, *gx, *gy;              // the hypotheses, H*W each (read and written in place)
    uint32_t *cells;                 // their packed cells
    float *cost;                     // the cells as mean costs (+inf for cell 0)
    unsigned long long *counters;    // kept, near, far, random
    int keep;
    int half;                        // 0 / 1: the half-pass; -1: the init pass
    int nrandom;
    float dz, dg;                    // the random steps of this iteration
    uint32_t seed;                   // mix(seed + (2 t + h))
    int tau;                         // the gate of section 26: member q of p is live only if |G(q) - G(p)| <= tau (255: no gate)
    const uint8_t *guide;            // G, H*W; null: the main image
};

__host__ __device__ __forceinline__ uint32_t prop_mix(uint32_t x)
{
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

__device__ __forceinline__ float prop_uniform(uint32_t x)   // [-1, 1) in steps of 2^-23, every operation exact
{
    return ((float)(int32_t)(x >> 8) - 8388608.0f) * (1.0f / 8388608.0f);
}

__device__ __forceinline__ bool prop_inside(float z) { return z > -1.0f && z < 1.0f; }   // false for NaN

// rule 4: argmin_update_packed<CS_FIXED>'s comparison of two packed cells (the products stay below 2^32: s < 2^24, k < 2^8)
__device__ __forceinline__ bool prop_better(uint32_t c, uint32_t b)
{
    return (c >> 24) != 0u && (b == 0u || umul24u(c & 0xffffffu, b >> 24) < umul24u(b & 0xffffffu, c >> 24));
}

template <int COST, int R, int KMAX>
__global__ __launch_bounds__(ZN_THREADS) void propagate_pass(SweepParams p, const uint32_t *__restrict__ lut_g, PropArgs a)
{
    using S = ZnShape<R>;
    using C = BkCost<COST>;
    using Elem = typename C::Elem;
    constexpr bool ZNCC = COST == MVS_COST_ZNCC;
    __shared__ uint32_t lut[1024];
    __shared__ uint8_t mainl[S::SAMPLES];   // [HH][HW] the main image of tile + halo (0 outside the frame: such a member is never sampled)
    __shared__ uint8_t guidel[S::SAMPLES];  // [HH][HW] the gate's guide likewise: the main image again, or the stage's copy of the caller's
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * ZN_TW, y0 = blockIdx.y * ZN_TH;
#pragma unroll
    for (int i = 0; i < 4; i++) lut[tid + ZN_THREADS * i] = lut_g[tid + ZN_THREADS * i];
    for (int i = tid; i < S::SAMPLES; i += ZN_THREADS) {
        const int hy = i / S::HW, hx = i - hy * S::HW;
        const int col = x0 - R + hx, row = y0 - R + hy;
        const bool in = col >= 0 && col < p.W && row >= 0 && row < p.H;
        const size_t at = in ? (size_t)row * p.W + col : 0;
        const uint8_t m = in ? p.main_img[at] : (uint8_t)0;
        mainl[i] = m;
        guidel[i] = (in && a.guide) ? a.guide[at] : m;
    }
    __syncthreads();   // the only barrier: everything below is per thread
    const float hix = ZN_MAGIC + 132.0f + 256.0f * (float)p.W, hiy = ZN_MAGIC + 132.0f + 256.0f * (float)p.H;
    const bool init = a.half < 0;
    const int ly = tid / (ZN_TW / 2), j = tid - ly * (ZN_TW / 2);
    const int row = y0 + ly;
    int cls = -1;   // the class of what the pixel holds at the end of its list; -1: not an active pixel of the frame
    for (int s = 0; s < (init ? 2 : 1); s++) {
        const int lx = 2 * j + (init ? s : ((row + a.half) & 1));
        const int col = x0 + lx;
        if (col >= p.W || row >= p.H) continue;
        const size_t pix = (size_t)row * p.W + col;
        float z = a.z[pix], gx = a.gx[pix], gy = a.gy[pix];
        uint32_t cell = init ? 0u : a.cells[pix];
        cls = PR_KEPT;
        const uint32_t g0 = guidel[(ly + R) * S::HW + lx + R];
        const int ncand = init ? 1 : 8 + a.nrandom;
        for (int ci = 0; ci < ncand; ci++) {
            // the candidate (cz, cgx, cgy); cz = NaN: there is none (such a candidate has no counted view and never wins)
            float cz = __builtin_nanf(""), cgx = 0.0f, cgy = 0.0f;
            int ccls;
            if (init) {
                cz = z, cgx = gx, cgy = gy;
                ccls = PR_KEPT;
            } else if (ci < 8) {
                const int d = ci < 4 ? 1 : 5;
                const int dc = (ci & 2) ? 0 : ((ci & 1) ? d : -d), dr = (ci & 2) ? ((ci & 1) ? d : -d) : 0;   // (-d,0) (d,0) (0,-d) (0,d)
                const int nc = col + dc, nr = row + dr;
                ccls = ci < 4 ? PR_NEAR : PR_FAR;
                if (nc >= 0 && nc < p.W && nr >= 0 && nr < p.H) {
                    const size_t n = (size_t)nr * p.W + nc;
                    const float zn = a.z[n];
                    if (prop_inside(zn)) {
                        cgx = a.gx[n];
                        cgy = a.gy[n];
                        cz = (zn - cgx * (float)dc) - cgy * (float)dr;   // the neighbour's plane extended to this pixel
                    }
                }
            } else {
                ccls = PR_RANDOM;
                if (prop_inside(z)) {
                    const uint32_t base = prop_mix(a.seed ^ (uint32_t)(row * p.W + col));
                    const uint32_t k = 4u * (uint32_t)(ci - 8);
                    cz = z + a.dz * prop_uniform(prop_mix(base ^ k));
                    cgx = gx + a.dg * prop_uniform(prop_mix(base ^ (k + 1u)));
                    cgy = gy + a.dg * prop_uniform(prop_mix(base ^ (k + 2u)));
                }
            }
            if (!prop_inside(cz)) continue;   // the centre is not live: cell 0
            // rules 1-3: the candidate's cell
            BkList<KMAX> acc;
            acc.clear();
            for (int v = p.v0; v < p.v0 + p.vcount; v++) {
                const float *q = p.Q + 12 * v;
                const uint32_t *qv = p.quads + p.pad_slab * (size_t)(p.view_slot ? p.view_slot[v] : v);
                const float bx = q[2], by = q[6], bw = q[10];
                Elem sum;
                if constexpr (ZNCC)
                    sum = make_uint4(0u, 0u, 0u, 0u);
                else
                    sum = 0u;
                uint32_t centre_ok = 0u;
#pragma unroll 1
                for (int dr = -R; dr <= R; dr++) {
                    const int qr = row + dr;
                    const float yn = __builtin_fmaf(-(float)(2 * qr + 1), p.invH, 1.0f);
                    const float zr = cgy * (float)dr;
#pragma unroll 1
                    for (int dc = -R; dc <= R; dc++) {
                        const int qc = col + dc;
                        const bool in = qc >= 0 && qc < p.W && qr >= 0 && qr < p.H;
                        const float zq = (cz + cgx * (float)dc) + zr;
                        const uint32_t gq = guidel[(ly + dr + R) * S::HW + lx + dc + R];
                        const bool gate = max(gq, g0) - min(gq, g0) <= (uint32_t)a.tau;
                        const float zs = (in && gate && prop_inside(zq)) ? zq : __builtin_nanf("");   // not live: the sampler's s.w > 0 test rejects NaN
                        const float xn = __builtin_fmaf((float)(2 * qc + 1), p.invW, -1.0f);
                        const Affine A = view_affine(q, xn, yn);
                        const uint32_t am = mainl[(ly + dr + R) * S::HW + lx + dc + R];
                        Elem e;
                        if constexpr (ZNCC)
                            e = zncc_sample(A, bx, by, bw, zs, qv, (uint32_t)p.pitch, hix, hiy, lut, am, am * am);
                        else
                            e = absdiff_sample(A, bx, by, bw, zs, qv, (uint32_t)p.pitch, hix, hiy, lut, 255u * am);
                        sum = C::add(sum, e);
                        if (dr == 0 && dc == 0) centre_ok = C::ok(e);
                    }
                }
                acc.insert(C::cost(sum, centre_ok));
            }
            const uint32_t cc = acc.cell(a.keep);
            if (prop_better(cc, cell)) {
                z = cz, gx = cgx, gy = cgy;
                cell = cc;
                cls = ccls;
            }
        }
        a.z[pix] = z;
        a.gx[pix] = gx;
        a.gy[pix] = gy;
        a.cells[pix] = cell;
        a.cost[pix] = cell ? cell_cost<CS_FIXED>(cell & 0xffffffu, cell >> 24) : __builtin_inff();
    }
    if (!init) {
        // the report's counters: one ballot and one atomic per wave and class
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned long long m = __ballot(cls == k);
            if (m != 0ull && (tid & 63) == 0) atomicAdd(a.counters + k, (unsigned long long)__popcll(m));
        }
    }
}

// rule 5: the start map -> z (invalid values become the background depth) and the slopes.  `src` may be the z map itself: a pixel then
// rewrites its own value only, with the value it holds or, for an invalid one, with another invalid one, so what a neighbour reads of
// it means the same before and after
__global__ __launch_bounds__(256) void propagate_seed(const float *src, float *z, float *gx, float *gy, int W, int H, int slopes, float max_step)
{
    const int col = blockIdx.x * 32 + (threadIdx.x & 31), row = blockIdx.y * 8 + (threadIdx.x >> 5);
    if (col >= W || row >= H) return;
    const size_t pix = (size_t)row * W + col;
    const float zp = src[pix];
    const bool has = prop_inside(zp);
    float g[2] = {0.0f, 0.0f};
    if (has && slopes) {
#pragma unroll
        for (int ax = 0; ax < 2; ax++) {
            const int at = ax ? row : col, n = ax ? H : W;
            const size_t stride = ax ? (size_t)W : 1;
            const float zm = at > 0 ? src[pix - stride] : __builtin_nanf(""), zq = at + 1 < n ? src[pix + stride] : __builtin_nanf("");
            const bool um = prop_inside(zm) && fabsf(zm - zp) <= max_step, uq = prop_inside(zq) && fabsf(zq - zp) <= max_step;
            g[ax] = um && uq ? (zq - zm) * 0.5f : uq ? zq - zp : um ? zp - zm : 0.0f;
        }
    }
    z[pix] = has ? zp : MVS_BACKGROUND_DEPTH;
    gx[pix] = g[0];
    gy[pix] = g[1];
}

template <int COST, int R>
void pass_launch(mvs_ctx *ctx, const SweepParams &p, const PropArgs &a)
{
    const dim3 grid((unsigned)div_up(ctx->W, ZN_TW), (unsigned)div_up(ctx->H, ZN_TH));
    const uint32_t *lut = (const uint32_t *)ctx->fx_lut.ptr;
    if (a.keep == MVS_KEEP_ALL)
        propagate_pass<COST, R, 0><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, a);
    else if (a.keep <= 2)
        propagate_pass<COST, R, 2><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, a);
    else if (a.keep <= 4)
        propagate_pass<COST, R, 4><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, a);
    else
        propagate_pass<COST, R, 8><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, a);
}

template <int COST>
void pass_launch_radius(mvs_ctx *ctx, const SweepParams &p, const PropArgs &a, int radius)
{
    switch (radius) {
    case 0:
        if constexpr (COST == MVS_COST_ABSDIFF) pass_launch<COST, 0>(ctx, p, a);   // (refused for ZNCC by the caller)
        break;
    case 1: pass_launch<COST, 1>(ctx, p, a); break;
    case 2: pass_launch<COST, 2>(ctx, p, a); break;
    case 3: pass_launch<COST, 3>(ctx, p, a); break;
    default: pass_launch<COST, 4>(ctx, p, a); break;
    }
}

// one launch of the pass kernel on the recorded cost, radius, keep and view range
void pass(mvs_ctx *ctx, PropArgs &a)
{
    const size_t P = (size_t)ctx->W * ctx->H;
    float *maps = (float *)ctx->prop_maps.ptr;
    a.z = maps;
    a.gx = maps + P;
    a.gy = maps + 2 * P;
    a.cells = (uint32_t *)(maps + 3 * P);
    a.cost = maps + 4 * P;
    a.counters = (unsigned long long *)ctx->prop_counters.ptr;
    a.keep = ctx->prop_keep;
    a.tau = ctx->prop_tau;
    a.guide = ctx->prop_guide_own ? (const uint8_t *)(maps + 5 * P) : nullptr;
    SweepParams p;
    fill_params(ctx, p, ctx->prop_view_first, ctx->prop_view_count, ZN_TH, ZN_PC);
    if (ctx->prop_cost == MVS_COST_ZNCC)
        pass_launch_radius<MVS_COST_ZNCC>(ctx, p, a, ctx->prop_radius);
    else
        pass_launch_radius<MVS_COST_ABSDIFF>(ctx, p, a, ctx->prop_radius);
}

// what init and run refuse alike: the staged state the sampler reads
int staged_state(mvs_ctx *ctx, const char *who)
{
    if (!ctx->have_main || !ctx->have_views) return fail(ctx, MVS_ESTATE, "%s: set main view and side views first", who);
    if (ctx->sampler != MVS_SAMPLER_FIXED) return fail(ctx, MVS_ESTATE, "%s: implemented for MVS_SAMPLER_FIXED (the library default)", who);
    return MVS_OK;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_propagate_init(mvs_ctx *ctx, const void *depth_dev, int view_first, int view_count, int cost, int radius, int keep, float max_step, unsigned flags)
{
    static const char who[] = "mvs_propagate_init";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!depth_dev) return fail(ctx, MVS_EINVAL, "%s: depth_dev is null", who);
    if (cost != MVS_COST_ABSDIFF && cost != MVS_COST_ZNCC) return fail(ctx, MVS_EINVAL, "%s: unknown cost %d", who, cost);
    const int rmin = cost == MVS_COST_ZNCC ? 1 : 0;
    if (radius < rmin || radius > 4) return fail(ctx, MVS_EINVAL, "%s: radius %d outside %d..4", who, radius, rmin);
    if (keep < 0 || keep > 8) return fail(ctx, MVS_EINVAL, "%s: keep %d outside 1..8 and not MVS_KEEP_ALL", who, keep);
    if (flags & ~MVS_PROPAGATE_SLOPES) return fail(ctx, MVS_EINVAL, "%s: unknown flag bits 0x%x (MVS_PROPAGATE_SLOPES only)", who, flags & ~MVS_PROPAGATE_SLOPES);
    if (!(max_step >= 0.0f)) return fail(ctx, MVS_EINVAL, "%s: max_step %g is negative or NaN", who, (double)max_step);
    int rc;
    if ((rc = staged_state(ctx, who))) return rc;
    if (view_first < 0 || view_count < 0 || view_first + view_count > ctx->V)
        return fail(ctx, MVS_EINVAL, "%s: view range [%d,%d) outside 0..%d", who, view_first, view_first + view_count, ctx->V);
    if (ctx->V > 255) return fail(ctx, MVS_EINVAL, "%s: the fixed sampler's cells hold at most 255 views (have %d)", who, ctx->V);
    if (ctx->W > 16383 || ctx->H > 16383) return fail(ctx, MVS_EINVAL, "%s: the fixed sampler addresses images of up to 16383 x 16383", who);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    if ((rc = ensure(ctx, ctx->prop_maps, 5 * P * sizeof(float) + P))) return rc;   // z, gx, gy, the cells, the cost map; the gate's guide (u8)
    if ((rc = ensure(ctx, ctx->prop_counters, 4 * sizeof(unsigned long long)))) return rc;
    if ((rc = ensure_fx_lut(ctx))) return rc;
    ctx->prop_cost = cost;
    ctx->prop_radius = radius;
    ctx->prop_keep = keep;
    ctx->prop_view_first = view_first;
    ctx->prop_view_count = view_count;
    ctx->prop_iter = 0;
    ctx->prop_tau = ctx->prop_gate_tau;
    ctx->prop_guide_own = ctx->prop_gate_guide != nullptr;
    float *maps = (float *)ctx->prop_maps.ptr;
    if (ctx->prop_guide_own) MVS_HIP(ctx, hipMemcpyAsync(maps + 5 * P, ctx->prop_gate_guide, P, hipMemcpyDeviceToDevice, ctx->stream));
    MVS_HIP(ctx, hipMemsetAsync(ctx->prop_counters.ptr, 0, 4 * sizeof(unsigned long long), ctx->stream));
    {
        ProfileScope ps(ctx, MVS_K_SWEEP);
        const dim3 grid((unsigned)div_up(ctx->W, 32), (unsigned)div_up(ctx->H, 8));
        propagate_seed<<<grid, 256, 0, ctx->stream>>>((const float *)depth_dev, maps, maps + P, maps + 2 * P, ctx->W, ctx->H, (flags & MVS_PROPAGATE_SLOPES) ? 1 : 0, max_step);
        PropArgs a = {};
        a.half = -1;
        pass(ctx, a);
    }
    MVS_HIP(ctx, hipGetLastError());
    ctx->prop_have = true;
    return MVS_OK;
}

int mvs_propagate_run(mvs_ctx *ctx, int iterations, float dz, float dg, int nrandom, unsigned seed)
{
    static const char who[] = "mvs_propagate_run";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (iterations < 1) return fail(ctx, MVS_EINVAL, "%s: iterations %d below 1", who, iterations);
    if (nrandom < 0 || nrandom > 4) return fail(ctx, MVS_EINVAL, "%s: nrandom %d outside 0..4", who, nrandom);
    if (!(dz >= 0.0f) || !std::isfinite(dz) || !(dg >= 0.0f) || !std::isfinite(dg))
        return fail(ctx, MVS_EINVAL, "%s: dz %g / dg %g negative or not finite", who, (double)dz, (double)dg);
    int rc;
    if ((rc = staged_state(ctx, who))) return rc;
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "%s: no hypotheses yet (mvs_propagate_init first)", who);
    if (ctx->prop_view_first + ctx->prop_view_count > ctx->V)
        return fail(ctx, MVS_ESTATE, "%s: the views changed since mvs_propagate_init: its range [%d,%d) is outside 0..%d", who, ctx->prop_view_first,
                    ctx->prop_view_first + ctx->prop_view_count, ctx->V);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = ensure_fx_lut(ctx))) return rc;
    {
        ProfileScope ps(ctx, MVS_K_SWEEP);
        for (int i = 0; i < iterations; i++) {
            const long long t = ctx->prop_iter + i;
            PropArgs a = {};
            a.dz = dz;
            a.dg = dg;
            for (long long k = 0; k < t && (a.dz != 0.0f || a.dg != 0.0f); k++) {   // halved t times, one rounding each
                a.dz *= 0.5f;
                a.dg *= 0.5f;
            }
            a.nrandom = nrandom;
            for (int h = 0; h < 2; h++) {
                a.half = h;
                a.seed = prop_mix(seed + (uint32_t)(2 * t + h));
                pass(ctx, a);
            }
        }
    }
    MVS_HIP(ctx, hipGetLastError());
    ctx->prop_iter += iterations;
    return MVS_OK;
}

int mvs_propagate_set_gate(mvs_ctx *ctx, int tau, const void *guide_dev)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_set_gate: null context");
    if (tau < 0 || tau > 255) return fail(ctx, MVS_EINVAL, "mvs_propagate_set_gate: tau %d outside 0..255", tau);
    ctx->prop_gate_tau = tau;
    ctx->prop_gate_guide = guide_dev;
    return MVS_OK;
}

int mvs_propagate_fetch(mvs_ctx *ctx, float *z_hw, float *gx_hw, float *gy_hw, uint32_t *cells_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_fetch: null context");
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "mvs_propagate_fetch: no hypotheses yet (mvs_propagate_init first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    const float *maps = (const float *)ctx->prop_maps.ptr;
    void *const out[4] = {z_hw, gx_hw, gy_hw, cells_hw};
    for (int i = 0; i < 4; i++)
        if (out[i]) MVS_HIP(ctx, hipMemcpyAsync(out[i], maps + i * P, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

void *mvs_propagate_depth_device(mvs_ctx *ctx) { return ctx && ctx->prop_have ? ctx->prop_maps.ptr : nullptr; }

void *mvs_propagate_cost_device(mvs_ctx *ctx) { return ctx && ctx->prop_have ? (float *)ctx->prop_maps.ptr + 4 * (size_t)ctx->W * ctx->H : nullptr; }

int mvs_propagate_report(mvs_ctx *ctx, long long out[5])
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_report: null context");
    if (!out) return fail(ctx, MVS_EINVAL, "mvs_propagate_report: out is null");
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "mvs_propagate_report: no hypotheses yet (mvs_propagate_init first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    std::vector<uint32_t> cells(P);
    unsigned long long counters[4];
    MVS_HIP(ctx, hipMemcpyAsync(counters, ctx->prop_counters.ptr, sizeof(counters), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipMemcpyAsync(cells.data(), (const float *)ctx->prop_maps.ptr + 3 * P, P * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++) out[k] = (long long)counters[k];
    out[4] = 0;
    for (size_t i = 0; i < P; i++) out[4] += cells[i] != 0u;
    return MVS_OK;
}
