// bestk_gated.hip -- the occlusion-robust sweep with a guide-gated support window (DESIGN.md section 26 is the contract;
// tests/gated_mirror.py states it with integer arrays).
//
// mvs_sweep_run_bestk (bestk.hip, section 22) takes every in-frame pixel of the (2 R + 1)^2 square whose sample is inside the view's frame
// as a member of the window.  Beside a depth step half of those pixels lie on the other surface.  Here q is a member of the window of p
// only if, besides, |G(q) - G(p)| <= tau on a guide image G (the staged main image, or the caller's): the gate of mvs_sweep_window
// (window.hip, section 18), but in front of the per-view costs, so that ZNCC's sums and the best-K merge see the gated window.
//
// sweep_fx_bestk_gated<COST, R, KMAX> is sweep_fx_bestk's skeleton up to its first barrier: a 32 x 16-pixel tile, 256 threads, two pixels
// per thread, tile + halo sampled once per (plane, view) into LDS, a chunk of ZN_PC planes in registers, BkList's merge, the fused argmin.
//   The window is not separable (the members depend on the centre): no row sums and no second pass; each pixel adds its own (2 R + 1)^2
//     elements, each ANDed with all ones or zero, so that an element that is gated out adds exact zeros to every field, the count too.
//   The members depend on neither plane nor view: a thread builds the (2 R + 1)^2 bits of its two pixels once, before the plane loop,
//     from the guide's tile + halo in LDS (at most 960 bytes), as 96 bits per pixel, row by row from bit 0.
//   The loop over the window's rows is NOT unrolled and shifts the bits down by a row per turn (propagate.hip keeps its window loops
//     rolled for the same reason): unrolled, every mask of both pixels is invariant in the plane and view loops and is hoisted out of
//     them, 2 x 81 registers at radius 4 (window.hip met the same with 8 x 81 and spilled).
//   Instantiations: 2 costs x 4 radii x KMAX in {0, 2, 4, 8} = 32.  Radius 0 has no window to gate and is refused.
#include "bestk_rules.hpp"   // BkCost, BkList, with_bestk_shape: shared with bestk.hip and propagate.hip

namespace mvs {

namespace {

// the element where m is all ones, exact zeros where m is 0
__device__ __forceinline__ uint4 gate_elem(uint4 e, uint32_t m) { return make_uint4(e.x & m, e.y & m, e.z & m, e.w & m); }
__device__ __forceinline__ uint32_t gate_elem(uint32_t e, uint32_t m) { return e & m; }

template <int COST, int R, int KMAX>
__global__ __launch_bounds__(ZN_THREADS) void sweep_fx_bestk_gated(SweepParams p, const uint32_t *__restrict__ lut_g, const uint8_t *__restrict__ guide, int tau, int keep,
                                                                   int write_volume, int fused)
{
    using S = ZnShape<R>;
    using C = BkCost<COST>;
    using Elem = typename C::Elem;
    constexpr bool ZNCC = COST == MVS_COST_ZNCC;
    constexpr int K = 2 * R + 1;
    static_assert(R >= 1 && K * K <= 96, "a window of up to 96 members");
    __shared__ uint32_t lut[1024];
    __shared__ Elem smp[S::SAMPLES];       // [HH][HW] window elements of the current (plane, view)
    __shared__ uint8_t gl[S::SAMPLES];     // [HH][HW] the guide of tile + halo (outside the frame: any value, the elements there are 0)
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; i++) lut[tid + ZN_THREADS * i] = lut_g[tid + ZN_THREADS * i];
    const int x0 = blockIdx.x * ZN_TW, y0 = blockIdx.y * ZN_TH;
    // this thread's sample positions: elements tid + 256 s of tile + halo
    float sxn[S::NS], syn[S::NS];
    uint32_t sa[S::NS], saa[S::NS];   // ZNCC: a, a a; absolute difference: 255 a, unused
#pragma unroll
    for (int s = 0; s < S::NS; s++) {
        const int i = tid + ZN_THREADS * s;
        const int hy = i / S::HW, hx = i - hy * S::HW;
        const int col = x0 - R + hx, row = y0 - R + hy;
        const bool live = i < S::SAMPLES && col >= 0 && col < p.W && row >= 0 && row < p.H;   // pixels outside the frame are no members
        const size_t at = live ? (size_t)row * p.W + col : 0;
        const uint32_t a = live ? (uint32_t)p.main_img[at] : 0u;
        if (i < S::SAMPLES) gl[i] = live ? guide[at] : (uint8_t)0;
        sa[s] = ZNCC ? a : 255u * a;
        saa[s] = a * a;
        sxn[s] = live ? __builtin_fmaf((float)(2 * col + 1), p.invW, -1.0f) : __builtin_nanf("");
        syn[s] = __builtin_fmaf(-(float)(2 * row + 1), p.invH, 1.0f);
    }
    __syncthreads();
    const int c = tid & (ZN_TW - 1), ty = tid / ZN_TW;   // pixels (c, ty) and (c, ty + 8) of the tile
    const int col = x0 + c;
    // the members of the two windows: bit dy K + dx of pixel h is halo element (ty + 8 h + dy, c + dx)
    uint64_t mlo[2];
    uint32_t mhi[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const uint8_t *g = gl + (ty + 8 * h) * S::HW + c;
        const uint32_t g0 = g[R * S::HW + R];
        mlo[h] = 0ull;
        mhi[h] = 0u;
#pragma unroll
        for (int dy = 0; dy < K; dy++)
#pragma unroll
            for (int dx = 0; dx < K; dx++) {
                const uint32_t gq = g[dy * S::HW + dx];
                const uint32_t in = (max(gq, g0) - min(gq, g0)) <= (uint32_t)tau ? 1u : 0u;
                const int bit = dy * K + dx;
                if (bit < 64)
                    mlo[h] |= (uint64_t)in << bit;
                else
                    mhi[h] |= in << (bit - 64);
            }
    }
    const size_t P = (size_t)p.W * p.H;
    const float hix = ZN_MAGIC + 132.0f + 256.0f * (float)p.W, hiy = ZN_MAGIC + 132.0f + 256.0f * (float)p.H;
    uint32_t best[2] = {0u, 0u};
    int bi[2] = {-1, -1};
    for (int d0 = 0; d0 < p.D; d0 += ZN_PC) {
        const int n = min(ZN_PC, p.D - d0);   // (uniform: the barriers below are reached by every thread or by none)
        BkList<KMAX> acc[2][ZN_PC];
#pragma unroll
        for (int k = 0; k < ZN_PC; k++) {
            acc[0][k].clear();
            acc[1][k].clear();
        }
        for (int v = p.v0; v < p.v0 + p.vcount; v++) {
            const float *q = p.Q + 12 * v;
            Affine A[S::NS];
#pragma unroll
            for (int s = 0; s < S::NS; s++) A[s] = view_affine(q, sxn[s], syn[s]);
            const uint32_t *qv = p.quads + p.pad_slab * (size_t)(p.view_slot ? p.view_slot[v] : v);
#pragma unroll
            for (int k = 0; k < ZN_PC; k++) {
                if (k >= n) break;
                const float z = p.z[d0 + k];
#pragma unroll
                for (int s = 0; s < S::NS; s++) {
                    const int i = tid + ZN_THREADS * s;
                    Elem e;
                    if constexpr (ZNCC)
                        e = zncc_sample(A[s], q[2], q[6], q[10], z, qv, (uint32_t)p.pitch, hix, hiy, lut, sa[s], saa[s]);
                    else
                        e = absdiff_sample(A[s], q[2], q[6], q[10], z, qv, (uint32_t)p.pitch, hix, hiy, lut, sa[s]);
                    if (i < S::SAMPLES) smp[i] = e;
                }
                __syncthreads();
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const Elem *src = smp + (ty + 8 * h) * S::HW + c;   // the window's first row
                    const uint32_t okc = C::ok(src[R * S::HW + R]);      // ok(p): the centre passes its own gate
                    uint64_t lo = mlo[h];
                    uint32_t hi = mhi[h];
                    Elem sum;
                    if constexpr (ZNCC)
                        sum = make_uint4(0u, 0u, 0u, 0u);
                    else
                        sum = 0u;
#pragma unroll 1
                    for (int dy = 0; dy < K; dy++) {
                        const uint32_t bits = (uint32_t)lo;   // the row's K members from bit 0
#pragma unroll
                        for (int dx = 0; dx < K; dx++) sum = C::add(sum, gate_elem(src[dx], 0u - ((bits >> dx) & 1u)));
                        src += S::HW;
                        lo = (lo >> K) | ((uint64_t)hi << (64 - K));
                        hi >>= K;
                    }
                    acc[h][k].insert(C::cost(sum, okc));
                }
                __syncthreads();   // the samples are rewritten behind this
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int row = y0 + ty + 8 * h;
            if (col < p.W && row < p.H) {
                const size_t pix = (size_t)row * p.W + col;
#pragma unroll
                for (int k = 0; k < ZN_PC; k++)
                    if (k < n) {
                        const uint32_t cell = acc[h][k].cell(keep);
                        if (write_volume) __builtin_nontemporal_store(cell, p.volume + (size_t)(d0 + k) * P + pix);  // written once, read by a later kernel
                        if (fused) argmin_update_packed<CS_FIXED>(cell, d0 + k, best[h], bi[h]);
                    }
            }
        }
    }
    if (fused) {
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const int row = y0 + ty + 8 * h;
            if (col < p.W && row < p.H) store_best<CS_FIXED>(p, (size_t)row * p.W + col, best[h] & 0xffffffu, best[h] >> 24, bi[h]);
        }
    }
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_run_bestk_gated(mvs_ctx *ctx, int view_first, int view_count, int cost, int radius, int keep, int tau, const void *guide_dev, unsigned flags)
{
    static const char who[] = "mvs_sweep_run_bestk_gated";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (cost != MVS_COST_ABSDIFF && cost != MVS_COST_ZNCC) return fail(ctx, MVS_EINVAL, "%s: unknown cost %d", who, cost);
    if (radius < 1 || radius > 4) return fail(ctx, MVS_EINVAL, "%s: radius %d outside 1..4 (radius 0 has no window to gate)", who, radius);
    if (keep < 0 || keep > 8) return fail(ctx, MVS_EINVAL, "%s: keep %d outside 1..8 and not MVS_KEEP_ALL", who, keep);
    if (tau < 0 || tau > 255) return fail(ctx, MVS_EINVAL, "%s: tau %d outside 0..255", who, tau);
    return fx_sweep_run(ctx, {who, view_first, view_count, flags, nullptr, ZN_TH, ZN_PC}, [&](const SweepParams &p, const uint32_t *lut, const float *, bool vol, bool fused) {
        const dim3 grid((unsigned)div_up(ctx->W, ZN_TW), (unsigned)div_up(ctx->H, ZN_TH));
        const uint8_t *guide = guide_dev ? (const uint8_t *)guide_dev : p.main_img;   // (the preconditions hold that a main image is staged)
        with_bestk_shape<1>(cost, radius, keep, [&](auto c, auto r, auto kmax) {
            sweep_fx_bestk_gated<decltype(c)::value, decltype(r)::value, decltype(kmax)::value><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, guide, tau, keep, vol, fused);
        });
    });
}
