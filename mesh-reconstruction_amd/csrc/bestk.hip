// bestk.hip -- occlusion-robust sweep: the cell keeps the K best (lowest) per-view windowed costs instead of the sum over every view
// (DESIGN.md section 22 is the contract; tests/bestk_mirror.py states it with integer arrays).
//
// A view that cannot see the surface point of a (pixel, plane), because a nearer surface hides it, adds a wrong cost to the summing
// sweeps' cell.  Here the per-view costs c_v of the counted views are merged as k << 24 | (the sum of the k smallest), k = min(keep,
// counted views): the views that disagree most are left out.  The cost of a view is windowed (best-K of single-pixel costs picks texture
// aliasing): either the ZNCC cost of zncc.hip, rules 1-4 unchanged, or the mean of |dot - 255 I_main| over the window's members in integer
// division.  The volume is the packed volume of the ordinary sweep, so everything behind it runs unchanged.
//
// sweep_fx_bestk<COST, R, KMAX> is sweep_fx_zncc's skeleton: a 32 x 16-pixel tile, 256 threads, two pixels per thread, tile + halo sampled
// once per (plane, view) into LDS, a separable window sum (horizontal pass, barrier, vertical pass), a chunk of ZN_PC planes in registers.
//   The window element: ZNCC's 16-byte element as it is (sweep_shared.hpp); for the absolute difference ONE dword e | ok << 24, so that
//     the window sum is N << 24 | S with plain adds (N <= 81 < 2^7, S <= 81 * 65025 < 2^23): a quarter of the LDS and ds_read_b32.
//     Radius 0 of the absolute difference has no window: the thread's two samples ARE its two pixels, no LDS pass and no barrier.
//   The merge: where sweep_fx_zncc adds the view's cell, this kernel keeps the KMAX smallest costs of each (pixel, plane) of the chunk in
//     registers, sorted by a branch-free insertion chain (v_min_u32 / v_max_u32 per slot); a view that does not count carries 0xffffffff,
//     which sinks to the end.  The chunk's epilogue counts and sums the first `keep` slots below the sentinel.  The sum of the k smallest
//     values does not depend on how equal values are ordered, so there is no tie rule.  KMAX = 0 is MVS_KEEP_ALL: a plain accumulator.
//   Instantiations: (4 radii of ZNCC + 5 of the absolute difference) x KMAX in {0, 2, 4, 8} = 36; `keep` (<= KMAX) and the two outputs are
//     kernel arguments, uniform branches in the chunk's epilogue, not template parameters (x 3 would be 108 kernels for nothing measurable).
#include "bestk_rules.hpp"   // BkCost, BkList, absdiff_sample: shared with band_bestk.hip

namespace mvs {

int ensure_fx_lut(mvs_ctx *ctx);  // sweep_fx.hip: the 32 x 32 weight table on the device

namespace {

template <int COST, int R, int KMAX>
__global__ __launch_bounds__(ZN_THREADS) void sweep_fx_bestk(SweepParams p, const uint32_t *__restrict__ lut_g, int keep, int write_volume, int fused)
{
    using S = ZnShape<R>;
    using C = BkCost<COST>;
    using Elem = typename C::Elem;
    constexpr bool ZNCC = COST == MVS_COST_ZNCC;
    constexpr bool WINDOW = R > 0;
    __shared__ uint32_t lut[1024];
    __shared__ Elem smp[WINDOW ? S::SAMPLES : 1];    // [HH][HW] window elements of the current (plane, view)
    __shared__ Elem rows[WINDOW ? S::ROWSUMS : 1];   // [HH][32] horizontal sums
    const int tid = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 4; i++) lut[tid + ZN_THREADS * i] = lut_g[tid + ZN_THREADS * i];
    __syncthreads();
    const int x0 = blockIdx.x * ZN_TW, y0 = blockIdx.y * ZN_TH;
    // this thread's sample positions: elements tid + 256 s of tile + halo (R = 0: its own two pixels)
    float sxn[S::NS], syn[S::NS];
    uint32_t sa[S::NS], saa[S::NS];   // ZNCC: a, a a; absolute difference: 255 a, unused
#pragma unroll
    for (int s = 0; s < S::NS; s++) {
        const int i = tid + ZN_THREADS * s;
        const int hy = i / S::HW, hx = i - hy * S::HW;
        const int col = x0 - R + hx, row = y0 - R + hy;
        const bool live = i < S::SAMPLES && col >= 0 && col < p.W && row >= 0 && row < p.H;   // pixels outside the frame are no members
        const uint32_t a = live ? (uint32_t)p.main_img[(size_t)row * p.W + col] : 0u;
        sa[s] = ZNCC ? a : 255u * a;
        saa[s] = a * a;
        sxn[s] = live ? __builtin_fmaf((float)(2 * col + 1), p.invW, -1.0f) : __builtin_nanf("");
        syn[s] = __builtin_fmaf(-(float)(2 * row + 1), p.invH, 1.0f);
    }
    const int c = tid & (ZN_TW - 1), ty = tid / ZN_TW;   // pixels (c, ty) and (c, ty + 8) of the tile
    const int col = x0 + c;
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
                if constexpr (!WINDOW) {
                    // c = e(p): sample s is pixel (c, ty + 8 s)
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const uint32_t e = absdiff_sample(A[h], q[2], q[6], q[10], z, qv, (uint32_t)p.pitch, hix, hiy, lut, sa[h]);
                        acc[h][k].insert(e ? e & 0xffffffu : BK_NONE);
                    }
                } else {
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
                    for (int t = 0; t < S::NR; t++) {
                        const int j = tid + ZN_THREADS * t;   // row sum (hy, cc) = (j / 32, j % 32): elements cc .. cc + 2R of row hy
                        if (j < S::ROWSUMS) {
                            const Elem *src = smp + (j / ZN_TW) * S::HW + (j & (ZN_TW - 1));
                            Elem sum = src[0];
#pragma unroll
                            for (int e = 1; e <= 2 * R; e++) sum = C::add(sum, src[e]);
                            rows[j] = sum;
                        }
                    }
                    // ok(p) of the thread's own pixels: read here, the samples are rewritten behind the next barrier
                    const uint32_t ok0 = C::ok(smp[(ty + R) * S::HW + c + R]), ok1 = C::ok(smp[(ty + 8 + R) * S::HW + c + R]);
                    __syncthreads();
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const Elem *src = rows + (ty + 8 * h) * ZN_TW + c;   // rows ty + 8h .. + 2R of the halo = the window of tile row ty + 8h
                        Elem sum = src[0];
#pragma unroll
                        for (int e = 1; e <= 2 * R; e++) sum = C::add(sum, src[e * ZN_TW]);
                        acc[h][k].insert(C::cost(sum, h ? ok1 : ok0));
                    }
                }
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

template <int COST, int R>
void bestk_launch(mvs_ctx *ctx, const SweepParams &p, int keep, bool vol, bool fused)
{
    const dim3 grid((unsigned)div_up(ctx->W, ZN_TW), (unsigned)div_up(ctx->H, ZN_TH));
    const uint32_t *lut = (const uint32_t *)ctx->fx_lut.ptr;
    if (keep == MVS_KEEP_ALL)
        sweep_fx_bestk<COST, R, 0><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, keep, vol, fused);
    else if (keep <= 2)
        sweep_fx_bestk<COST, R, 2><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, keep, vol, fused);
    else if (keep <= 4)
        sweep_fx_bestk<COST, R, 4><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, keep, vol, fused);
    else
        sweep_fx_bestk<COST, R, 8><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, keep, vol, fused);
}

template <int COST>
void bestk_launch_radius(mvs_ctx *ctx, const SweepParams &p, int radius, int keep, bool vol, bool fused)
{
    switch (radius) {
    case 0:
        if constexpr (COST == MVS_COST_ABSDIFF) bestk_launch<COST, 0>(ctx, p, keep, vol, fused);   // (refused for ZNCC by the caller)
        break;
    case 1: bestk_launch<COST, 1>(ctx, p, keep, vol, fused); break;
    case 2: bestk_launch<COST, 2>(ctx, p, keep, vol, fused); break;
    case 3: bestk_launch<COST, 3>(ctx, p, keep, vol, fused); break;
    default: bestk_launch<COST, 4>(ctx, p, keep, vol, fused); break;
    }
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_run_bestk(mvs_ctx *ctx, int view_first, int view_count, int cost, int radius, int keep, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_run_bestk: null context");
    if (cost != MVS_COST_ABSDIFF && cost != MVS_COST_ZNCC) return fail(ctx, MVS_EINVAL, "mvs_sweep_run_bestk: unknown cost %d", cost);
    const int rmin = cost == MVS_COST_ZNCC ? 1 : 0;
    if (radius < rmin || radius > 4) return fail(ctx, MVS_EINVAL, "mvs_sweep_run_bestk: radius %d outside %d..4", radius, rmin);
    if (keep < 0 || keep > 8) return fail(ctx, MVS_EINVAL, "mvs_sweep_run_bestk: keep %d outside 1..8 and not MVS_KEEP_ALL", keep);
    bool vol, fused;
    int rc;
    if ((rc = fx_sweep_preconditions(ctx, "mvs_sweep_run_bestk", view_first, view_count, flags, vol, fused))) return rc;
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    if ((rc = sweep_outputs(ctx, vol, "mvs_sweep_run_bestk"))) return rc;
    if ((rc = ensure_fx_lut(ctx))) return rc;
    SweepParams p;
    fill_params(ctx, p, view_first, view_count, ZN_TH, ZN_PC);
    {
        ProfileScope ps(ctx, MVS_K_SWEEP);
        if (cost == MVS_COST_ZNCC)
            bestk_launch_radius<MVS_COST_ZNCC>(ctx, p, radius, keep, vol, fused);
        else
            bestk_launch_radius<MVS_COST_ABSDIFF>(ctx, p, radius, keep, vol, fused);
    }
    MVS_HIP(ctx, hipGetLastError());
    note_ordinary_sweep(ctx);
    fused ? note_full_selection(ctx) : note_no_selection(ctx);
    return MVS_OK;
}
