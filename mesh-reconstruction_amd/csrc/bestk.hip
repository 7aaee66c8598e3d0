// bestk.hip -- occlusion-robust sweep: the cell keeps the K best (lowest) per-view windowed costs instead of the sum over every view
// (DESIGN.md section 22 is the contract; tests/bestk_mirror.py states it with integer arrays).
//
// A view that cannot see the surface point of a (pixel, plane), because a nearer surface hides it, adds a wrong cost to the summing
// sweeps' cell.  Here the per-view costs c_v of the counted views are merged as k << 24 | (the sum of the k smallest), k = min(keep,
// counted views): the views that disagree most are left out.  The cost of a view is windowed (best-K of single-pixel costs picks texture
// aliasing): either the ZNCC cost of section 21, rules 1-4 unchanged, or the mean of |dot - 255 I_main| over the window's members in integer
// division.  The volume is the packed volume of the ordinary sweep, so everything behind it runs unchanged.
//
// The same cell on the band sweep's planes (mvs_sweep_run_band_bestk; DESIGN.md section 24 is the contract, tests/band_bestk_mirror.py
// states it): plane d of pixel q is  z_d(q) = prior(q) + delta_d  with delta the context's plane table, and window member q is sampled at
// ITS OWN pixel's plane z_d(q), not at z_d(p), so the window follows the prior surface (a slanted support window where the prior is
// smooth).  The state afterwards is the band state (band.hip).  MVS_COST_ZNCC with MVS_KEEP_ALL writes the cells of the ZNCC sweep
// (zncc.hip keeps a kernel of its own: this one was 1-7 % slower there) or is the ZNCC band sweep.
//
// sweep_fx_bestk<COST, R, KMAX, BAND>, sweep_fx_zncc's skeleton: a workgroup is a 32 x 16-pixel tile, 256 threads, two
// pixels per thread (rows ty and ty + 8 of the tile).  Per (plane, view) the threads sample tile + halo once, (32 + 2R)(16 + 2R) samples,
// band.hip's un-tiled sample with one dword gather per quad and the weight table in LDS, into one LDS element each; the window sum is
// separable with plain adds and no unpacking: a horizontal pass ((16 + 2R) x 32 outputs of 2R + 1 reads), a barrier, a vertical pass
// (2R + 1 reads per pixel); a wavefront reads 64 consecutive elements, which is conflict free.  Two barriers per (plane, view): samples ->
// row sums -> pixels; the next iteration's sample writes come behind the second barrier and its row-sum writes behind its own first, so
// neither buffer is doubled.  Barriers are hidden by the other workgroups of the CU, not by a pipeline inside the workgroup.  The view's
// affine part of the thread's sample positions is amortised over a chunk of ZN_PC planes, whose cells live in registers until the
// chunk's epilogue.
//   The window element: ZNCC's 16-byte element (sweep_shared.hpp: zncc_sample; LDS: 4 KiB table + 16 B (HH HW + 32 HH) = 22.6 / 25.3 /
//     28.1 / 31.0 KiB at R = 1 .. 4); for the absolute difference ONE dword e | ok << 24, so that the window sum is N << 24 | S with plain
//     adds (N <= 81 < 2^7, S <= 81 * 65025 < 2^23): a quarter of the LDS and ds_read_b32.  Radius 0 of the absolute difference has no
//     window: the thread's two samples ARE its two pixels, no LDS pass and no barrier.
//   The merge: the kernel keeps the KMAX smallest costs of each (pixel, plane) of the chunk in registers, sorted by a branch-free
//     insertion chain (v_min_u32 / v_max_u32 per slot); a view that does not count carries 0xffffffff, which sinks to the end.  The
//     chunk's epilogue counts and sums the first `keep` slots below the sentinel.  The sum of the k smallest values does not depend on
//     how equal values are ordered, so there is no tie rule.  KMAX = 0 is MVS_KEEP_ALL: a plain accumulator that adds the view's cell.
//   BAND: each of the thread's sample positions loads its prior once, and the z of a sample is prior + delta_d, or NaN for a dead plane
//     (no prior, or the sum outside (-1, 1)); the sampler's own s.w > 0 test rejects NaN, as in band.hip, so there is no second mask.  A
//     position outside the frame carries NaN already.  The add and the range test are done per (view, plane, sample), not once per
//     chunk: a chunk's planes kept in NS x ZN_PC registers cost a wave per SIMD in most instantiations and, where they did, 7 % at
//     1080p x 16 views.  Without BAND `prior` is unused and every sample of a plane has the table's z.
//   Instantiations: (4 radii of ZNCC + 5 of the absolute difference) x KMAX in {0, 2, 4, 8} x BAND = 72; `keep` (<= KMAX) and the two
//     outputs are kernel arguments, uniform branches in the chunk's epilogue, not template parameters (x 3 would be 216 kernels for
//     nothing measurable).
//   The body stays inside the one __global__ template: a thin kernel per sweep around a __forceinline__ body cost 6 vector registers and
//     a wave per SIMD in most instantiations.
#include "bestk_rules.hpp"   // BkCost, BkList, with_bestk_shape, bestk_arguments

namespace mvs {

namespace {

template <int COST, int R, int KMAX, bool BAND>
__global__ __launch_bounds__(ZN_THREADS) void sweep_fx_bestk(SweepParams p, const uint32_t *__restrict__ lut_g, const float *__restrict__ prior, int keep, int write_volume,
                                                              int fused)
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
    // this thread's sample positions: elements tid + 256 s of tile + halo (R = 0: its own two pixels); BAND: each with its own prior
    float sxn[S::NS], syn[S::NS], sz0[BAND ? S::NS : 1];
    uint32_t sa[S::NS], saa[S::NS];   // ZNCC: a, a a; absolute difference: 255 a, unused
#pragma unroll
    for (int s = 0; s < S::NS; s++) {
        const int i = tid + ZN_THREADS * s;
        const int hy = i / S::HW, hx = i - hy * S::HW;
        const int col = x0 - R + hx, row = y0 - R + hy;
        const bool live = i < S::SAMPLES && col >= 0 && col < p.W && row >= 0 && row < p.H;   // pixels outside the frame are no members
        const size_t at = live ? (size_t)row * p.W + col : 0;
        const uint32_t a = live ? (uint32_t)p.main_img[at] : 0u;
        sa[s] = ZNCC ? a : 255u * a;
        saa[s] = a * a;
        sxn[s] = live ? __builtin_fmaf((float)(2 * col + 1), p.invW, -1.0f) : __builtin_nanf("");
        syn[s] = __builtin_fmaf(-(float)(2 * row + 1), p.invH, 1.0f);
        if constexpr (BAND) {
            const float z0 = prior[at];
            sz0[s] = (live && z0 > -1.0f && z0 < 1.0f) ? z0 : __builtin_nanf("");   // section 19 rule 1 (false for NaN)
        }
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
                const float zk = p.z[d0 + k];   // BAND: the offset delta_d
                float zs[S::NS];                // the plane of every sample position; BAND: NaN where it is dead
#pragma unroll
                for (int s = 0; s < S::NS; s++) {
                    if constexpr (BAND) {
                        const float z = sz0[s] + zk;   // one add (section 19 rule 2)
                        zs[s] = (z > -1.0f && z < 1.0f) ? z : __builtin_nanf("");
                    } else {
                        zs[s] = zk;
                    }
                }
                if constexpr (!WINDOW) {
                    // c = e(p): sample s is pixel (c, ty + 8 s)
#pragma unroll
                    for (int h = 0; h < 2; h++) {
                        const uint32_t e = absdiff_sample(A[h], q[2], q[6], q[10], zs[h], qv, (uint32_t)p.pitch, hix, hiy, lut, sa[h]);
                        acc[h][k].insert(e ? e & 0xffffffu : BK_NONE);
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < S::NS; s++) {
                        const int i = tid + ZN_THREADS * s;
                        Elem e;
                        if constexpr (ZNCC)
                            e = zncc_sample(A[s], q[2], q[6], q[10], zs[s], qv, (uint32_t)p.pitch, hix, hiy, lut, sa[s], saa[s]);
                        else
                            e = absdiff_sample(A[s], q[2], q[6], q[10], zs[s], qv, (uint32_t)p.pitch, hix, hiy, lut, sa[s]);
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
            if (col < p.W && row < p.H) store_best<CS_FIXED>(p, (size_t)row * p.W + col, best[h] & 0xffffffu, best[h] >> 24, bi[h]);   // BAND: depth = delta[index], an offset
        }
    }
}

// the launch for checked (cost, radius, keep); `prior` non-null: the band's planes prior + delta
void bestk_tile_launch(mvs_ctx *ctx, const SweepParams &p, const float *prior, int cost, int radius, int keep, bool vol, bool fused)
{
    const dim3 grid((unsigned)div_up(ctx->W, ZN_TW), (unsigned)div_up(ctx->H, ZN_TH));
    const uint32_t *lut = (const uint32_t *)ctx->fx_lut.ptr;
    with_bestk_shape<0>(cost, radius, keep, [&](auto c, auto r, auto kmax) {
        constexpr int COST = decltype(c)::value, R = decltype(r)::value, KMAX = decltype(kmax)::value;
        if (prior)
            sweep_fx_bestk<COST, R, KMAX, true><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, prior, keep, vol, fused);
        else
            sweep_fx_bestk<COST, R, KMAX, false><<<grid, ZN_THREADS, 0, ctx->stream>>>(p, lut, prior, keep, vol, fused);
    });
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_run_bestk(mvs_ctx *ctx, int view_first, int view_count, int cost, int radius, int keep, unsigned flags)
{
    static const char who[] = "mvs_sweep_run_bestk";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (int rc = bestk_arguments(ctx, who, cost, radius, keep)) return rc;
    return fx_sweep_run(ctx, {who, view_first, view_count, flags, nullptr, ZN_TH, ZN_PC}, [&](const SweepParams &p, const uint32_t *, const float *prior, bool vol, bool fused) {
        bestk_tile_launch(ctx, p, prior, cost, radius, keep, vol, fused);
    });
}

int mvs_sweep_run_band_bestk(mvs_ctx *ctx, int view_first, int view_count, const void *prior_dev, int cost, int radius, int keep, unsigned flags)
{
    static const char who[] = "mvs_sweep_run_band_bestk";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!prior_dev) return fail(ctx, MVS_EINVAL, "%s: prior_dev is null", who);
    if (int rc = bestk_arguments(ctx, who, cost, radius, keep)) return rc;
    return fx_sweep_run(ctx, {who, view_first, view_count, flags, prior_dev, ZN_TH, ZN_PC}, [&](const SweepParams &p, const uint32_t *, const float *prior, bool vol, bool fused) {
        bestk_tile_launch(ctx, p, prior, cost, radius, keep, vol, fused);
    });
}
