// window.hip -- windowed matching cost: gated box aggregation of the packed volume (include/mvs.h "mvs_sweep_window", DESIGN.md
// section 18 holds the arithmetic contract; tests/window_mirror.py restates it in numpy, bit for bit).  Integer arithmetic only, so
// nothing below depends on the order in which the hardware runs it.
//   window_kernel<R, CS, GATED>   one wavefront owns a 64 x 8 pixel tile for all planes; a lane owns a COLUMN of 8 pixels.  Plane d's
//                        cells of the tile plus an R-wide halo ((64 + 2R) x (8 + 2R) dwords; a cell outside the frame or with count 0
//                        staged as 0, so it adds nothing) sit in one of two LDS slots; plane d + 1's loads are issued before plane d is
//                        summed and land in the other slot afterwards: one barrier per plane.  A cell read from LDS serves every pixel
//                        of the lane's column whose window holds it, so a lane reads (8 + 2R)(2R + 1) cells for 8 pixels, not
//                        8 (2R + 1)^2.
//                        GATED: the members of a pixel's window do not depend on the plane; each lane builds the (2R + 1)^2 membership
//                        bits of its 8 pixels once, from the guide's tile plus halo staged in the same LDS, and reuses them for every
//                        plane.  Not GATED (tau = 255, or R = 0): the window is separable; the lane sums the 8 + 2R rows once each and
//                        the 8 pixels add 2R + 1 row sums.  Both give the same bytes where they overlap (tests).
//                        floor(S n / N) is a float estimate corrected by exact 32-bit integer arithmetic (window_quotient).
//                        With `select` the kernel keeps, per pixel, the running best cell of Wv with its plane and the cells of Wv next
//                        to it while it walks the planes, and writes the depth / cost / index maps (and the parabola of
//                        select_rules.hpp) at the end: what mvs_sweep_argmin + mvs_sweep_refine_depth give on Wv, without reading Wv again.
// Which packed volume the readers read (mvs_sweep_set_volume_source) is select.hip's decision.
// No atomics, no scalar memory writes.
#include "sweep_shared.hpp"

namespace mvs {

namespace {

constexpr int kWinTileW = 64, kWinTileH = 8, kWinMaxRadius = 4;

// floor(S n / N) for S < 2^32, n < 2^9, 0 < N < 2^15 and a quotient below 2^24 + 2^20 (the contract's cells: N >= n and S <= N * the
// largest per-sample cost).  The float estimate is off by at most 6 (three roundings and v_rcp_f32's 1 ulp on a value below 2^24.1), so the
// remainder S n - q N is below 2^18 in magnitude and its low 32 bits are the remainder: no 64-bit product is formed.  A second estimate
// from that remainder is off by at most 1 either way, which the two tests settle.  tools/window_quotient_check.cpp runs the same
// arithmetic on the host against 64-bit division, with the reciprocal perturbed by an ulp either way.
__device__ __forceinline__ uint32_t window_quotient(uint32_t S, uint32_t n, uint32_t N)
{
    const float rn = __builtin_amdgcn_rcpf((float)N);
    const uint32_t lo = S * n;
    uint32_t q = (uint32_t)(((float)S * (float)n) * rn);
    int r = (int)(lo - q * N);
    q += (uint32_t)(int)__builtin_floorf((float)r * rn);
    r = (int)(lo - q * N);
    if (r < 0) {
        q -= 1u;
        r += (int)N;
    }
    if (r >= (int)N) q += 1u;
    return q;
}

// all ones when bit b of v is set, else 0
__device__ __forceinline__ uint32_t bit_mask(uint32_t v, int b) { return (uint32_t)((int32_t)(v << (31 - b)) >> 31); }

struct WindowArgs {
    const uint32_t *__restrict__ vol;   // [D][H][W] packed cells, read only
    uint32_t *__restrict__ out;         // Wv
    const uint8_t *__restrict__ guide;  // H*W u8 (GATED only)
    const float *__restrict__ z;
    float *__restrict__ depth;
    float *__restrict__ cost;
    int *__restrict__ index;
    int W, H, D, tau, select, refine;
};

template <int R, int CS, bool GATED>
__global__ __launch_bounds__(64) void window_kernel(const WindowArgs a)
{
    constexpr int K = 2 * R + 1, LW = kWinTileW + 2 * R, LH = kWinTileH + 2 * R, CELLS = LW * LH, NE = (CELLS + 63) / 64;
    constexpr int MW = (K * K + 31) / 32, TH = kWinTileH;
    constexpr uint32_t M = (1u << CS) - 1u;
    __shared__ uint32_t slot[2][CELLS];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * kWinTileW, y0 = blockIdx.y * kWinTileH;
    const int W = a.W, H = a.H, D = a.D;
    const size_t P = (size_t)W * H;

    // element e = 64 k + lane of the staged region: its pixel number in a plane and bit k of `inside`; an element beyond the frame or beyond
    // the region loads pixel 0 and is masked to 0.  (Masks, not conditions: a condition per element is a pair of SGPRs kept for the whole
    // plane loop, and 18 of those, with the 8 of the stores, spill.)
    uint32_t off[NE], inside = 0u;
#pragma unroll
    for (int k = 0; k < NE; k++) {
        const int e = 64 * k + lane, row = e / LW, col = e - row * LW;
        const int gy = y0 - R + row, gx = x0 - R + col;
        const bool ok = e < CELLS && gx >= 0 && gx < W && gy >= 0 && gy < H;
        off[k] = ok ? (uint32_t)gy * (uint32_t)W + (uint32_t)gx : 0u;
        inside |= (ok ? 1u : 0u) << k;
    }
    static_assert(NE <= 32, "one bit per staged element of a lane");
    int nrows = H - y0 < TH ? H - y0 : TH;   // rows of the tile inside the frame (uniform)
    const bool xok = x0 + lane < W;

    // membership bits of the lane's 8 pixels: bit dy K + dx of pixel i is neighbour (i + dy - R, lane + dx - R)
    uint32_t member[TH][MW];
    if (GATED) {
#pragma unroll
        for (int k = 0; k < NE; k++) {
            const int e = 64 * k + lane;
            if (64 * k + 63 < CELLS || e < CELLS) slot[0][e] = (uint32_t)a.guide[off[k]];   // (outside the frame: any value, the cells there are 0)
        }
        __syncthreads();
        const uint32_t tau = (uint32_t)a.tau;
#pragma unroll
        for (int i = 0; i < TH; i++) {
#pragma unroll
            for (int w = 0; w < MW; w++) member[i][w] = 0u;
            const uint32_t g0 = slot[0][(i + R) * LW + lane + R];
#pragma unroll
            for (int dy = 0; dy < K; dy++)
#pragma unroll
                for (int dx = 0; dx < K; dx++) {
                    const uint32_t g = slot[0][(i + dy) * LW + lane + dx];
                    const uint32_t diff = max(g, g0) - min(g, g0);
                    const int bit = dy * K + dx;
                    member[i][bit >> 5] |= (~(tau - diff) >> 31) << (bit & 31);   // diff <= tau, both below 256
                }
        }
        __syncthreads();
    }

    // selection state per pixel: best cell of Wv, its plane, the cell of the plane before the current one, the cells next to the best
    uint32_t best[TH], prev[TH], before[TH], after[TH];
    int bi[TH];
#pragma unroll
    for (int i = 0; i < TH; i++) {
        best[i] = prev[i] = before[i] = after[i] = 0u;
        bi[i] = -1;
    }

    uint32_t pf[NE];
#pragma unroll
    for (int k = 0; k < NE; k++) {
        const uint32_t c = a.vol[off[k]] & bit_mask(inside, k);
        if (64 * k + 63 < CELLS || 64 * k + lane < CELLS) slot[0][64 * k + lane] = (c >> CS) ? c : 0u;
    }

    for (int d = 0; d < D; d++) {
        __syncthreads();   // plane d is in slot[d & 1]; everybody is done reading the other slot
        const bool more = d + 1 < D;
        if (more) {
            const uint32_t *vn = a.vol + (size_t)(d + 1) * P;
#pragma unroll
            for (int k = 0; k < NE; k++) pf[k] = vn[off[k]];
        }
        // (plane-invariant values the loop is to make again, not to keep in registers: see the membership bits below)
        asm volatile("" : "+v"(inside));
        asm volatile("" : "+s"(nrows));
        const uint32_t *s = slot[d & 1];
        uint32_t S[TH], N[TH], own[TH];
#pragma unroll
        for (int i = 0; i < TH; i++) S[i] = N[i] = own[i] = 0u;
        if (!GATED) {
            uint32_t rs[LH], rn[LH];
#pragma unroll
            for (int j = 0; j < LH; j++) {
                uint32_t ss = 0u, nn = 0u;
#pragma unroll
                for (int dx = 0; dx < K; dx++) {
                    const uint32_t c = s[j * LW + lane + dx];
                    ss += c & M;
                    nn += c >> CS;
                    if (dx == R && j >= R && j < R + TH) own[j - R] = c;
                }
                rs[j] = ss;
                rn[j] = nn;
            }
#pragma unroll
            for (int i = 0; i < TH; i++)
#pragma unroll
                for (int dy = 0; dy < K; dy++) {
                    S[i] += rs[i + dy];
                    N[i] += rn[i + dy];
                }
        } else {
            // the bits are the same for every plane, and so is every mask made from them: left visible, all 8 K K masks are hoisted out of
            // the plane loop and spilled.  Behind this the loop makes them again, one shift each.
#pragma unroll
            for (int i = 0; i < TH; i++)
#pragma unroll
                for (int w = 0; w < MW; w++) asm volatile("" : "+v"(member[i][w]));
#pragma unroll
            for (int j = 0; j < LH; j++)
#pragma unroll
                for (int dx = 0; dx < K; dx++) {
                    const uint32_t c = s[j * LW + lane + dx];
                    if (dx == R && j >= R && j < R + TH) own[j - R] = c;
                    const uint32_t cs = c & M, cn = c >> CS;   // unpacked once, for the up to K pixels of the column that hold the cell
#pragma unroll
                    for (int i = 0; i < TH; i++) {
                        const int dy = j - i;   // row of the window of pixel i
                        if (dy >= 0 && dy < K) {
                            const int bit = dy * K + dx;
                            const uint32_t in = (member[i][bit >> 5] >> (bit & 31)) & 1u;
                            S[i] = umul24u(cs, in) + S[i];   // three full-rate instructions per (pixel, neighbour): the bit and two 24-bit multiply-adds
                            N[i] = umul24u(cn, in) + N[i];
                        }
                    }
                }
        }
        uint32_t *on = a.out + (size_t)d * P;
        const int x = x0 + lane;
#pragma unroll
        for (int i = 0; i < TH; i++) {
            const uint32_t n = own[i] >> CS;
            const uint32_t q = window_quotient(S[i], n, N[i] ? N[i] : 1u);
            const uint32_t cell = n ? (n << CS) | q : 0u;
            if (i < nrows && xok) on[(size_t)(y0 + i) * W + x] = cell;
            if (a.select) {
                after[i] = d == bi[i] + 1 ? cell : after[i];
                const bool better = n != 0u && (bi[i] < 0 || umul24u(q, best[i] >> CS) < umul24u(best[i] & M, n));
                before[i] = better ? prev[i] : before[i];
                after[i] = better ? 0u : after[i];
                best[i] = better ? cell : best[i];
                bi[i] = better ? d : bi[i];
                prev[i] = cell;
            }
        }
        if (more) {
            uint32_t *nx = slot[(d + 1) & 1];
#pragma unroll
            for (int k = 0; k < NE; k++) {
                const uint32_t c = pf[k] & bit_mask(inside, k);
                if (64 * k + 63 < CELLS || 64 * k + lane < CELLS) nx[64 * k + lane] = (c >> CS) ? c : 0u;
            }
        }
    }

    if (a.select) {
        const int x = x0 + lane;
#pragma unroll
        for (int i = 0; i < TH; i++) {
            if (x >= W || y0 + i >= H) continue;
            const size_t p = (size_t)(y0 + i) * W + x;
            const int b = bi[i];
            a.index[p] = b;
            if (b < 0) {
                a.depth[p] = MVS_BACKGROUND_DEPTH;
                a.cost[p] = __builtin_inff();
                continue;
            }
            a.cost[p] = cell_cost<CS>(best[i] & M, best[i] >> CS);
            float zr = a.z[b];
            if (a.refine && b > 0 && b < D - 1 && (before[i] >> CS) != 0u && (after[i] >> CS) != 0u)
                zr = refine_parabola(cell_mean<CS>(before[i]), cell_mean<CS>(best[i]), cell_mean<CS>(after[i]), a.z, b, D);
            a.depth[p] = zr;
        }
    }
}

template <int R>
void launch_window(mvs_ctx *ctx, bool gated, const WindowArgs &a)
{
    const dim3 grid((unsigned)div_up(a.W, kWinTileW), (unsigned)div_up(a.H, kWinTileH));
    with_cells(ctx, [&](auto cs) {
        constexpr int CS = decltype(cs)::value;
        if (gated)
            window_kernel<R, CS, (R > 0)><<<grid, 64, 0, ctx->stream>>>(a);   // radius 0 has no neighbours to gate: no such instantiation
        else
            window_kernel<R, CS, false><<<grid, 64, 0, ctx->stream>>>(a);
    });
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_window(mvs_ctx *ctx, int radius, int tau, const void *guide_dev, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_window: null context");
    if (radius < 0 || radius > kWinMaxRadius) return fail(ctx, MVS_EINVAL, "mvs_sweep_window: radius %d outside 0..%d", radius, kWinMaxRadius);
    if (tau < 0 || tau > 255) return fail(ctx, MVS_EINVAL, "mvs_sweep_window: tau %d outside 0..255", tau);
    if (flags & ~(MVS_WINDOW_SELECT | MVS_WINDOW_REFINE))
        return fail(ctx, MVS_EINVAL, "mvs_sweep_window: unknown flag bits 0x%x", flags & ~(MVS_WINDOW_SELECT | MVS_WINDOW_REFINE));
    if ((flags & MVS_WINDOW_REFINE) && !(flags & MVS_WINDOW_SELECT)) return fail(ctx, MVS_EINVAL, "mvs_sweep_window: MVS_WINDOW_REFINE without MVS_WINDOW_SELECT");
    const int W = ctx->W, H = ctx->H, D = ctx->D;
    const size_t P = (size_t)W * H, N = P * (size_t)D;
    if (P > (size_t)INT_MAX) return fail(ctx, MVS_EINVAL, "mvs_sweep_window: %zu pixels do not fit the 32-bit pixel numbers", P);
    if (!ctx->have_planes || D < 1) return fail(ctx, MVS_ESTATE, "mvs_sweep_window: no planes (mvs_sweep_set_planes first)");
    if (!ctx->volume || ctx->volume_bytes < N * sizeof(uint32_t))
        return fail(ctx, MVS_ESTATE, "mvs_sweep_window: no packed volume of %d x %d x %d cells (mvs_sweep_run with MVS_SWEEP_VOLUME)", D, H, W);
    if (int rc = cells_readable(ctx, "mvs_sweep_window", "the packed volume", ctx->vol_cells_sampler)) return rc;
    const bool gated = radius > 0 && tau < 255;
    const uint8_t *guide = guide_dev ? (const uint8_t *)guide_dev : (ctx->have_main ? main_image_ptr(ctx) : nullptr);
    if (gated && !guide) return fail(ctx, MVS_ESTATE, "mvs_sweep_window: tau %d needs a guide image: pass one, or stage a main image (mvs_sweep_set_main)", tau);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const bool select = (flags & MVS_WINDOW_SELECT) != 0;
    int rc;
    if (select && (rc = ensure_maps(ctx))) return rc;
    if (ctx->win_vol.bytes < N * sizeof(uint32_t)) {
        // a larger Wv: the new buffer first, so that a failed allocation leaves the old Wv as it was (ensure() frees before it allocates)
        DevBuf larger;
        if ((rc = ensure(ctx, larger, N * sizeof(uint32_t)))) return rc;
        if (ctx->win_vol.ptr) {
            hipError_t e = hipStreamSynchronize(ctx->stream);   // queued kernels may still read the old one
            if (e == hipSuccess) e = hipFree(ctx->win_vol.ptr);
            if (e != hipSuccess) {
                (void)hipFree(larger.ptr);
                return fail(ctx, MVS_EHIP, "mvs_sweep_window: releasing the smaller windowed volume failed: %s", hipGetErrorString(e));
            }
        }
        ctx->win_vol = larger;
        note_no_window(ctx);   // no Wv until this call's launch is queued
    }
    WindowArgs a;
    a.vol = ctx->volume;
    a.out = (uint32_t *)ctx->win_vol.ptr;
    a.guide = guide;
    a.z = (const float *)ctx->ztab.ptr;
    a.depth = (float *)ctx->depth.ptr;
    a.cost = (float *)ctx->cost.ptr;
    a.index = (int *)ctx->index.ptr;
    a.W = W;
    a.H = H;
    a.D = D;
    a.tau = tau;
    a.select = select ? 1 : 0;
    a.refine = (flags & MVS_WINDOW_REFINE) ? 1 : 0;
    ProfileScope ps(ctx, MVS_K_ARGMIN);
    switch (radius) {
    case 0: launch_window<0>(ctx, gated, a); break;
    case 1: launch_window<1>(ctx, gated, a); break;
    case 2: launch_window<2>(ctx, gated, a); break;
    case 3: launch_window<3>(ctx, gated, a); break;
    default: launch_window<4>(ctx, gated, a); break;
    }
    MVS_HIP(ctx, hipGetLastError());
    note_window_written(ctx);
    if (select) note_full_selection(ctx);
    return MVS_OK;
}

void *mvs_sweep_windowed_device(mvs_ctx *ctx, size_t *bytes)
{
    if (bytes) *bytes = 0;
    if (!ctx || !ctx->win_planes) return nullptr;
    if (bytes) *bytes = (size_t)ctx->win_planes * ctx->W * ctx->H * sizeof(uint32_t);
    return ctx->win_vol.ptr;
}

int mvs_sweep_window_fetch(mvs_ctx *ctx, uint32_t *cells_dhw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_window_fetch: null context");
    if (!cells_dhw) return fail(ctx, MVS_EINVAL, "mvs_sweep_window_fetch: cells_dhw is null");
    if (!ctx->win_planes) return fail(ctx, MVS_ESTATE, "mvs_sweep_window_fetch: no windowed volume yet (mvs_sweep_window first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->win_planes * ctx->W * ctx->H * sizeof(uint32_t);
    MVS_HIP(ctx, hipMemcpyAsync(cells_dhw, ctx->win_vol.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

