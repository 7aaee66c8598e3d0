// aggregate.hip -- semi-global aggregation of the sweep's packed cost volume before depth selection (include/mvs.h
// "mvs_sweep_aggregate", DESIGN.md section 13 holds the arithmetic contract; tests/sgm_mirror.py restates it in numpy, bit for bit).
//
// Everything is exact integer arithmetic on u16 values, so the launch structure below is free to order its work as it likes:
//   agg_cost_kernel      one thread per cell: packed cell -> matching cost C in 1/16 grey levels, capped (rule 1), u16 [D][H][W].
//   agg_rows_kernel      the horizontal paths.  One wavefront per image row; PLANES run across the lanes (lane l owns planes l, l + 64, ...).
//                        Blocks of [D][64 pixels] of C are staged in LDS with coalesced loads (a lane per pixel), then the wave steps
//                        through the block's pixels: the d - 1 / d + 1 terms are lane shuffles, the min over planes is four DPP row
//                        rotations and three scalar mins.  L replaces C in the LDS block and is flushed coalesced.  The wave runs the row
//                        left to right (S = L) and then right to left (S += L): S is zeroed by nobody, the first path stores.
//   agg_columns_kernel   one vertical or diagonal path direction per launch.  A lane owns two neighbouring PATHS (the two halves of a packed
//                        u16 pair), whose column moves by dx per row, so a wave's accesses to one plane stay one contiguous run of pixels;
//                        a path that leaves the image at one side starts again at the other with L = C.  The workgroup's waves split the
//                        planes (DPW per wave), L(p - r, .) lives in registers, the recurrence is packed 16-bit adds and mins, and the
//                        waves exchange their partial minimum and their boundary planes through LDS with one barrier per row.  The next
//                        row's C and S are loaded before the current row is computed.  S += L; the launch owns every cell it touches.
//   agg_select_kernel    a pixel per lane, planes streamed: lowest plane with the smallest S among the seen cells, cost, depth and
//                        (MVS_AGGREGATE_REFINE) the parabola of select_rules.hpp on (float)S.
// No atomics, no scalar memory writes; results do not depend on the launch order (integer sums commute).
#include "sweep_shared.hpp"

namespace mvs {

namespace {

constexpr int kAggMaxPlanes = 256, kAggMaxCap = 4080;
constexpr int kRowPitch = 66;       // u16 per plane row of an LDS block of 64 pixels: 33 dwords, so 64 planes at one pixel hit 64 banks
constexpr int kColMaxWaves = 16;    // waves of a column workgroup (planes / DPW)

typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u16x2 pk(uint32_t v) { return __builtin_bit_cast(u16x2, v); }
__device__ __forceinline__ uint32_t up(u16x2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ u16x2 pk_min(u16x2 a, u16x2 b) { return __builtin_elementwise_min(a, b); }
__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// ---- rule 1: matching cost ----------------------------------------------------------------------------------------------------
template <int CS>
__global__ __launch_bounds__(256) void agg_cost_kernel(const uint32_t *__restrict__ vol, size_t N, uint32_t cap, uint16_t *__restrict__ C)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const uint32_t cell = __builtin_nontemporal_load(vol + i);
    const uint32_t s = cell & ((1u << CS) - 1u), n = cell >> CS;
    uint32_t c = cap;
    if (n) {
        c = CS == CS_FIXED ? (16u * s) / (255u * n) : (16u * s) / n;   // 16 s < 2^28: exact in u32
        c = c < cap ? c : cap;
    }
    C[i] = (uint16_t)c;
}

// ---- horizontal paths ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t row_rotate_min(uint32_t v)
{
    // min over each row of 16 lanes by rotations within the row (every lane ends with its row's minimum)
    v = umin(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false));  // row_ror:1
    v = umin(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false));  // row_ror:2
    v = umin(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false));  // row_ror:4
    v = umin(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false));  // row_ror:8
    return v;
}

__device__ __forceinline__ uint32_t wave_min(uint32_t v)
{
    v = row_rotate_min(v);
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0), b = (uint32_t)__builtin_amdgcn_readlane((int)v, 16);
    const uint32_t c = (uint32_t)__builtin_amdgcn_readlane((int)v, 32), d = (uint32_t)__builtin_amdgcn_readlane((int)v, 48);
    return umin(umin(a, b), umin(c, d));
}

constexpr uint32_t kAbsent = 0x3fffffffu;   // L of a plane >= D: larger than any L, and + P1 cannot wrap

// NP = planes per lane (D <= 64 NP).  One wave per row: blockIdx.x = row.
template <int NP>
__global__ __launch_bounds__(64) void agg_rows_kernel(const uint16_t *__restrict__ C, uint16_t *__restrict__ S, int W, int H, int D, uint32_t P1, uint32_t P2)
{
    extern __shared__ uint16_t lds[];
    uint16_t *blk = lds;   // [D][kRowPitch]: C of the block's pixels on the way in, L (written in place by the lane that read C) on the way out
    const int lane = threadIdx.x, y = blockIdx.x;
    const size_t P = (size_t)W * H, row = (size_t)y * W;
    const int nblocks = (W + 63) / 64;
    for (int dir = 0; dir < 2; dir++) {   // 0: path (0, +1), left to right, stores S.  1: path (0, -1), right to left, adds.
        uint32_t prev[NP];
#pragma unroll
        for (int i = 0; i < NP; i++) prev[i] = lane + 64 * i < D ? 0u : kAbsent;   // all-zero L(p - r, .) gives L = C at the path's first pixel
        uint32_t m = 0u;
        for (int bb = 0; bb < nblocks; bb++) {
            const int b = dir == 0 ? bb : nblocks - 1 - bb;
            const int x0 = b * 64, nb = W - x0 < 64 ? W - x0 : 64;
            if (lane < nb)
                for (int d = 0; d < D; d++) blk[d * kRowPitch + lane] = C[(size_t)d * P + row + x0 + lane];
            __syncthreads();
            for (int xx = 0; xx < nb; xx++) {
                const int x = dir == 0 ? xx : nb - 1 - xx;
                uint32_t cur[NP];
#pragma unroll
                for (int i = 0; i < NP; i++) {
                    const int d = lane + 64 * i;
                    // L(p - r, d - 1): the lane below, or lane 63 of the slot below, or absent (then the own value stands in: + P1 cannot win)
                    uint32_t dn = (uint32_t)__shfl_up((int)prev[i], 1);
                    if (i > 0) {
                        const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)prev[i > 0 ? i - 1 : 0], 63);
                        dn = lane == 0 ? t : dn;
                    }
                    uint32_t upn = (uint32_t)__shfl_down((int)prev[i], 1);
                    if (i + 1 < NP) {
                        const uint32_t t = (uint32_t)__builtin_amdgcn_readlane((int)prev[i + 1 < NP ? i + 1 : i], 0);
                        upn = lane == 63 ? t : upn;
                    }
                    uint32_t best = umin(prev[i], m + P2);
                    best = umin(best, umin(dn, upn) + P1);
                    const uint32_t c = d < D ? (uint32_t)blk[d * kRowPitch + x] : 0u;
                    cur[i] = d < D ? c + best - m : kAbsent;
                    if (d < D) blk[d * kRowPitch + x] = (uint16_t)cur[i];
                }
                uint32_t mm = cur[0];
#pragma unroll
                for (int i = 1; i < NP; i++) mm = umin(mm, cur[i]);
                m = wave_min(mm);
#pragma unroll
                for (int i = 0; i < NP; i++) prev[i] = cur[i];
            }
            __syncthreads();
            if (lane < nb) {
                if (dir == 0)
                    for (int d = 0; d < D; d++) S[(size_t)d * P + row + x0 + lane] = blk[d * kRowPitch + lane];
                else
                    for (int d = 0; d < D; d++) {
                        const size_t a = (size_t)d * P + row + x0 + lane;   // the lane that stored this cell in the first direction
                        S[a] = (uint16_t)(S[a] + blk[d * kRowPitch + lane]);
                    }
            }
            __syncthreads();
        }
    }
}

// ---- vertical and diagonal paths ----------------------------------------------------------------------------------------------
// the lane's pair of neighbouring pixels (x0, x1) of one plane row: one 4-byte access where they are contiguous
__device__ __forceinline__ uint32_t load_pair(const uint16_t *rowp, int x0, int x1, bool v0, bool v1)
{
    uint32_t r = 0u;
    if (v1 && x1 == x0 + 1) {
        __builtin_memcpy(&r, rowp + x0, 4);
    } else if (v0) {
        r = rowp[x0];
        if (v1) r |= (uint32_t)rowp[x1] << 16;
    }
    return r;
}

__device__ __forceinline__ void store_pair(uint16_t *rowp, int x0, int x1, bool v0, bool v1, uint32_t v)
{
    if (v1 && x1 == x0 + 1) {
        __builtin_memcpy(rowp + x0, &v, 4);
    } else if (v0) {
        rowp[x0] = (uint16_t)v;
        if (v1) rowp[x1] = (uint16_t)(v >> 16);
    }
}

// DPW planes per wave; blockDim.x = 64 * ceil(D / DPW); blockIdx.x = group of 128 paths.  Path j is at column (j + dx t) mod W in
// step t, at row t (dy = +1) or H - 1 - t (dy = -1).
template <int DPW>
__global__ __launch_bounds__(64 * kColMaxWaves) void agg_columns_kernel(const uint16_t *__restrict__ C, uint16_t *__restrict__ S, int W, int H, int D, int dy,
                                                                        int dx, uint32_t P1, uint32_t P2)
{
    __shared__ uint32_t xch[2][3][kColMaxWaves][64];   // per row parity: partial minimum, first plane, last plane of every wave
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int d0 = w * DPW, nreal = D - d0 < DPW ? D - d0 : DPW;
    const size_t P = (size_t)W * H;
    const int j0 = blockIdx.x * 128 + 2 * lane;
    const bool v0 = j0 < W, v1 = j0 + 1 < W;
    const u16x2 p1 = pk(P1 * 0x10001u), p2 = pk(P2 * 0x10001u);

    u16x2 prev[DPW], cc[DPW], sc[DPW];
#pragma unroll
    for (int k = 0; k < DPW; k++) prev[k] = cc[k] = sc[k] = pk(0u);
    int x0 = v0 ? j0 : 0, x1 = v1 ? j0 + 1 : 0;
    {
        const size_t r0 = (size_t)(dy > 0 ? 0 : H - 1) * W;
#pragma unroll
        for (int k = 0; k < DPW; k++)
            if (k < nreal) {
                cc[k] = pk(load_pair(C + (size_t)(d0 + k) * P + r0, x0, x1, v0, v1));
                sc[k] = pk(load_pair(S + (size_t)(d0 + k) * P + r0, x0, x1, v0, v1));
            }
    }
    for (int t = 0; t < H; t++) {
        const int y = dy > 0 ? t : H - 1 - t;
        // the next row's columns and cells, in flight while this row is computed
        int nx0 = x0 + dx, nx1 = x1 + dx;
        nx0 = nx0 == W ? 0 : (nx0 < 0 ? W - 1 : nx0);
        nx1 = nx1 == W ? 0 : (nx1 < 0 ? W - 1 : nx1);
        u16x2 cn[DPW], sn[DPW];
#pragma unroll
        for (int k = 0; k < DPW; k++) cn[k] = sn[k] = pk(0u);
        if (t + 1 < H) {
            const size_t rn = (size_t)(y + dy) * W;
#pragma unroll
            for (int k = 0; k < DPW; k++)
                if (k < nreal) {
                    cn[k] = pk(load_pair(C + (size_t)(d0 + k) * P + rn, nx0, nx1, v0, v1));
                    sn[k] = pk(load_pair(S + (size_t)(d0 + k) * P + rn, nx0, nx1, v0, v1));
                }
        }
        // what the other waves know of L(p - r, .): the minimum over all planes and the planes next to this wave's range
        u16x2 m = pk(0u), lo_nb = prev[0], hi_nb = pk(0u);
        if (t > 0) {
            const int par = (t - 1) & 1;
            m = pk(xch[par][0][0][lane]);
            for (int ww = 1; ww < nw; ww++) m = pk_min(m, pk(xch[par][0][ww][lane]));
            if (w > 0) lo_nb = pk(xch[par][2][w - 1][lane]);
            if (w + 1 < nw) hi_nb = pk(xch[par][1][w + 1][lane]);
        }
        // a path whose previous pixel lies outside the image starts here: zero L(p - r, .) makes L = C
        const bool s0 = dx > 0 ? x0 == 0 : (dx < 0 ? x0 == W - 1 : false), s1 = dx > 0 ? x1 == 0 : (dx < 0 ? x1 == W - 1 : false);
        const uint32_t keep = (s0 ? 0u : 0xffffu) | (s1 ? 0u : 0xffff0000u);
        if (__any(keep != 0xffffffffu)) {
#pragma unroll
            for (int k = 0; k < DPW; k++) prev[k] = pk(up(prev[k]) & keep);
            m = pk(up(m) & keep);
            lo_nb = pk(up(lo_nb) & keep);
            hi_nb = pk(up(hi_nb) & keep);
        }
        const u16x2 mp2 = m + p2;
        u16x2 below = w > 0 ? lo_nb : prev[0];   // absent d - 1: the own value stands in (+ P1 cannot win)
        u16x2 part = pk(0xffffffffu), first = pk(0u), last = pk(0u);
        const size_t r = (size_t)y * W;
#pragma unroll
        for (int k = 0; k < DPW; k++)
            if (k < nreal) {
                const u16x2 own = prev[k];
                const u16x2 above = k + 1 < nreal ? prev[k + 1 < DPW ? k + 1 : k] : (w + 1 < nw ? hi_nb : own);
                const u16x2 best = pk_min(pk_min(own, mp2), pk_min(below, above) + p1);
                const u16x2 L = cc[k] + best - m;
                below = own;
                prev[k] = L;
                part = pk_min(part, L);
                if (k == 0) first = L;
                last = L;
                store_pair(S + (size_t)(d0 + k) * P + r, x0, x1, v0, v1, up(sc[k] + L));
            }
        const int par = t & 1;
        xch[par][0][w][lane] = up(part);
        xch[par][1][w][lane] = up(first);
        xch[par][2][w][lane] = up(last);
        __syncthreads();
        x0 = nx0;
        x1 = nx1;
#pragma unroll
        for (int k = 0; k < DPW; k++) {
            cc[k] = cn[k];
            sc[k] = sn[k];
        }
    }
}

// ---- rules 4 and 5: selection ---------------------------------------------------------------------------------------------------
template <int CS>
__global__ __launch_bounds__(256) void agg_select_kernel(const uint16_t *__restrict__ S, const uint32_t *__restrict__ vol, size_t P, int D, const float *__restrict__ z,
                                                         float cost_div, int refine, float *__restrict__ depth, float *__restrict__ cost, int *__restrict__ index)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= P) return;
    uint32_t best = 0xffffffffu;
    int bi = -1;
    constexpr int UNR = 8;
    int d = 0;
    for (; d + UNR <= D; d += UNR) {
        uint32_t s[UNR], c[UNR];
#pragma unroll
        for (int u = 0; u < UNR; u++) {
            s[u] = __builtin_nontemporal_load(S + (size_t)(d + u) * P + p);
            c[u] = __builtin_nontemporal_load(vol + (size_t)(d + u) * P + p);
        }
#pragma unroll
        for (int u = 0; u < UNR; u++)
            if ((c[u] >> CS) != 0u && s[u] < best) {
                best = s[u];
                bi = d + u;
            }
    }
    for (; d < D; d++) {
        const uint32_t s = S[(size_t)d * P + p], c = vol[(size_t)d * P + p];
        if ((c >> CS) != 0u && s < best) {
            best = s;
            bi = d;
        }
    }
    index[p] = bi;
    if (bi < 0) {
        depth[p] = MVS_BACKGROUND_DEPTH;
        cost[p] = __builtin_inff();
        return;
    }
    cost[p] = (float)best / cost_div;
    float zr = z[bi];
    if (refine && bi > 0 && bi < D - 1) {
        const size_t a = (size_t)(bi - 1) * P + p, c = (size_t)(bi + 1) * P + p;
        // the volume's counts say which neighbours are seen; the parabola runs on (float)S in place of the mean costs
        if ((vol[a] >> CS) != 0u && (vol[c] >> CS) != 0u) zr = refine_parabola((float)S[a], (float)best, (float)S[c], z, bi, D);
    }
    depth[p] = zr;
}

template <int NP>
void launch_rows(mvs_ctx *ctx, const uint16_t *C, uint16_t *S, int D, uint32_t p1, uint32_t p2)
{
    const size_t lds = (size_t)D * kRowPitch * sizeof(uint16_t);
    agg_rows_kernel<NP><<<(unsigned)ctx->H, 64, lds, ctx->stream>>>(C, S, ctx->W, ctx->H, D, p1, p2);
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_aggregate(mvs_ctx *ctx, int paths, int p1, int p2, int cost_cap, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_aggregate: null context");
    if (paths != 4 && paths != 8) return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: paths %d is not 4 or 8", paths);
    if (p1 < 0 || p2 < p1) return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: penalties need 0 <= p1 <= p2 (p1 %d, p2 %d)", p1, p2);
    if (cost_cap < 1 || cost_cap > kAggMaxCap) return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: cost_cap %d outside 1..%d", cost_cap, kAggMaxCap);
    if ((long long)paths * ((long long)cost_cap + p2) > 65535)
        return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: paths (cost_cap + p2) = %lld does not fit 16 bits", (long long)paths * ((long long)cost_cap + p2));
    if (flags & ~MVS_AGGREGATE_REFINE) return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: unknown flag bits 0x%x", flags & ~MVS_AGGREGATE_REFINE);
    const uint32_t *vol;
    size_t vol_bytes;
    if (int rc = reader_volume(ctx, "mvs_sweep_aggregate", vol, vol_bytes)) return rc;
    if (!ctx->have_planes || !vol)
        return fail(ctx, MVS_ESTATE, "mvs_sweep_aggregate: no cost volume (run mvs_sweep_run with MVS_SWEEP_VOLUME)");
    const int W = ctx->W, H = ctx->H, D = ctx->D;
    if (D < 2 || D > kAggMaxPlanes) return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: %d planes outside 2..%d", D, kAggMaxPlanes);
    const size_t P = (size_t)W * H, N = P * (size_t)D;
    if (vol_bytes < volume_need(ctx))
        return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate: the volume is %zu bytes, %d planes need %zu", vol_bytes, D, volume_need(ctx));
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure_maps(ctx))) return rc;
    ctx->agg_planes = 0;   // no S until every launch of this call is queued
    if ((rc = ensure(ctx, ctx->agg_sum, N * sizeof(uint16_t)))) return rc;
    if ((rc = ensure(ctx, ctx->agg_cost, N * sizeof(uint16_t)))) return rc;
    uint16_t *C = (uint16_t *)ctx->agg_cost.ptr, *S = (uint16_t *)ctx->agg_sum.ptr;
    ProfileScope ps(ctx, MVS_K_ARGMIN);
    const unsigned cblocks = (unsigned)((N + 255) / 256);
    with_cells(ctx, [&](auto cs) { agg_cost_kernel<decltype(cs)::value><<<cblocks, 256, 0, ctx->stream>>>(vol, N, (uint32_t)cost_cap, C); });
    MVS_HIP(ctx, hipGetLastError());
    // paths (0, +1) and (0, -1): the launch that stores S
    if (D <= 64)
        launch_rows<1>(ctx, C, S, D, (uint32_t)p1, (uint32_t)p2);
    else if (D <= 128)
        launch_rows<2>(ctx, C, S, D, (uint32_t)p1, (uint32_t)p2);
    else
        launch_rows<4>(ctx, C, S, D, (uint32_t)p1, (uint32_t)p2);
    MVS_HIP(ctx, hipGetLastError());
    // paths (+1, 0), (-1, 0) and, with 8 paths, (+1, +1), (-1, -1), (+1, -1), (-1, +1): a launch each, all adding into S
    static const int dirs[6][2] = {{+1, 0}, {-1, 0}, {+1, +1}, {-1, -1}, {+1, -1}, {-1, +1}};
    const unsigned groups = (unsigned)div_up(W, 128);
    for (int r = 0; r < paths - 2; r++) {
        if (D <= 128)
            agg_columns_kernel<8><<<groups, 64 * div_up(D, 8), 0, ctx->stream>>>(C, S, W, H, D, dirs[r][0], dirs[r][1], (uint32_t)p1, (uint32_t)p2);
        else
            agg_columns_kernel<16><<<groups, 64 * div_up(D, 16), 0, ctx->stream>>>(C, S, W, H, D, dirs[r][0], dirs[r][1], (uint32_t)p1, (uint32_t)p2);
        MVS_HIP(ctx, hipGetLastError());
    }
    const float cost_div = (float)(16 * paths);
    const int refine = (flags & MVS_AGGREGATE_REFINE) ? 1 : 0;
    const unsigned sblocks = (unsigned)((P + 255) / 256);
    with_cells(ctx, [&](auto cs) {
        agg_select_kernel<decltype(cs)::value><<<sblocks, 256, 0, ctx->stream>>>(S, vol, P, D, (const float *)ctx->ztab.ptr, cost_div, refine, (float *)ctx->depth.ptr,
                                                                                 (float *)ctx->cost.ptr, (int *)ctx->index.ptr);
    });
    MVS_HIP(ctx, hipGetLastError());
    ctx->agg_planes = D;
    note_full_selection(ctx);
    return MVS_OK;
}

void *mvs_sweep_aggregated_device(mvs_ctx *ctx, size_t *bytes)
{
    if (bytes) *bytes = 0;
    if (!ctx || !ctx->agg_planes) return nullptr;
    if (bytes) *bytes = (size_t)ctx->agg_planes * ctx->W * ctx->H * sizeof(uint16_t);
    return ctx->agg_sum.ptr;
}

int mvs_sweep_aggregate_fetch(mvs_ctx *ctx, uint16_t *s_dhw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_aggregate_fetch: null context");
    if (!ctx->agg_planes) return fail(ctx, MVS_ESTATE, "mvs_sweep_aggregate_fetch: nothing aggregated yet (mvs_sweep_aggregate first)");
    if (!s_dhw) return fail(ctx, MVS_EINVAL, "mvs_sweep_aggregate_fetch: s_dhw is null");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->agg_planes * ctx->W * ctx->H * sizeof(uint16_t);
    MVS_HIP(ctx, hipMemcpyAsync(s_dhw, ctx->agg_sum.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}
