// clean.hip -- rejection of unreliable pixels of the selected depth / cost / index maps (include/mvs.h "mvs_sweep_clean", DESIGN.md
// section 16 holds the contract; tests/clean_mirror.py restates it in numpy).  Integer arithmetic only, so nothing below depends on
// the order in which the hardware runs it.
//   clean_rules_kernel   rules 1 and 2, a pixel per lane, the D planes of the volume (and of S) streamed plane-major like
//                        agg_select_kernel.  Both rules read the incoming maps and the decision of a pixel depends on that pixel
//                        alone, so the maps are rewritten in place.  Skipped when both rules are off (clean_count_kernel counts then).
//   rule 3, connected components of the index map, in a number of launches that depends on nothing:
//   clean_tile_kernel    one workgroup per 64 x 16 tile: union-find over the tile's pixels in LDS (link by atomicMin of the larger
//                        root onto the smaller), flattened, written out as the image-wide pixel number of the tile-local root.
//   clean_merge_kernel   a thread per pixel pair that straddles a tile border: the same lock-free union-find on the label array in
//                        global memory.  Labels only decrease, nobody waits for anybody.  Every access to the labels in this launch
//                        is an agent-scope atomic (the XCDs' L2s are private: a plain load may return a stale line, and the union
//                        it then skips is a component counted in two halves).  find() halves the paths it walks with a
//                        compare-and-swap: the replaced link x -> p goes to p's own parent, so no connection is lost.
//   clean_roots_kernel   a new launch, plain loads: every pixel's root, and the components' sizes by integer atomicAdd onto the root's
//                        counter (runs of equal roots inside a wavefront are added once).
//   clean_apply_kernel   sizes spread from the roots to their pixels, pixels of small components rejected and counted.
// The counters and the size array are zeroed on the stream by every call.  No scalar memory writes.
#include "sweep_shared.hpp"

namespace mvs {

namespace {

constexpr int kTileW = 64, kTileH = 16, kTilePixels = kTileW * kTileH;   // 256 threads, 4 pixels each
constexpr int kValid = 0, kRule1 = 1, kRule2 = 2, kRule3 = 3;             // the counters, in the order of mvs_sweep_clean_report

__device__ __forceinline__ void count_lanes(unsigned *counter, bool mine)
{
    const unsigned long long m = __ballot(mine);
    if (m != 0ull && (threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned)__popcll(m));
}

__device__ __forceinline__ void reject_pixel(size_t p, float *depth, float *cost, int *index)
{
    index[p] = -1;
    depth[p] = MVS_BACKGROUND_DEPTH;
    cost[p] = __builtin_inff();
}

// ---- rules 1 and 2 ----------------------------------------------------------------------------------------------------------------
// rival test of rule 2 for plane d: the cell `c` (and its sum `s` of S with AGG) against the winner's terms
template <int CS, bool AGG>
__device__ __forceinline__ bool rival(uint32_t c, uint32_t s, uint32_t win32, uint64_t a64, uint64_t b64, uint32_t hundred_minus_u)
{
    const uint32_t n = c >> CS;
    if (n == 0u) return false;
    if (AGG) return s * hundred_minus_u < win32;                                  // S(d) (100 - u) < S(i) 100: at most 65535 * 100
    return (uint64_t)(c & ((1u << CS) - 1u)) * a64 < b64 * (uint64_t)n;           // s_d n_i (100 - u) < s_i n_d 100: below 2^48
}

template <int CS, bool AGG>
__global__ __launch_bounds__(256) void clean_rules_kernel(const uint16_t *__restrict__ S, const uint32_t *__restrict__ vol, size_t P, int D, int rule1,
                                                          uint32_t min_views, uint32_t u, float *__restrict__ depth, float *__restrict__ cost,
                                                          int *__restrict__ index, unsigned *__restrict__ counters)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = p < P ? index[p] : -1;
    const bool valid = i >= 0;
    bool r1 = false, r2 = false;
    if (valid && i < D) {   // (an index of an earlier, larger plane count has no cell to test)
        const uint32_t ci = vol[(size_t)i * P + p];
        const uint32_t ni = ci >> CS, si = ci & ((1u << CS) - 1u);
        r1 = rule1 && ni < min_views;
        if (!r1 && u != 0u) {
            const uint32_t hmu = 100u - u;
            const uint32_t win32 = AGG ? 100u * (uint32_t)S[(size_t)i * P + p] : 0u;
            const uint64_t a64 = (uint64_t)ni * hmu, b64 = (uint64_t)si * 100u;
            constexpr int UNR = 8;
            int d = 0;
            for (; d + UNR <= D; d += UNR) {
                uint32_t s[UNR], c[UNR];
#pragma unroll
                for (int k = 0; k < UNR; k++) {
                    s[k] = AGG ? (uint32_t)__builtin_nontemporal_load(S + (size_t)(d + k) * P + p) : 0u;
                    c[k] = __builtin_nontemporal_load(vol + (size_t)(d + k) * P + p);
                }
#pragma unroll
                for (int k = 0; k < UNR; k++) {
                    const int away = d + k - i;
                    if ((away >= 2 || away <= -2) && rival<CS, AGG>(c[k], s[k], win32, a64, b64, hmu)) r2 = true;
                }
            }
            for (; d < D; d++) {
                const uint32_t s = AGG ? (uint32_t)S[(size_t)d * P + p] : 0u, c = vol[(size_t)d * P + p];
                const int away = d - i;
                if ((away >= 2 || away <= -2) && rival<CS, AGG>(c, s, win32, a64, b64, hmu)) r2 = true;
            }
        }
        if (r1 || r2) reject_pixel(p, depth, cost, index);
    }
    count_lanes(counters + kValid, valid);
    count_lanes(counters + kRule1, r1);
    count_lanes(counters + kRule2, r2);
}

__global__ __launch_bounds__(256) void clean_count_kernel(const int *__restrict__ index, size_t P, unsigned *__restrict__ counters)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    count_lanes(counters + kValid, p < P && index[p] >= 0);
}

// ---- rule 3 -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool connected(int a, int b, int max_diff)
{
    const int d = a > b ? a - b : b - a;
    return a >= 0 && b >= 0 && d <= max_diff;
}

// union-find on labels in LDS, shared by one workgroup
__device__ __forceinline__ int lds_load(int *lab, int x) { return __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(int *lab, int x)
{
    for (int p = lds_load(lab, x); p != x; p = lds_load(lab, x)) x = p;
    return x;
}

__device__ __forceinline__ void lds_union(int *lab, int a, int b)
{
    for (;;) {
        a = lds_find(lab, a);
        b = lds_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        // a > b.  Whatever a pointed to (itself, if it still was a root) now points no higher than b; what it pointed to before is joined next.
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (old == a) return;
        a = old;
    }
}

__global__ __launch_bounds__(256) void clean_tile_kernel(const int *__restrict__ index, int W, int H, int max_diff, int *__restrict__ labels)
{
    __shared__ int idx[kTilePixels], lab[kTilePixels];
    const int t = threadIdx.x, lx = t & (kTileW - 1), ly0 = t >> 6;   // pixels (lx, ly0 + 4 k), k = 0..3
    const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
    const int x = x0 + lx;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ly0 + 4 * k, y = y0 + ly, l = ly * kTileW + lx;
        idx[l] = x < W && y < H ? index[(size_t)y * W + x] : -1;
        lab[l] = l;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ly0 + 4 * k, l = ly * kTileW + lx;
        const int me = idx[l];
        if (lx > 0 && connected(me, idx[l - 1], max_diff)) lds_union(lab, l, l - 1);
        if (ly > 0 && connected(me, idx[l - kTileW], max_diff)) lds_union(lab, l, l - kTileW);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ly = ly0 + 4 * k, y = y0 + ly, l = ly * kTileW + lx;
        if (x < W && y < H) {
            const int r = lds_find(lab, l);
            labels[(size_t)y * W + x] = idx[l] >= 0 ? (y0 + (r >> 6)) * W + x0 + (r & (kTileW - 1)) : -1;
        }
    }
}

// union-find on the label array in global memory, shared by the whole grid: agent-scope atomics only
__device__ __forceinline__ int g_load(int *lab, int x) { return __hip_atomic_load(lab + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(int *lab, int x)
{
    int p = g_load(lab, x);
    while (p != x) {
        const int g = g_load(lab, p);
        // path halving: x -> p becomes x -> g only if it still is x -> p (p keeps its own way up, so x loses no connection)
        if (g != p) {
            int expect = p;
            __hip_atomic_compare_exchange_strong(lab + x, &expect, g, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        x = p;
        p = g;
    }
    return x;
}

__device__ __forceinline__ void g_union(int *lab, int a, int b)
{
    for (;;) {
        a = g_find(lab, a);
        b = g_find(lab, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == a) return;
        a = old;   // a had been linked meanwhile: its former parent and b are joined next (labels only decrease: this ends)
    }
}

// pairs across the vertical tile borders first ((ntx - 1) per image row), then across the horizontal ones (W per border)
__global__ __launch_bounds__(256) void clean_merge_kernel(const int *__restrict__ index, int W, int H, int max_diff, int *labels)
{
    const int ntx = (W + kTileW - 1) / kTileW, nty = (H + kTileH - 1) / kTileH;
    const size_t nv = (size_t)(ntx - 1) * H, nh = (size_t)(nty - 1) * W;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nv + nh) return;
    size_t a, b;   // b is the left / upper pixel
    if (t < nv) {
        const int y = (int)(t / (size_t)(ntx - 1)), x = kTileW * ((int)(t % (size_t)(ntx - 1)) + 1);
        a = (size_t)y * W + x;
        b = a - 1;
    } else {
        const size_t s = t - nv;
        const int y = kTileH * ((int)(s / (size_t)W) + 1), x = (int)(s % (size_t)W);
        a = (size_t)y * W + x;
        b = a - W;
    }
    if (connected(index[a], index[b], max_diff)) g_union(labels, (int)a, (int)b);
}

__global__ __launch_bounds__(256) void clean_roots_kernel(const int *__restrict__ labels, size_t P, int *__restrict__ roots, int *__restrict__ sizes)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int r = -1;
    if (p < P) {
        r = labels[p];
        if (r >= 0)
            for (int n = labels[r]; n != r; n = labels[r]) r = n;
        roots[p] = r;
    }
    // one add per run of equal roots in the wavefront (the lanes are neighbours in a row, so a run is the rule)
    const int lane = threadIdx.x & 63;
    const int before = __shfl_up(r, 1);
    const unsigned long long heads = __ballot(lane == 0 || before != r);
    if ((heads >> lane) & 1ull) {
        const unsigned long long later = lane == 63 ? 0ull : heads >> (lane + 1);
        const int run = later ? __ffsll((long long)later) : 64 - lane;
        if (r >= 0) atomicAdd(sizes + r, run);
    }
}

__global__ __launch_bounds__(256) void clean_apply_kernel(const int *__restrict__ roots, size_t P, int min_size, int *sizes, float *__restrict__ depth,
                                                          float *__restrict__ cost, int *__restrict__ index, unsigned *__restrict__ counters)
{
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool r3 = false;
    if (p < P) {
        const int r = roots[p];
        if (r >= 0) {
            const int size = sizes[r];          // only roots' entries are read in this launch ...
            if ((size_t)r != p) sizes[p] = size;   // ... and only the others' are written
            r3 = size < min_size;
            if (r3) reject_pixel(p, depth, cost, index);
        }
    }
    count_lanes(counters + kRule3, r3);
}

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_sweep_clean(mvs_ctx *ctx, int min_views, int uniqueness_percent, int speckle_min_size, int speckle_max_diff, unsigned flags)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_clean: null context");
    if (min_views < 0 || min_views > 255) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean: min_views %d outside 0..255", min_views);
    if (uniqueness_percent < 0 || uniqueness_percent > 99)
        return fail(ctx, MVS_EINVAL, "mvs_sweep_clean: uniqueness_percent %d outside 0..99", uniqueness_percent);
    if (speckle_min_size < 0) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean: speckle_min_size %d is negative", speckle_min_size);
    if (speckle_max_diff < 0 || speckle_max_diff > 255) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean: speckle_max_diff %d outside 0..255", speckle_max_diff);
    if (flags & ~MVS_CLEAN_SCORES_AGGREGATED) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean: unknown flag bits 0x%x", flags & ~MVS_CLEAN_SCORES_AGGREGATED);
    if (!ctx->index.ptr || !ctx->depth.ptr || !ctx->cost.ptr || !ctx->sel_planes)
        return fail(ctx, MVS_ESTATE, "mvs_sweep_clean: no depth selection yet (mvs_sweep_run with MVS_SWEEP_FUSED_ARGMIN, mvs_sweep_argmin or mvs_sweep_aggregate)");
    const int W = ctx->W, H = ctx->H, D = ctx->D;
    if (!selection_current(ctx))   // rules 1 and 2 read the volume (and S) at the selected plane
        return fail(ctx, MVS_ESTATE, "mvs_sweep_clean: the depth selection was made over %d planes, the context now has %d (select again)", ctx->sel_planes, D);
    const size_t P = (size_t)W * H;
    if (P > (size_t)INT_MAX) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean: %zu pixels do not fit the 32-bit labels", P);
    const bool agg = (flags & MVS_CLEAN_SCORES_AGGREGATED) != 0;
    const uint32_t *vol;
    size_t vol_bytes;
    if (int rc = reader_volume(ctx, "mvs_sweep_clean", vol, vol_bytes)) return rc;
    const bool have_volume = volume_holds_planes(ctx, vol, vol_bytes);
    // min_views 1 rejects a selected cell that no view sees; the library selects none, so without a volume there is nothing to test
    const bool rule1 = min_views >= 2 || (min_views == 1 && have_volume), rule2 = uniqueness_percent > 0, rule3 = speckle_min_size > 0;
    if ((rule1 || rule2) && !have_volume)
        return fail(ctx, MVS_ESTATE, "mvs_sweep_clean: min_views >= 2 and uniqueness need the packed volume of %d x %d x %d cells (mvs_sweep_run with MVS_SWEEP_VOLUME)", D,
                    H, W);
    if (agg && (ctx->agg_planes != D || !ctx->agg_sum.ptr))
        return fail(ctx, MVS_ESTATE, "mvs_sweep_clean: MVS_CLEAN_SCORES_AGGREGATED without sums of the current %d planes (mvs_sweep_aggregate first)", D);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure(ctx, ctx->clean_counters, 4 * sizeof(unsigned)))) return rc;
    if (rule3) {
        if ((rc = ensure(ctx, ctx->clean_labels, 2 * P * sizeof(int)))) return rc;   // labels, then roots
        if ((rc = ensure(ctx, ctx->clean_sizes, P * sizeof(int)))) return rc;
    }
    // from here on only launches: the maps change, and the report and the sizes are those of this call
    ctx->clean_have_sizes = false;
    ctx->clean_done = false;
    unsigned *counters = (unsigned *)ctx->clean_counters.ptr;
    float *depth = (float *)ctx->depth.ptr, *cost = (float *)ctx->cost.ptr;
    int *index = (int *)ctx->index.ptr;
    const unsigned pblocks = (unsigned)((P + 255) / 256);
    ProfileScope ps(ctx, MVS_K_ARGMIN);
    MVS_HIP(ctx, hipMemsetAsync(counters, 0, 4 * sizeof(unsigned), ctx->stream));
    if (rule1 || rule2) {
        const uint16_t *S = (const uint16_t *)ctx->agg_sum.ptr;
        const uint32_t mv = (uint32_t)min_views, u = (uint32_t)uniqueness_percent;
        with_cells(ctx, [&](auto cs) {
            constexpr int CS = decltype(cs)::value;
            if (agg)
                clean_rules_kernel<CS, true><<<pblocks, 256, 0, ctx->stream>>>(S, vol, P, D, rule1, mv, u, depth, cost, index, counters);
            else
                clean_rules_kernel<CS, false><<<pblocks, 256, 0, ctx->stream>>>(nullptr, vol, P, D, rule1, mv, u, depth, cost, index, counters);
        });
    } else {
        clean_count_kernel<<<pblocks, 256, 0, ctx->stream>>>(index, P, counters);
    }
    MVS_HIP(ctx, hipGetLastError());
    if (rule3) {
        int *labels = (int *)ctx->clean_labels.ptr, *roots = labels + P, *sizes = (int *)ctx->clean_sizes.ptr;
        const int ntx = div_up(W, kTileW), nty = div_up(H, kTileH);
        MVS_HIP(ctx, hipMemsetAsync(sizes, 0, P * sizeof(int), ctx->stream));
        clean_tile_kernel<<<dim3((unsigned)ntx, (unsigned)nty), 256, 0, ctx->stream>>>(index, W, H, speckle_max_diff, labels);
        MVS_HIP(ctx, hipGetLastError());
        const size_t pairs = (size_t)(ntx - 1) * H + (size_t)(nty - 1) * W;
        if (pairs) {
            clean_merge_kernel<<<(unsigned)((pairs + 255) / 256), 256, 0, ctx->stream>>>(index, W, H, speckle_max_diff, labels);
            MVS_HIP(ctx, hipGetLastError());
        }
        clean_roots_kernel<<<pblocks, 256, 0, ctx->stream>>>(labels, P, roots, sizes);
        MVS_HIP(ctx, hipGetLastError());
        clean_apply_kernel<<<pblocks, 256, 0, ctx->stream>>>(roots, P, speckle_min_size, sizes, depth, cost, index, counters);
        MVS_HIP(ctx, hipGetLastError());
        ctx->clean_have_sizes = true;
    }
    ctx->clean_done = true;
    return MVS_OK;
}

int mvs_sweep_clean_report(mvs_ctx *ctx, int out[4])
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_clean_report: null context");
    if (!out) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean_report: out is null");
    if (!ctx->clean_done) return fail(ctx, MVS_ESTATE, "mvs_sweep_clean_report: nothing cleaned yet (mvs_sweep_clean first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    unsigned h[4] = {0u, 0u, 0u, 0u};
    MVS_HIP(ctx, hipMemcpyAsync(h, ctx->clean_counters.ptr, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++) out[k] = (int)h[k];
    return MVS_OK;
}

void *mvs_sweep_clean_sizes_device(mvs_ctx *ctx) { return ctx && ctx->clean_have_sizes ? ctx->clean_sizes.ptr : nullptr; }

int mvs_sweep_clean_sizes_fetch(mvs_ctx *ctx, int32_t *sizes_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_sweep_clean_sizes_fetch: null context");
    if (!sizes_hw) return fail(ctx, MVS_EINVAL, "mvs_sweep_clean_sizes_fetch: sizes_hw is null");
    if (!ctx->clean_have_sizes) return fail(ctx, MVS_ESTATE, "mvs_sweep_clean_sizes_fetch: the last mvs_sweep_clean ran no speckle filter (speckle_min_size > 0)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(sizes_hw, ctx->clean_sizes.ptr, (size_t)ctx->W * ctx->H * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}
