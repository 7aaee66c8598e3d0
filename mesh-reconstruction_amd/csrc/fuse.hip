// fuse.hip -- depth-map fusion (include/mvs.h "depth store + fusion").
//
// The depth store keeps depth maps (main-camera NDC z, 1.0 = empty) with their best costs and cameras in HBM; mvs_fuse_depth back-projects one
// stored map, keeps the pixels that enough of the listed neighbour maps agree with, averages the agreeing points, takes a normal from the
// reference map's own 4-neighbours and writes (x, y, z, 1, nx, ny, nz) rows in ascending pixel index.
//
// One thread per reference pixel, 64 x 4 tiles of 256 threads: each wave is one 64-pixel run of one image row (a "segment" of the
// row-major order), so a wave's gathers from a neighbour map land on a few neighbouring lines and a ballot gives the wave's keep mask in
// pixel order.  Order-preserving compaction in three launches: fuse_count_kernel writes one keep count per segment, rocprim's exclusive
// scan turns them into row offsets, fuse_rows_kernel recomputes the same pixels and writes the rows at those offsets.  Every launch is a
// pure function of the inputs: the rows are the same from run to run.
//
// Arithmetic: f32, one rounding per operation, no contraction (the library builds with -ffp-contract=off; the pixel centres' fmaf is the
// sweep's and is written out); tests/fuse_mirror.py restates it in numpy.
#include "depth_rules.hpp"
#include "mvs_internal.hpp"

#include <rocprim/rocprim.hpp>

#include <cmath>

namespace mvs {

namespace {

constexpr int kFuseMaxNeighbours = 16;
constexpr int kFuseTX = 64, kFuseTY = 4;  // tile = 4 wave-wide rows

// Everything the kernels read besides the maps: passed by value, so the matrices sit in the kernel-argument segment and every lane reads
// them with the same (scalar) loads.  Index 0 is the reference view, 1..K the neighbours in the caller's order.
struct FuseArgs {
    const float *depth[kFuseMaxNeighbours + 1];
    const float *cost[kFuseMaxNeighbours + 1];  // null unless the cost threshold is finite
    float P[kFuseMaxNeighbours + 1][16];
    float Pi[kFuseMaxNeighbours + 1][16];
    float C[3];                                 // reference camera centre
    int W, H, K, min_consistent, ntx, use_cost;
    float invW, invH, halfW, halfH, max_reproj2, max_rel, max_cost;
};

// (x, y, z, w_r) of reference pixel (r, c); w = 0 marks a pixel that is not valid (rule 1, or w_r <= 0)
__device__ __forceinline__ float4 ref_point(const FuseArgs &a, int r, int c)
{
    const size_t p = (size_t)r * a.W + c;
    const float z = a.depth[0][p];
    if (!depth_valid(z, a.cost[0], p, a.use_cost, a.max_cost)) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float xn = __builtin_fmaf((float)(2 * c + 1), a.invW, -1.0f);
    const float yn = __builtin_fmaf(-(float)(2 * r + 1), a.invH, 1.0f);
    const float3 X = unproject(a.Pi[0], xn, yn, z);
    const float w = prow(a.P[0], 3, X);
    if (!(w > 0.f)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(X.x, X.y, X.z, w);
}

__device__ __forceinline__ bool same_surface(float4 n, float w, float max_rel) { return n.w > 0.f && fabsf(n.w - w) / w <= max_rel; }

// tangent from the two neighbours along one axis: central difference, else one-sided, else none
__device__ __forceinline__ bool tangent(float4 lo, float4 c, float4 hi, float max_rel, float3 &t)
{
    const bool ul = same_surface(lo, c.w, max_rel), uh = same_surface(hi, c.w, max_rel);
    if (ul && uh) t = make_float3(hi.x - lo.x, hi.y - lo.y, hi.z - lo.z);
    else if (uh) t = make_float3(hi.x - c.x, hi.y - c.y, hi.z - c.z);
    else if (ul) t = make_float3(c.x - lo.x, c.y - lo.y, c.z - lo.z);
    else return false;
    return true;
}

// the whole per-pixel contract; tile holds ref_point of the tile plus a one-pixel halo, (ty, tx) is this pixel's entry
__device__ __forceinline__ bool fuse_pixel(const FuseArgs &a, const float4 (*tile)[kFuseTX + 2], int ty, int tx, int row, int col, float out[7])
{
    const float4 c = tile[ty][tx];
    if (!(c.w > 0.f)) return false;
    // normal from the reference map alone (before the votes: a pixel without one is dropped anyway)
    float3 tc, tr;
    if (!tangent(tile[ty][tx - 1], c, tile[ty][tx + 1], a.max_rel, tc)) return false;
    if (!tangent(tile[ty - 1][tx], c, tile[ty + 1][tx], a.max_rel, tr)) return false;
    float nx = tc.y * tr.z - tc.z * tr.y;
    float ny = tc.z * tr.x - tc.x * tr.z;
    float nz = tc.x * tr.y - tc.y * tr.x;
    const float len = sqrtf((nx * nx + ny * ny) + nz * nz);
    if (!(len > 0.f && len < INFINITY)) return false;
    nx = nx / len;
    ny = ny / len;
    nz = nz / len;
    if ((nx * (a.C[0] - c.x) + ny * (a.C[1] - c.y)) + nz * (a.C[2] - c.z) < 0.f) {
        nx = -nx;
        ny = -ny;
        nz = -nz;
    }
    // votes of the neighbours, in the listed order
    const float3 X = make_float3(c.x, c.y, c.z);
    float sx = c.x, sy = c.y, sz = c.z;
    int agree = 0;
    for (int j = 1; j <= a.K; j++) {
        const float qw = prow(a.P[j], 3, X);
        if (!(qw > 0.f)) continue;
        const float u = (prow(a.P[j], 0, X) / qw + 1.0f) * a.halfW - 0.5f;
        const float v = (1.0f - prow(a.P[j], 1, X) / qw) * a.halfH - 0.5f;
        const float fc = floorf(u + 0.5f), fr = floorf(v + 0.5f);
        if (!(fc >= 0.f && fc < (float)a.W && fr >= 0.f && fr < (float)a.H)) continue;
        const int cj = (int)fc, rj = (int)fr;
        const size_t p = (size_t)rj * a.W + cj;
        const float zj = a.depth[j][p];
        if (!depth_valid(zj, a.cost[j], p, a.use_cost, a.max_cost)) continue;
        const float xn = __builtin_fmaf((float)(2 * cj + 1), a.invW, -1.0f);
        const float yn = __builtin_fmaf(-(float)(2 * rj + 1), a.invH, 1.0f);
        const float3 Xj = unproject(a.Pi[j], xn, yn, zj);
        const float sw = prow(a.P[0], 3, Xj);
        if (!(sw > 0.f)) continue;
        const float ur = (prow(a.P[0], 0, Xj) / sw + 1.0f) * a.halfW - 0.5f;
        const float vr = (1.0f - prow(a.P[0], 1, Xj) / sw) * a.halfH - 0.5f;
        const float du = ur - (float)col, dv = vr - (float)row;
        if (!(du * du + dv * dv <= a.max_reproj2)) continue;
        if (!(fabsf(sw - c.w) / c.w <= a.max_rel)) continue;
        sx = sx + Xj.x;
        sy = sy + Xj.y;
        sz = sz + Xj.z;
        agree++;
    }
    if (agree < a.min_consistent) return false;
    const float n = (float)(agree + 1);
    out[0] = sx / n;
    out[1] = sy / n;
    out[2] = sz / n;
    out[3] = 1.0f;
    out[4] = nx;
    out[5] = ny;
    out[6] = nz;
    return true;
}

// WRITE = false: keep count per segment (row * ntx + tile column) and counts[H * ntx] = 0; WRITE = true: rows at the scanned offsets
template <bool WRITE>
__device__ __forceinline__ void fuse_body(const FuseArgs &a, int *__restrict__ counts, const int *__restrict__ offsets, float *__restrict__ rows)
{
    __shared__ float4 tile[kFuseTY + 2][kFuseTX + 2];
    const int tx = threadIdx.x & (kFuseTX - 1), ty = threadIdx.x / kFuseTX;
    const int col0 = blockIdx.x * kFuseTX, row0 = blockIdx.y * kFuseTY;
    for (int e = threadIdx.x; e < (kFuseTY + 2) * (kFuseTX + 2); e += kFuseTX * kFuseTY) {
        const int er = e / (kFuseTX + 2), ec = e - er * (kFuseTX + 2);
        const int r = row0 + er - 1, c = col0 + ec - 1;
        tile[er][ec] = (r >= 0 && r < a.H && c >= 0 && c < a.W) ? ref_point(a, r, c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
    const int row = row0 + ty, col = col0 + tx;
    float out[7];
    const bool keep = row < a.H && col < a.W && fuse_pixel(a, tile, ty + 1, tx + 1, row, col, out);
    const unsigned long long m = __ballot(keep);
    const int seg = row * a.ntx + blockIdx.x;
    if (!WRITE) {
        if (tx == 0 && row < a.H) counts[seg] = __popcll(m);
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) counts[a.H * a.ntx] = 0;
    } else if (keep) {
        float *dst = rows + 7 * (size_t)(offsets[seg] + __popcll(m & ((1ull << tx) - 1ull)));
        for (int k = 0; k < 7; k++) dst[k] = out[k];
    }
}

__global__ __launch_bounds__(256) void fuse_count_kernel(const FuseArgs a, int *__restrict__ counts) { fuse_body<false>(a, counts, nullptr, nullptr); }
__global__ __launch_bounds__(256) void fuse_rows_kernel(const FuseArgs a, const int *__restrict__ offsets, float *__restrict__ rows)
{
    fuse_body<true>(a, nullptr, offsets, rows);
}

}  // namespace

// P^-1 by invert4 in double, rounded once; C = null vector of rows x, y, w of P (the signed 3 x 3 minors, as extractCameraCenter takes
// it), dehomogenised in double and rounded once.  (Declared in mvs_internal.hpp: mvs_tsdf_raycast derives its camera the same way.)
bool slot_matrices(const float cam[16], mvs_ctx::DepthSlot &s)
{
    double m[16], mi[16];
    for (int i = 0; i < 16; i++) {
        if (!std::isfinite(cam[i])) return false;
        m[i] = cam[i];
        s.P[i] = cam[i];
    }
    invert4(m, mi);
    for (int i = 0; i < 16; i++) {
        if (!std::isfinite(mi[i])) return false;
        s.Pi[i] = (float)mi[i];
    }
    const int rows[3] = {0, 1, 3};
    double p[3][4];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++) p[r][c] = m[4 * rows[r] + c];
    auto det3 = [&](int c0, int c1, int c2) {
        return p[0][c0] * (p[1][c1] * p[2][c2] - p[1][c2] * p[2][c1]) - p[0][c1] * (p[1][c0] * p[2][c2] - p[1][c2] * p[2][c0]) +
               p[0][c2] * (p[1][c0] * p[2][c1] - p[1][c1] * p[2][c0]);
    };
    const double h[4] = {det3(1, 2, 3), -det3(0, 2, 3), det3(0, 1, 3), -det3(0, 1, 2)};
    if (h[3] == 0.0) return false;  // no finite centre
    for (int i = 0; i < 3; i++) s.C[i] = (float)(h[i] / h[3]);
    s.C[3] = 1.0f;
    return true;
}

namespace {

int depth_upload_impl(mvs_ctx *ctx, int slot, const float cam[16], const float *depth, const float *cost, bool device)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_upload: null context");
    if (!cam || !depth) return fail(ctx, MVS_EINVAL, "mvs_depth_upload: null argument");
    if (slot < 0 || slot >= (int)ctx->dstore.size())
        return fail(ctx, MVS_EINVAL, "mvs_depth_upload: slot %d outside the depth store (capacity %d: mvs_depth_store first)", slot, (int)ctx->dstore.size());
    mvs_ctx::DepthSlot s;
    if (!slot_matrices(cam, s)) return fail(ctx, MVS_EINVAL, "mvs_depth_upload: camera of slot %d is singular or has no finite centre", slot);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    ctx->dstore[slot].have = false;
    MVS_HIP(ctx, hipMemcpyAsync((float *)ctx->dstore_depth.ptr + P * slot, depth, P * sizeof(float), kind, ctx->stream));
    if (cost) MVS_HIP(ctx, hipMemcpyAsync((float *)ctx->dstore_cost.ptr + P * slot, cost, P * sizeof(float), kind, ctx->stream));
    s.have = true;
    s.have_cost = cost != nullptr;
    ctx->dstore[slot] = s;
    return MVS_OK;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_depth_store(mvs_ctx *ctx, int capacity)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_store: null context");
    if (capacity < 1 || capacity > 8191) return fail(ctx, MVS_EINVAL, "mvs_depth_store: capacity %d out of range 1..8191", capacity);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->W * ctx->H * sizeof(float) * capacity;
    ctx->dstore.clear();  // empty until both buffers have their new size (ensure frees before it allocates)
    int rc;
    if ((rc = ensure(ctx, ctx->dstore_depth, bytes))) return rc;
    if ((rc = ensure(ctx, ctx->dstore_cost, bytes))) return rc;
    ctx->dstore.assign((size_t)capacity, mvs_ctx::DepthSlot());
    return MVS_OK;
}

int mvs_depth_upload(mvs_ctx *ctx, int slot, const float cam[16], const float *depth_hw, const float *cost_hw)
{
    return depth_upload_impl(ctx, slot, cam, depth_hw, cost_hw, false);
}

int mvs_depth_upload_device(mvs_ctx *ctx, int slot, const float cam[16], const void *depth_dev, const void *cost_dev)
{
    return depth_upload_impl(ctx, slot, cam, (const float *)depth_dev, (const float *)cost_dev, true);
}

int mvs_depth_slot_matrices(const mvs_ctx *ctx, int slot, float out[36])
{
    if (!ctx || !out) return fail(nullptr, MVS_EINVAL, "mvs_depth_slot_matrices: null argument");
    mvs_ctx *c = const_cast<mvs_ctx *>(ctx);  // (error text only)
    if (slot < 0 || slot >= (int)ctx->dstore.size()) return fail(c, MVS_EINVAL, "mvs_depth_slot_matrices: slot %d outside the depth store", slot);
    const mvs_ctx::DepthSlot &s = ctx->dstore[slot];
    if (!s.have) return fail(c, MVS_ESTATE, "mvs_depth_slot_matrices: slot %d holds no depth map", slot);
    memcpy(out, s.P, sizeof(s.P));
    memcpy(out + 16, s.Pi, sizeof(s.Pi));
    memcpy(out + 32, s.C, sizeof(s.C));
    return MVS_OK;
}

void *mvs_depth_slot_device(mvs_ctx *ctx, int slot)
{
    if (!ctx || slot < 0 || slot >= (int)ctx->dstore.size() || !ctx->dstore[slot].have) return nullptr;
    return (float *)ctx->dstore_depth.ptr + (size_t)ctx->W * ctx->H * slot;
}

int mvs_fuse_depth(mvs_ctx *ctx, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px, float max_rel_depth,
                   float max_cost, float *out_points7, int *out_count)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_fuse_depth: null context");
    if (!out_count) return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: out_count is null");
    *out_count = 0;
    const int cap = (int)ctx->dstore.size();
    if (nneighbours < 0 || nneighbours > kFuseMaxNeighbours) return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: nneighbours %d out of range 0..%d", nneighbours, kFuseMaxNeighbours);
    if (nneighbours > 0 && !neighbour_slots) return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: neighbour_slots is null");
    if (min_consistent < 0 || min_consistent > nneighbours) return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: min_consistent %d out of range 0..%d", min_consistent, nneighbours);
    if (!(max_reproj_px >= 0.f) || !(max_rel_depth >= 0.f) || !(max_cost >= 0.f))
        return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: thresholds must be >= 0 (max_reproj_px %g, max_rel_depth %g, max_cost %g)", max_reproj_px, max_rel_depth, max_cost);
    int slots[kFuseMaxNeighbours + 1];
    slots[0] = ref_slot;
    for (int j = 0; j < nneighbours; j++) slots[j + 1] = neighbour_slots[j];
    for (int j = 0; j <= nneighbours; j++) {
        if (slots[j] < 0 || slots[j] >= cap) return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: slot %d outside the depth store (capacity %d)", slots[j], cap);
        if (j > 0 && slots[j] == ref_slot) return fail(ctx, MVS_EINVAL, "mvs_fuse_depth: neighbour %d is the reference slot %d", j - 1, ref_slot);
    }
    const bool use_cost = max_cost < INFINITY;
    for (int j = 0; j <= nneighbours; j++) {
        const mvs_ctx::DepthSlot &s = ctx->dstore[slots[j]];
        if (!s.have) return fail(ctx, MVS_ESTATE, "mvs_fuse_depth: slot %d holds no depth map (mvs_depth_upload)", slots[j]);
        if (use_cost && !s.have_cost) return fail(ctx, MVS_ESTATE, "mvs_fuse_depth: max_cost %g is finite but slot %d was stored without a cost map", max_cost, slots[j]);
    }
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H;
    const size_t P = (size_t)W * H;
    FuseArgs a;
    memset(&a, 0, sizeof(a));
    for (int j = 0; j <= nneighbours; j++) {
        const mvs_ctx::DepthSlot &s = ctx->dstore[slots[j]];
        a.depth[j] = (const float *)ctx->dstore_depth.ptr + P * slots[j];
        a.cost[j] = use_cost ? (const float *)ctx->dstore_cost.ptr + P * slots[j] : nullptr;
        memcpy(a.P[j], s.P, sizeof(s.P));
        memcpy(a.Pi[j], s.Pi, sizeof(s.Pi));
    }
    memcpy(a.C, ctx->dstore[ref_slot].C, sizeof(a.C));
    a.W = W;
    a.H = H;
    a.K = nneighbours;
    a.min_consistent = min_consistent;
    a.ntx = div_up(W, kFuseTX);
    a.use_cost = use_cost ? 1 : 0;
    a.invW = 1.0f / (float)W;
    a.invH = 1.0f / (float)H;
    a.halfW = (float)W * 0.5f;
    a.halfH = (float)H * 0.5f;
    a.max_reproj2 = max_reproj_px * max_reproj_px;
    a.max_rel = max_rel_depth;
    a.max_cost = max_cost;
    const size_t nseg = (size_t)H * a.ntx;
    int rc;
    ctx->fuse_have_rows = false;
    if ((rc = ensure(ctx, ctx->fuse_rows, P * 7 * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->fuse_counts, 2 * (nseg + 1) * sizeof(int)))) return rc;
    int *counts = (int *)ctx->fuse_counts.ptr, *offsets = counts + nseg + 1;
    size_t scan_bytes = 0;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, counts, offsets, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
        return fail(ctx, MVS_EHIP, "mvs_fuse_depth: scan sizing failed");
    if ((rc = ensure(ctx, ctx->fuse_scan, scan_bytes > 0 ? scan_bytes : 1))) return rc;
    const dim3 grid((unsigned)a.ntx, (unsigned)div_up(H, kFuseTY));
    {
        ProfileScope ps(ctx, MVS_K_FUSE);
        fuse_count_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, counts);
        MVS_HIP(ctx, hipGetLastError());
        if (rocprim::exclusive_scan(ctx->fuse_scan.ptr, scan_bytes, counts, offsets, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
            return fail(ctx, MVS_EHIP, "mvs_fuse_depth: scan failed");
        fuse_rows_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, offsets, (float *)ctx->fuse_rows.ptr);
        MVS_HIP(ctx, hipGetLastError());
    }
    int total = 0;
    MVS_HIP(ctx, hipMemcpyAsync(&total, offsets + nseg, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (out_points7 && total > 0) {
        MVS_HIP(ctx, hipMemcpyAsync(out_points7, ctx->fuse_rows.ptr, (size_t)total * 7 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
        MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->fuse_have_rows = true;
    *out_count = total;
    return MVS_OK;
}

void *mvs_fuse_points_device(mvs_ctx *ctx)
{
    if (!ctx) {
        fail(nullptr, MVS_EINVAL, "mvs_fuse_points_device: null context");
        return nullptr;
    }
    return ctx->fuse_have_rows ? ctx->fuse_rows.ptr : nullptr;
}

}  // extern "C"
