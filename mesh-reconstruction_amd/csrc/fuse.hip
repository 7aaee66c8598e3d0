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
//
// Section 28 adds a support plane (H*W u8) per slot -- one buffer, made by the first mvs_depth_support_upload -- and mvs_fuse_depth_masked:
// the same three launches with rule 1s (support >= min_support) wherever a stored depth is read.  The per-pixel contract lives in
// fuse_rules.hpp, shared with fuse_sequence.hip; the checks and the argument block of one reference (fuse_check_*, fuse_fill_args) are
// defined here for both files.
#include "fuse_rules.hpp"
#include "mvs_internal.hpp"

#include <rocprim/rocprim.hpp>

#include <cmath>

namespace mvs {

namespace {

// fuse_body (fuse_rules.hpp) over the two argument blocks of this file
__global__ __launch_bounds__(256) void fuse_count_kernel(const FuseArgs a, int *__restrict__ counts) { fuse_body<false>(a, counts, nullptr, nullptr); }
__global__ __launch_bounds__(256) void fuse_rows_kernel(const FuseArgs a, const int *__restrict__ offsets, float *__restrict__ rows)
{
    fuse_body<true>(a, nullptr, offsets, rows);
}
__global__ __launch_bounds__(256) void fuse_count_masked_kernel(const FuseMaskedArgs a, int *__restrict__ counts) { fuse_body<false>(a, counts, nullptr, nullptr); }
__global__ __launch_bounds__(256) void fuse_rows_masked_kernel(const FuseMaskedArgs a, const int *__restrict__ offsets, float *__restrict__ rows)
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
    ctx->dstore[slot].have_support = false;  // a new map is not described by the old plane's bytes
    ctx->dstore[slot].have_normals = false;  // (nor by the old normals': section 31)
    MVS_HIP(ctx, hipMemcpyAsync((float *)ctx->dstore_depth.ptr + P * slot, depth, P * sizeof(float), kind, ctx->stream));
    if (cost) MVS_HIP(ctx, hipMemcpyAsync((float *)ctx->dstore_cost.ptr + P * slot, cost, P * sizeof(float), kind, ctx->stream));
    s.have = true;
    s.have_cost = cost != nullptr;
    s.have_support = false;
    ctx->dstore[slot] = s;
    return MVS_OK;
}

// mvs_depth_support_upload / _upload_device: the one place the support buffer is allocated (capacity planes of H*W bytes)
int support_upload_impl(mvs_ctx *ctx, const char *who, int slot, const void *support, bool device)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!support) return fail(ctx, MVS_EINVAL, "%s: support is null", who);
    if (slot < 0 || slot >= (int)ctx->dstore.size())
        return fail(ctx, MVS_EINVAL, "%s: slot %d outside the depth store (capacity %d: mvs_depth_store first)", who, slot, (int)ctx->dstore.size());
    if (!ctx->dstore[slot].have) return fail(ctx, MVS_ESTATE, "%s: slot %d holds no depth map (mvs_depth_upload first)", who, slot);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->dstore_support, P * ctx->dstore.size()))) return rc;
    ctx->dstore[slot].have_support = false;
    MVS_HIP(ctx, hipMemcpyAsync((uint8_t *)ctx->dstore_support.ptr + P * slot, support, P, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    ctx->dstore[slot].have_support = true;
    return MVS_OK;
}

// the three launches of one reference into the context's fusion buffers (mvs_fuse_depth: min_support = 0, mvs_fuse_depth_masked)
int fuse_depth_impl(mvs_ctx *ctx, const char *who, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px,
                    float max_rel_depth, float max_cost, int min_support, float *out_points7, int *out_count)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!out_count) return fail(ctx, MVS_EINVAL, "%s: out_count is null", who);
    *out_count = 0;
    int rc;
    if ((rc = fuse_check_thresholds(ctx, who, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost, min_support))) return rc;
    if ((rc = fuse_check_slots(ctx, who, ref_slot, nneighbours, neighbour_slots, max_cost, min_support))) return rc;
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H;
    const size_t P = (size_t)W * H;
    FuseMaskedArgs a;
    fuse_fill_args(ctx, a, ref_slot, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost, min_support);
    const size_t nseg = (size_t)H * a.ntx;
    ctx->fuse_have_rows = false;
    if ((rc = ensure(ctx, ctx->fuse_rows, P * 7 * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->fuse_counts, 2 * (nseg + 1) * sizeof(int)))) return rc;
    int *counts = (int *)ctx->fuse_counts.ptr, *offsets = counts + nseg + 1;
    size_t scan_bytes = 0;
    if (rocprim::exclusive_scan(nullptr, scan_bytes, counts, offsets, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
        return fail(ctx, MVS_EHIP, "%s: scan sizing failed", who);
    if ((rc = ensure(ctx, ctx->fuse_scan, scan_bytes > 0 ? scan_bytes : 1))) return rc;
    const dim3 grid((unsigned)a.ntx, (unsigned)div_up(H, kFuseTY));
    {
        ProfileScope ps(ctx, MVS_K_FUSE);
        if (min_support > 0) fuse_count_masked_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, counts);
        else fuse_count_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, counts);
        MVS_HIP(ctx, hipGetLastError());
        if (rocprim::exclusive_scan(ctx->fuse_scan.ptr, scan_bytes, counts, offsets, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
            return fail(ctx, MVS_EHIP, "%s: scan failed", who);
        if (min_support > 0) fuse_rows_masked_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, offsets, (float *)ctx->fuse_rows.ptr);
        else fuse_rows_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, offsets, (float *)ctx->fuse_rows.ptr);
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

}  // namespace

int fuse_check_thresholds(mvs_ctx *ctx, const char *who, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px, float max_rel_depth, float max_cost, int min_support)
{
    if (nneighbours < 0 || nneighbours > kFuseMaxNeighbours) return fail(ctx, MVS_EINVAL, "%s: nneighbours %d out of range 0..%d", who, nneighbours, kFuseMaxNeighbours);
    if (nneighbours > 0 && !neighbour_slots) return fail(ctx, MVS_EINVAL, "%s: neighbour_slots is null", who);
    if (min_consistent < 0 || min_consistent > nneighbours) return fail(ctx, MVS_EINVAL, "%s: min_consistent %d out of range 0..%d", who, min_consistent, nneighbours);
    if (!(max_reproj_px >= 0.f) || !(max_rel_depth >= 0.f) || !(max_cost >= 0.f))
        return fail(ctx, MVS_EINVAL, "%s: thresholds must be >= 0 (max_reproj_px %g, max_rel_depth %g, max_cost %g)", who, max_reproj_px, max_rel_depth, max_cost);
    if (min_support < 0 || min_support > 255) return fail(ctx, MVS_EINVAL, "%s: min_support %d out of range 0..255", who, min_support);
    return MVS_OK;
}

int fuse_check_slots(mvs_ctx *ctx, const char *who, int ref_slot, int n, const int *slots, float max_cost, int min_support)
{
    const int cap = (int)ctx->dstore.size();
    const bool use_cost = max_cost < INFINITY;
    for (int j = -1; j < n; j++) {
        const int slot = j < 0 ? ref_slot : slots[j];
        if (slot < 0 || slot >= cap) return fail(ctx, MVS_EINVAL, "%s: slot %d outside the depth store (capacity %d)", who, slot, cap);
        if (j >= 0 && slot == ref_slot) return fail(ctx, MVS_EINVAL, "%s: neighbour %d is the reference slot %d", who, j, ref_slot);
    }
    for (int j = -1; j < n; j++) {
        const int slot = j < 0 ? ref_slot : slots[j];
        const mvs_ctx::DepthSlot &s = ctx->dstore[slot];
        if (!s.have) return fail(ctx, MVS_ESTATE, "%s: slot %d holds no depth map (mvs_depth_upload)", who, slot);
        if (use_cost && !s.have_cost) return fail(ctx, MVS_ESTATE, "%s: max_cost %g is finite but slot %d was stored without a cost map", who, max_cost, slot);
        if (min_support > 0 && !s.have_support)
            return fail(ctx, MVS_ESTATE, "%s: min_support %d > 0 but slot %d has no support plane (mvs_depth_support_upload)", who, min_support, slot);
    }
    return MVS_OK;
}

void fuse_fill_args(mvs_ctx *ctx, FuseMaskedArgs &a, int ref_slot, int n, const int *slots, int min_consistent, float max_reproj_px, float max_rel_depth,
                    float max_cost, int min_support)
{
    const int W = ctx->W, H = ctx->H;
    const size_t P = (size_t)W * H;
    const bool use_cost = max_cost < INFINITY;
    memset(&a, 0, sizeof(a));
    for (int j = 0; j <= n; j++) {
        const int slot = j ? slots[j - 1] : ref_slot;
        const mvs_ctx::DepthSlot &s = ctx->dstore[slot];
        a.depth[j] = (const float *)ctx->dstore_depth.ptr + P * slot;
        a.cost[j] = use_cost ? (const float *)ctx->dstore_cost.ptr + P * slot : nullptr;
        a.support[j] = min_support > 0 ? (const uint8_t *)ctx->dstore_support.ptr + P * slot : nullptr;
        memcpy(a.P[j], s.P, sizeof(s.P));
        memcpy(a.Pi[j], s.Pi, sizeof(s.Pi));
    }
    memcpy(a.C, ctx->dstore[ref_slot].C, sizeof(a.C));
    a.W = W;
    a.H = H;
    a.K = n;
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
    a.min_support = min_support;
}

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
    if (ctx->dstore_support.ptr) {  // the planes go with the store they described; the next support upload makes a buffer of the new capacity
        MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        MVS_HIP(ctx, hipFree(ctx->dstore_support.ptr));
        ctx->dstore_support = DevBuf();
    }
    if (ctx->store_normals.ptr) {  // and so do the normal planes (section 31)
        MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
        MVS_HIP(ctx, hipFree(ctx->store_normals.ptr));
        ctx->store_normals = DevBuf();
    }
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

int mvs_depth_support_upload(mvs_ctx *ctx, int slot, const uint8_t *support_hw) { return support_upload_impl(ctx, "mvs_depth_support_upload", slot, support_hw, false); }

int mvs_depth_support_upload_device(mvs_ctx *ctx, int slot, const void *support_dev)
{
    return support_upload_impl(ctx, "mvs_depth_support_upload_device", slot, support_dev, true);
}

int mvs_depth_support_fetch(mvs_ctx *ctx, int slot, uint8_t *support_hw)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_support_fetch: null context");
    if (!support_hw) return fail(ctx, MVS_EINVAL, "mvs_depth_support_fetch: support is null");
    if (slot < 0 || slot >= (int)ctx->dstore.size()) return fail(ctx, MVS_EINVAL, "mvs_depth_support_fetch: slot %d outside the depth store (capacity %d)", slot, (int)ctx->dstore.size());
    if (!ctx->dstore[slot].have || !ctx->dstore[slot].have_support) return fail(ctx, MVS_ESTATE, "mvs_depth_support_fetch: slot %d has no support plane", slot);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    MVS_HIP(ctx, hipMemcpyAsync(support_hw, (const uint8_t *)ctx->dstore_support.ptr + P * slot, P, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_depth_support_drop(mvs_ctx *ctx, int slot)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_support_drop: null context");
    if (slot < 0 || slot >= (int)ctx->dstore.size()) return fail(ctx, MVS_EINVAL, "mvs_depth_support_drop: slot %d outside the depth store (capacity %d)", slot, (int)ctx->dstore.size());
    ctx->dstore[slot].have_support = false;
    return MVS_OK;
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
    return fuse_depth_impl(ctx, "mvs_fuse_depth", ref_slot, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost, 0, out_points7,
                           out_count);
}

int mvs_fuse_depth_masked(mvs_ctx *ctx, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px, float max_rel_depth,
                          float max_cost, int min_support, float *out_points7, int *out_count)
{
    return fuse_depth_impl(ctx, "mvs_fuse_depth_masked", ref_slot, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost,
                           min_support, out_points7, out_count);
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
