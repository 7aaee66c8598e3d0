// normals.hip -- normal maps from the propagation's slopes, a normal plane per depth slot and the fusion that reads the planes
// (include/mvs.h "normals").
//
// mvs_propagate_normals turns the stage's hypotheses (z, gx, gy) into world-space unit normals (rule N1): the NDC plane of a pixel times
// the main camera's matrix is its world plane.  One thread per pixel, three coalesced plane reads and one 12-byte write; the matrix and the
// centre are kernel arguments, which every lane reads with the same (scalar) loads.  The kernel is launch-bound at every size.
//
// A normal plane is H*W*3 f32 (interleaved, unit, zeros = none: the ray-cast's layout) per depth slot, in one buffer beside the depth store
// that the first normals upload makes -- handled like section 28's support planes.
//
// mvs_fuse_depth_normals is mvs_fuse_depth_masked with rules 3n and 5n: fuse_rules.hpp's fuse_pixel / fuse_body over FuseNormalArgs, in
// two kernels of this file, with the 64 x 4 tiles, the compaction and the one host synchronisation of csrc/fuse.hip.
//
// Arithmetic: f32, one rounding per operation, no contraction; tests/normals_mirror.py restates it in numpy.
#include "fuse_rules.hpp"
#include "mvs_internal.hpp"
#include "normals_rules.hpp"

#include <rocprim/rocprim.hpp>

#include <cmath>

namespace mvs {

namespace {

// rule N1 (normals_rules.hpp holds its body)
__global__ __launch_bounds__(256) void hypothesis_normals_kernel(const NormalCam k, const float *__restrict__ zmap, const float *__restrict__ gxmap,
                                                                  const float *__restrict__ gymap, float *__restrict__ out, int W, int H, float invW, float invH,
                                                                  float halfW, float halfH)
{
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= (size_t)W * H) return;
    const int row = (int)(p / W), col = (int)(p - (size_t)row * W);
    const float z = zmap[p], gx = gxmap[p], gy = gymap[p];
    float nx, ny, nz;
    rule_n1(k, row, col, z, gx, gy, invW, invH, halfW, halfH, nx, ny, nz);
    out[3 * p] = nx;
    out[3 * p + 1] = ny;
    out[3 * p + 2] = nz;
}

__global__ __launch_bounds__(256) void fuse_count_normals_kernel(const FuseNormalArgs a, int *__restrict__ counts) { fuse_body<false>(a, counts, nullptr, nullptr); }
__global__ __launch_bounds__(256) void fuse_rows_normals_kernel(const FuseNormalArgs a, const int *__restrict__ offsets, float *__restrict__ rows)
{
    fuse_body<true>(a, nullptr, offsets, rows);
}

// mvs_depth_normals_upload / _upload_device: the one place the planes' buffer is allocated (capacity planes of H*W*3 f32)
int normals_upload_impl(mvs_ctx *ctx, const char *who, int slot, const void *normals, bool device)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!normals) return fail(ctx, MVS_EINVAL, "%s: normals is null", who);
    if (slot < 0 || slot >= (int)ctx->dstore.size())
        return fail(ctx, MVS_EINVAL, "%s: slot %d outside the depth store (capacity %d: mvs_depth_store first)", who, slot, (int)ctx->dstore.size());
    if (!ctx->dstore[slot].have) return fail(ctx, MVS_ESTATE, "%s: slot %d holds no depth map (mvs_depth_upload first)", who, slot);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->W * ctx->H * 3 * sizeof(float);
    int rc;
    if ((rc = ensure(ctx, ctx->store_normals, bytes * ctx->dstore.size()))) return rc;
    ctx->dstore[slot].have_normals = false;
    MVS_HIP(ctx, hipMemcpyAsync((char *)ctx->store_normals.ptr + bytes * slot, normals, bytes, device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    ctx->dstore[slot].have_normals = true;
    return MVS_OK;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_propagate_normals(mvs_ctx *ctx, const float cam[16])
{
    static const char who[] = "mvs_propagate_normals";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!cam) return fail(ctx, MVS_EINVAL, "%s: cam is null", who);
    if (!ctx->prop_have) return fail(ctx, MVS_ESTATE, "%s: no hypotheses yet (mvs_propagate_init first)", who);
    mvs_ctx::DepthSlot s;
    if (!slot_matrices(cam, s)) return fail(ctx, MVS_EINVAL, "%s: the camera has a non-finite entry, is singular or has no finite centre", who);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->hyp_normals, P * 3 * sizeof(float)))) return rc;
    NormalCam k;
    memcpy(k.P, s.P, sizeof(k.P));
    memcpy(k.C, s.C, sizeof(k.C));
    const float *maps = (const float *)mvs_propagate_depth_device(ctx);   // z, gx, gy: H*W f32 each, one behind the other
    {
        ProfileScope ps(ctx, MVS_K_FUSE);
        hypothesis_normals_kernel<<<(unsigned)((P + 255) / 256), 256, 0, ctx->stream>>>(k, maps, maps + P, maps + 2 * P, (float *)ctx->hyp_normals.ptr, ctx->W, ctx->H,
                                                                                     1.0f / (float)ctx->W, 1.0f / (float)ctx->H, (float)ctx->W * 0.5f,
                                                                                     (float)ctx->H * 0.5f);
        MVS_HIP(ctx, hipGetLastError());
    }
    ctx->hyp_normals_have = true;
    return MVS_OK;
}

void *mvs_propagate_normals_device(mvs_ctx *ctx) { return ctx && ctx->hyp_normals_have ? ctx->hyp_normals.ptr : nullptr; }

int mvs_propagate_normals_fetch(mvs_ctx *ctx, float *normals_hw3)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_propagate_normals_fetch: null context");
    if (!normals_hw3) return fail(ctx, MVS_EINVAL, "mvs_propagate_normals_fetch: normals_hw3 is null");
    if (!ctx->hyp_normals_have) return fail(ctx, MVS_ESTATE, "mvs_propagate_normals_fetch: no normals yet (mvs_propagate_normals first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(normals_hw3, ctx->hyp_normals.ptr, (size_t)ctx->W * ctx->H * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_depth_normals_upload(mvs_ctx *ctx, int slot, const float *normals_hw3) { return normals_upload_impl(ctx, "mvs_depth_normals_upload", slot, normals_hw3, false); }

int mvs_depth_normals_upload_device(mvs_ctx *ctx, int slot, const void *normals_dev)
{
    return normals_upload_impl(ctx, "mvs_depth_normals_upload_device", slot, normals_dev, true);
}

int mvs_depth_normals_fetch(mvs_ctx *ctx, int slot, float *normals_hw3)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_normals_fetch: null context");
    if (!normals_hw3) return fail(ctx, MVS_EINVAL, "mvs_depth_normals_fetch: normals is null");
    if (slot < 0 || slot >= (int)ctx->dstore.size()) return fail(ctx, MVS_EINVAL, "mvs_depth_normals_fetch: slot %d outside the depth store (capacity %d)", slot, (int)ctx->dstore.size());
    if (!ctx->dstore[slot].have || !ctx->dstore[slot].have_normals) return fail(ctx, MVS_ESTATE, "mvs_depth_normals_fetch: slot %d has no normal plane", slot);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->W * ctx->H * 3 * sizeof(float);
    MVS_HIP(ctx, hipMemcpyAsync(normals_hw3, (const char *)ctx->store_normals.ptr + bytes * slot, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_depth_normals_drop(mvs_ctx *ctx, int slot)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_depth_normals_drop: null context");
    if (slot < 0 || slot >= (int)ctx->dstore.size()) return fail(ctx, MVS_EINVAL, "mvs_depth_normals_drop: slot %d outside the depth store (capacity %d)", slot, (int)ctx->dstore.size());
    ctx->dstore[slot].have_normals = false;
    return MVS_OK;
}

int mvs_fuse_depth_normals(mvs_ctx *ctx, int ref_slot, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px, float max_rel_depth,
                           float max_cost, int min_support, float min_normal_cos, float *out_points7, int *out_count)
{
    static const char who[] = "mvs_fuse_depth_normals";
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!out_count) return fail(ctx, MVS_EINVAL, "%s: out_count is null", who);
    *out_count = 0;
    int rc;
    if ((rc = fuse_check_thresholds(ctx, who, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost, min_support))) return rc;
    if (!(min_normal_cos <= 1.0f)) return fail(ctx, MVS_EINVAL, "%s: min_normal_cos %g is NaN or above 1", who, (double)min_normal_cos);
    if ((rc = fuse_check_slots(ctx, who, ref_slot, nneighbours, neighbour_slots, max_cost, min_support))) return rc;
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H;
    const size_t P = (size_t)W * H;
    FuseNormalArgs a;
    fuse_fill_args(ctx, a, ref_slot, nneighbours, neighbour_slots, min_consistent, max_reproj_px, max_rel_depth, max_cost, min_support);
    for (int j = 0; j <= kFuseMaxNeighbours; j++) {
        const int slot = j == 0 ? ref_slot : j <= nneighbours ? neighbour_slots[j - 1] : -1;
        a.normals[j] = slot >= 0 && ctx->dstore[slot].have_normals ? (const float *)ctx->store_normals.ptr + 3 * P * slot : nullptr;
    }
    a.min_cos = min_normal_cos;
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
        fuse_count_normals_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, counts);
        MVS_HIP(ctx, hipGetLastError());
        if (rocprim::exclusive_scan(ctx->fuse_scan.ptr, scan_bytes, counts, offsets, 0, nseg + 1, rocprim::plus<int>(), ctx->stream) != hipSuccess)
            return fail(ctx, MVS_EHIP, "%s: scan failed", who);
        fuse_rows_normals_kernel<<<grid, kFuseTX * kFuseTY, 0, ctx->stream>>>(a, offsets, (float *)ctx->fuse_rows.ptr);
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

}  // extern "C"
