// appearance.hip -- reading the TSDF volume's appearance (include/mvs.h "appearance of the TSDF volume"): the grey
// level the frames voted into the volume (mvs_tsdf_integrate_frames, csrc/tsdf.hip), at the surface points of a depth map
// (mvs_tsdf_shade) or at a caller's points (mvs_tsdf_sample_appearance).
//
//   tsdf_shade_kernel    one thread per pixel, a wavefront is an 8 x 8 pixel tile as in the ray kernel (its 8 corner gathers of 4 bytes land
//                        on a few lines), a workgroup 16 x 16 pixels: the pixel's depth back-projected as the fusion reads a stored map
//                        (csrc/depth_rules.hpp), the appearance there, a (value, 255) or (0, 0) pair of u8 like mvs_warp_by_depth's;
//   tsdf_sample_kernel   one thread per point (x, y, z, w): the appearance at (x, y, z) / w, NaN where there is none.
// Both go through appearance_at: trilinear over the cell's corners that hold a vote, renormalised by their weight; no clamping into the box.
//
// Arithmetic: f32, one rounding per operation, no contraction (-ffp-contract=off); tests/appearance_mirror.py restates it in numpy, bit for bit.
#include "depth_rules.hpp"
#include "mvs_internal.hpp"
#include "volume_rules.hpp"

#include <cmath>

namespace mvs {

namespace {

constexpr int kShadeTile = 16;  // workgroup: 16 x 16 pixels = 4 wavefronts of 8 x 8

struct AppVolume {
    const uint32_t *cells;
    float o[3];
    float inv_h;
    int G;
};

struct ShadeArgs {
    float P[16], Pi[16];
    AppVolume vol;
    float invW, invH;
    int W, H;
    const float *depth;
    unsigned char *out;
};

// rule C: false = none
__device__ __forceinline__ bool appearance_at(const AppVolume &a, float3 X, float &value)
{
    const float gx = (X.x - a.o[0]) * a.inv_h, gy = (X.y - a.o[1]) * a.inv_h, gz = (X.z - a.o[2]) * a.inv_h;
    const float top = (float)(a.G - 1);
    if (!(gx >= 0.f && gx <= top && gy >= 0.f && gy <= top && gz >= 0.f && gz <= top)) return false;  // (NaN fails too)
    float fx, fy, fz;
    const int ix = cell_axis(gx, a.G, fx), iy = cell_axis(gy, a.G, fy), iz = cell_axis(gz, a.G, fz);
    const int G = a.G, GG = a.G * a.G;
    const uint32_t *q = a.cells + ((iz * G + iy) * G + ix);   // < 2^27 at G = 512; the cell index is at most G - 2: all 8 corners exist
    const uint32_t c[8] = {q[0], q[1], q[G], q[G + 1], q[GG], q[GG + 1], q[GG + G], q[GG + G + 1]};
    float num = 0.f, den = 0.f;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        const float wx = (d & 1) ? fx : 1.0f - fx, wy = (d & 2) ? fy : 1.0f - fy, wz = (d & 4) ? fz : 1.0f - fz;
        const float w = (wx * wy) * wz;
        const uint32_t n = c[d] >> 24;
        if (n > 0) {
            const float v = (float)(c[d] & 0xFFFFFFu) / (float)n;
            num = num + w * v;
            den = den + w;
        }
    }
    if (!(den > 0.f)) return false;
    value = num / den;
    return true;
}

__global__ __launch_bounds__(256) void tsdf_shade_kernel(const ShadeArgs a)
{
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * kShadeTile + (wave & 1) * 8 + (lane & 7);
    const int row = blockIdx.y * kShadeTile + (wave >> 1) * 8 + (lane >> 3);
    if (col >= a.W || row >= a.H) return;
    const size_t p = (size_t)row * a.W + col;
    unsigned char grey = 0, have = 0;
    const float z = a.depth[p];
    if (depth_valid(z, nullptr, p, 0, 0.f)) {
        const float xn = __builtin_fmaf((float)(2 * col + 1), a.invW, -1.0f);
        const float yn = __builtin_fmaf(-(float)(2 * row + 1), a.invH, 1.0f);
        const float3 X = unproject(a.Pi, xn, yn, z);
        float value;
        if (prow(a.P, 3, X) > 0.f && appearance_at(a.vol, X, value)) {
            const float r = floorf(value + 0.5f);
            grey = (unsigned char)(r < 255.0f ? (int)r : 255);
            have = 255;
        }
    }
    reinterpret_cast<uchar2 *>(a.out)[p] = make_uchar2(grey, have);
}

__global__ __launch_bounds__(256) void tsdf_sample_kernel(const AppVolume a, int n, const float4 *__restrict__ points, float *__restrict__ out)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const float4 h = points[q];
    float value;
    out[q] = appearance_at(a, make_float3(h.x / h.w, h.y / h.w, h.z / h.w), value) ? value : __builtin_nanf("");
}

AppVolume app_volume(const mvs_ctx *ctx)
{
    AppVolume v;
    v.cells = (const uint32_t *)ctx->tsdf_app.ptr;
    for (int c = 0; c < 3; c++) v.o[c] = ctx->tsdf_origin[c];
    v.inv_h = 1.0f / ctx->tsdf_h;  // rounded once, as the raycast's
    v.G = ctx->tsdf_G;
    return v;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_tsdf_shade(mvs_ctx *ctx, const float cam[16], const void *depth_dev)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_shade: null context");
    if (!cam || !depth_dev) return fail(ctx, MVS_EINVAL, "mvs_tsdf_shade: null argument");
    mvs_ctx::DepthSlot s;
    if (!slot_matrices(cam, s)) return fail(ctx, MVS_EINVAL, "mvs_tsdf_shade: the camera is not finite, is singular or has no finite centre");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_shade: no volume (mvs_tsdf_volume first)");
    if (!ctx->tsdf_app_have) return fail(ctx, MVS_ESTATE, "mvs_tsdf_shade: no appearance volume (mvs_tsdf_integrate_frames or mvs_tsdf_appearance_upload first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->shade_map, (size_t)W * H * 2))) return rc;
    ShadeArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.P, s.P, sizeof(a.P));
    memcpy(a.Pi, s.Pi, sizeof(a.Pi));
    a.vol = app_volume(ctx);
    a.invW = 1.0f / (float)W;
    a.invH = 1.0f / (float)H;
    a.W = W;
    a.H = H;
    a.depth = (const float *)depth_dev;
    a.out = (unsigned char *)ctx->shade_map.ptr;
    ProfileScope ps(ctx, MVS_K_TSDF);
    tsdf_shade_kernel<<<dim3((unsigned)div_up(W, kShadeTile), (unsigned)div_up(H, kShadeTile)), 256, 0, ctx->stream>>>(a);
    MVS_HIP(ctx, hipGetLastError());
    ctx->shade_have = true;
    return MVS_OK;
}

void *mvs_tsdf_shade_device(mvs_ctx *ctx) { return ctx && ctx->shade_have ? ctx->shade_map.ptr : nullptr; }

int mvs_tsdf_shade_fetch(mvs_ctx *ctx, uint8_t *shaded_hw2)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_shade_fetch: null context");
    if (!shaded_hw2) return fail(ctx, MVS_EINVAL, "mvs_tsdf_shade_fetch: null array");
    if (!ctx->shade_have) return fail(ctx, MVS_ESTATE, "mvs_tsdf_shade_fetch: no shaded map yet (mvs_tsdf_shade first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    MVS_HIP(ctx, hipMemcpyAsync(shaded_hw2, ctx->shade_map.ptr, (size_t)ctx->W * ctx->H * 2, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_tsdf_sample_appearance(mvs_ctx *ctx, const float *points4, int n, float *out)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_sample_appearance: null context");
    if (!points4 || !out) return fail(ctx, MVS_EINVAL, "mvs_tsdf_sample_appearance: null array");
    if (n < 1) return fail(ctx, MVS_EINVAL, "mvs_tsdf_sample_appearance: n %d < 1", n);
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_sample_appearance: no volume (mvs_tsdf_volume first)");
    if (!ctx->tsdf_app_have) return fail(ctx, MVS_ESTATE, "mvs_tsdf_sample_appearance: no appearance volume (mvs_tsdf_integrate_frames or mvs_tsdf_appearance_upload first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = ensure(ctx, ctx->app_points, (size_t)n * 5 * sizeof(float)))) return rc;
    float4 *pts = (float4 *)ctx->app_points.ptr;
    float *vals = (float *)(pts + n);
    MVS_HIP(ctx, hipMemcpyAsync(pts, points4, (size_t)n * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    {
        ProfileScope ps(ctx, MVS_K_TSDF);
        tsdf_sample_kernel<<<(unsigned)div_up(n, 256), 256, 0, ctx->stream>>>(app_volume(ctx), n, pts, vals);
        MVS_HIP(ctx, hipGetLastError());
    }
    MVS_HIP(ctx, hipMemcpyAsync(out, vals, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

}  // extern "C"
