// lens.hip -- the tracks file's radial lens model on the device: a distorted frame resampled into the pinhole frame the cameras
// describe.  The model is the reference's cameraToScreen (configuration.cpp:248-259) with the pixel mapping of
// configuration.cpp:292-293, applied to the pixel centres of the OUTPUT frame; the sampler is remap_cubic_kernel's (photometric.hip)
// with a replicated border instead of a zero one.  All f32, one rounding per operation (the library is built with -ffp-contract=off;
// the two pixel-centre expressions are the sweep's explicit fmas).
#include <cmath>

#include "mvs_internal.hpp"

namespace mvs {

struct LensArgs {
    int W, H;
    float invW, invH, Wf, Hf;
    float a;       // (float)H / (float)W, rounded once on the host
    float cx, hc;  // centre x; (float)H - centre y (the tracks files measure the centre's y from the bottom), rounded once on the host
    float k1, k2, k3;
};

// rules 1-4: the source position, in pixel indices, of output pixel (row, col)
__device__ __forceinline__ void lens_position(const LensArgs &L, int col, int row, float &mx, float &my)
{
    const float xn = __builtin_fmaf((float)(2 * col + 1), L.invW, -1.0f);  // the sweep's pixel centres (sweep.hip: sweep_generic)
    const float yn = __builtin_fmaf(-(float)(2 * row + 1), L.invH, 1.0f);
    const float r2 = (xn * xn + ((yn * yn) * L.a) * L.a) * 0.25f;
    const float k = 1.0f + r2 * (L.k1 + r2 * (L.k2 + r2 * L.k3));
    const float X = L.cx + ((xn * k) * L.Wf) * 0.5f;
    const float Y = L.hc - ((yn * k) * L.Hf) * 0.5f;
    mx = X - 0.5f;
    my = Y - 0.5f;
}

// one thread per output pixel, 64 x 4 pixels per workgroup, blockIdx.z = frame (source and destination W*H bytes apart)
__global__ __launch_bounds__(256) void undistort_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const short *__restrict__ itab, LensArgs L)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= L.W || y >= L.H) return;
    const size_t P = (size_t)L.W * L.H;
    src += P * blockIdx.z;
    dst += P * blockIdx.z;
    float mx, my;
    lens_position(L, x, y, mx, my);
    const int qx = __float2int_rn(mx * 32.0f), qy = __float2int_rn(my * 32.0f);
    int sx = (qx >> 5) - 1, sy = (qy >> 5) - 1;
    const int fx = qx & 31, fy = qy & 31;
    sx = max(-32767, min(32767, sx));
    sy = max(-32767, min(32767, sy));
    // the 16 Q15 weights of this pair of fractions: 32 bytes, 32-byte aligned
    const int4 *w4 = reinterpret_cast<const int4 *>(itab + (size_t)(fy * 32 + fx) * 16);
    const int4 wa = w4[0], wb = w4[1];
    const int wp[8] = {wa.x, wa.y, wa.z, wa.w, wb.x, wb.y, wb.z, wb.w};
    int xs[4];
#pragma unroll
    for (int k2 = 0; k2 < 4; k2++) xs[k2] = max(0, min(L.W - 1, sx + k2));  // a tap outside the frame takes the nearest frame pixel
    int sum = 0;
#pragma unroll
    for (int k1 = 0; k1 < 4; k1++) {
        const uint8_t *row = src + (size_t)max(0, min(L.H - 1, sy + k1)) * L.W;
#pragma unroll
        for (int k2 = 0; k2 < 4; k2++) {
            const int pair = wp[k1 * 2 + (k2 >> 1)];
            const int w = (k2 & 1) ? (pair >> 16) : (int)(short)(pair & 0xffff);
            sum += (int)row[xs[k2]] * w;
        }
    }
    const int v = (sum + (1 << 14)) >> 15;
    dst[(size_t)y * L.W + x] = (uint8_t)max(0, min(255, v));
}

// diagnostic: (mx, my) of every output pixel
__global__ __launch_bounds__(256) void undistort_map_kernel(float *__restrict__ map, LensArgs L)
{
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= L.W || y >= L.H) return;
    float mx, my;
    lens_position(L, x, y, mx, my);
    float *m = map + ((size_t)y * L.W + x) * 2;
    m[0] = mx;
    m[1] = my;
}

static LensArgs lens_args(const mvs_ctx *ctx)
{
    LensArgs L;
    L.W = ctx->W;
    L.H = ctx->H;
    L.invW = 1.0f / (float)ctx->W;
    L.invH = 1.0f / (float)ctx->H;
    L.Wf = (float)ctx->W;
    L.Hf = (float)ctx->H;
    L.a = (float)ctx->H / (float)ctx->W;
    L.cx = ctx->lens_cx;
    L.hc = (float)ctx->H - ctx->lens_cy;
    L.k1 = ctx->lens_k[0];
    L.k2 = ctx->lens_k[1];
    L.k3 = ctx->lens_k[2];
    return L;
}

// nframes tightly packed frames through the context's lens, in one launch on the context's stream (the caller has checked the lens,
// the pointers and that the ranges do not overlap)
int undistort_launch(mvs_ctx *ctx, const uint8_t *src_dev, uint8_t *dst_dev, int nframes)
{
    int rc = ensure_cubic_table(ctx);
    if (rc) return rc;
    ProfileScope ps(ctx, MVS_K_PROJECT);
    undistort_kernel<<<dim3(div_up(ctx->W, 64), div_up(ctx->H, 4), (unsigned)nframes), 256, 0, ctx->stream>>>(src_dev, dst_dev, (const short *)ctx->cubic_tab.ptr, lens_args(ctx));
    MVS_HIP(ctx, hipGetLastError());
    return MVS_OK;
}

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_set_lens(mvs_ctx *ctx, const float k[3], float center_x, float center_y)
{
    if (!ctx) return fail(ctx, MVS_EINVAL, "mvs_set_lens: null context");
    if (!k) {
        ctx->lens_set = false;
        return MVS_OK;
    }
    if (!std::isfinite(center_x) || !std::isfinite(center_y)) return fail(ctx, MVS_EINVAL, "mvs_set_lens: the centre is not finite");
    for (int i = 0; i < 3; i++)
        if (!std::isfinite(k[i]) || std::fabs(k[i]) > MVS_LENS_MAX_COEFFICIENT)
            return fail(ctx, MVS_EINVAL, "mvs_set_lens: k[%d] = %g is not finite or beyond +-%d", i, (double)k[i], MVS_LENS_MAX_COEFFICIENT);
    // the radial map rho -> rho k(rho^2) must grow all the way to the farthest corner of the frame: its derivative
    // 1 + 3 k1 rho^2 + 5 k2 rho^4 + 7 k3 rho^6, in double, at rho_max i / 1024 for i = 1..1024, rho_max^2 = (1 + a^2) / 4
    const double a = (double)ctx->H / (double)ctx->W, rho_max = std::sqrt((1.0 + a * a) * 0.25);
    for (int i = 1; i <= 1024; i++) {
        const double rho = rho_max * i / 1024.0, s = rho * rho;
        if (!(1.0 + s * (3.0 * k[0] + s * (5.0 * k[1] + s * 7.0 * k[2])) > 0.0))
            return fail(ctx, MVS_EINVAL, "mvs_set_lens: the radial map folds over inside the frame (at %.3f of the way to the corner)", i / 1024.0);
    }
    for (int i = 0; i < 3; i++) ctx->lens_k[i] = k[i];
    ctx->lens_cx = center_x;
    ctx->lens_cy = center_y;
    ctx->lens_set = true;
    return MVS_OK;
}

int mvs_lens(mvs_ctx *ctx, float k_out[3], float *center_x, float *center_y)
{
    if (!ctx) return fail(ctx, MVS_EINVAL, "mvs_lens: null context");
    if (!ctx->lens_set) return 0;
    if (k_out)
        for (int i = 0; i < 3; i++) k_out[i] = ctx->lens_k[i];
    if (center_x) *center_x = ctx->lens_cx;
    if (center_y) *center_y = ctx->lens_cy;
    return 1;
}

int mvs_undistort(mvs_ctx *ctx, const uint8_t *src_hw, uint8_t *dst_hw)
{
    if (!ctx || !src_hw || !dst_hw) return fail(ctx, MVS_EINVAL, "mvs_undistort: null argument");
    if (!ctx->lens_set) return fail(ctx, MVS_ESTATE, "mvs_undistort: no lens is set (mvs_set_lens)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    int rc;
    if ((rc = ensure(ctx, ctx->upload, 2 * P))) return rc;
    uint8_t *src = (uint8_t *)ctx->upload.ptr, *dst = src + P;
    MVS_HIP(ctx, hipMemcpyAsync(src, src_hw, P, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = undistort_launch(ctx, src, dst, 1))) return rc;
    MVS_HIP(ctx, hipMemcpyAsync(dst_hw, dst, P, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_undistort_device(mvs_ctx *ctx, const void *src_dev, void *dst_dev, int nframes)
{
    if (!ctx || !src_dev || !dst_dev) return fail(ctx, MVS_EINVAL, "mvs_undistort_device: null argument");
    if (nframes < 1 || nframes > 65535) return fail(ctx, MVS_EINVAL, "mvs_undistort_device: nframes %d out of range 1..65535", nframes);
    if (!ctx->lens_set) return fail(ctx, MVS_ESTATE, "mvs_undistort_device: no lens is set (mvs_set_lens)");
    const size_t bytes = (size_t)ctx->W * ctx->H * (size_t)nframes;
    const uintptr_t s = (uintptr_t)src_dev, d = (uintptr_t)dst_dev;
    if (s < d + bytes && d < s + bytes) return fail(ctx, MVS_EINVAL, "mvs_undistort_device: source and destination overlap");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    return undistort_launch(ctx, (const uint8_t *)src_dev, (uint8_t *)dst_dev, nframes);
}

int mvs_undistort_map(mvs_ctx *ctx, float *map_hw2)
{
    if (!ctx || !map_hw2) return fail(ctx, MVS_EINVAL, "mvs_undistort_map: null argument");
    if (!ctx->lens_set) return fail(ctx, MVS_ESTATE, "mvs_undistort_map: no lens is set (mvs_set_lens)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t bytes = (size_t)ctx->W * ctx->H * 2 * sizeof(float);
    int rc;
    if ((rc = ensure(ctx, ctx->r_tmp0, bytes))) return rc;
    {
        ProfileScope ps(ctx, MVS_K_PROJECT);
        undistort_map_kernel<<<dim3(div_up(ctx->W, 64), div_up(ctx->H, 4)), 256, 0, ctx->stream>>>((float *)ctx->r_tmp0.ptr, lens_args(ctx));
        MVS_HIP(ctx, hipGetLastError());
    }
    MVS_HIP(ctx, hipMemcpyAsync(map_hw2, ctx->r_tmp0.ptr, bytes, hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

}  // extern "C"
