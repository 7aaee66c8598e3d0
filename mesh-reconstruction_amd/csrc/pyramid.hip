// pyramid.hip -- resolution pyramid for the band sweep (DESIGN.md section 20 is the contract; tests/pyramid_mirror.py restates it).
//
// The levels are separate contexts on one GPU: `fine` is W x H (both even), `coarse` exactly (W/2) x (H/2).  The cameras are NDC matrices
// and the centre of a coarse pixel is the mean of the centres of its four fine pixels, so the SAME 4 x 4 matrices serve every level; what a
// level needs is the frames at its size (rule D: the rounded mean of each 2 x 2 block) and, on the way back up, the coarser level's depth map
// as the finer level's prior (rule U: the 9-3-3-1 bilinear taps, optionally restricted to the taps whose guide pixel resembles the fine
// pixel's).  Three streaming kernels, bytes-bound by construction:
//   pyramid_down_raw    rule D on tightly packed frames: one thread = four coarse pixels = two dwords of each of two fine rows in, one dword out
//   pyramid_down_quads  rule D on quad images: the four texels of coarse pixel (r, c) are the four bytes of quad (2r + 1, 2c + 1)
//   pyramid_prior       rule U: one thread per fine pixel
// The two contexts have a stream each.  A kernel that reads one context's buffers and writes the other's runs on the CONSUMER's stream
// behind an event recorded on the producer's stream, and the producer's stream then waits for an event recorded behind that kernel, so its
// next work cannot overwrite what is still being read.  Nothing here waits on the host.
#include "sweep_shared.hpp"

namespace mvs {

namespace {

__device__ __forceinline__ uint32_t mean4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return (a + b + c + d + 2u) >> 2; }

// frame f of the launch is src + stride * (slots ? slots[f] : f): tightly packed frames, or slots of the frame store
__global__ __launch_bounds__(256) void pyramid_down_raw(const uint8_t *__restrict__ src, size_t stride, const int *__restrict__ slots, uint8_t *__restrict__ dst, int Wc, int Hc)
{
    const int c0 = 4 * (int)(blockIdx.x * 64 + (threadIdx.x & 63));
    const int r = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (c0 >= Wc || r >= Hc) return;
    const int W = 2 * Wc;
    const int f = blockIdx.z;
    const uint8_t *pa = src + stride * (size_t)(slots ? slots[f] : f) + (size_t)(2 * r) * W + 2 * c0, *pb = pa + W;
    uint8_t *out = dst + (size_t)Wc * Hc * f + (size_t)r * Wc + c0;
    const bool full = c0 + 4 <= Wc;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
    if (full && (((uintptr_t)pa | (uintptr_t)pb) & 3) == 0) {
        const uint32_t a0 = *(const uint32_t *)pa, a1 = *(const uint32_t *)(pa + 4), b0 = *(const uint32_t *)pb, b1 = *(const uint32_t *)(pb + 4);
        m[0] = mean4(a0 & 0xffu, (a0 >> 8) & 0xffu, b0 & 0xffu, (b0 >> 8) & 0xffu);
        m[1] = mean4((a0 >> 16) & 0xffu, a0 >> 24, (b0 >> 16) & 0xffu, b0 >> 24);
        m[2] = mean4(a1 & 0xffu, (a1 >> 8) & 0xffu, b1 & 0xffu, (b1 >> 8) & 0xffu);
        m[3] = mean4((a1 >> 16) & 0xffu, a1 >> 24, (b1 >> 16) & 0xffu, b1 >> 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c0 + k < Wc) m[k] = mean4(pa[2 * k], pa[2 * k + 1], pb[2 * k], pb[2 * k + 1]);
    }
    if (full && ((uintptr_t)out & 3) == 0) {
        *(uint32_t *)out = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c0 + k < Wc) out[k] = (uint8_t)m[k];
    }
}

// the side views of a context that built quad images (context.hip: quads[y][x] = texels (y-1, x-1), (y-1, x), (y, x-1), (y, x))
__global__ __launch_bounds__(256) void pyramid_down_quads(const uint32_t *__restrict__ quads, size_t slab, int pitch, uint8_t *__restrict__ dst, int Wc, int Hc)
{
    const int c0 = 4 * (int)(blockIdx.x * 64 + (threadIdx.x & 63));
    const int r = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (c0 >= Wc || r >= Hc) return;
    const int f = blockIdx.z;
    const uint32_t *q = quads + slab * f + (size_t)(2 * r + 1) * pitch + 2 * c0 + 1;
    uint8_t *out = dst + (size_t)Wc * Hc * f + (size_t)r * Wc + c0;
    uint32_t m[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (c0 + k < Wc) m[k] = __builtin_amdgcn_udot4(q[2 * k], 0x01010101u, 2u, false) >> 2;
    if (c0 + 4 <= Wc && ((uintptr_t)out & 3) == 0) {
        *(uint32_t *)out = m[0] | (m[1] << 8) | (m[2] << 16) | (m[3] << 24);
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (c0 + k < Wc) out[k] = (uint8_t)m[k];
    }
}

// rule U.  gc / gf: the coarse and fine guides, read only when tau < 255
__global__ __launch_bounds__(256) void pyramid_prior(const float *__restrict__ zc, const uint8_t *__restrict__ gc, const uint8_t *__restrict__ gf, float *__restrict__ out, int W,
                                                     int H, int tau)
{
    const int col = (int)(blockIdx.x * 64 + (threadIdx.x & 63));
    const int row = (int)(blockIdx.y * 4 + (threadIdx.x >> 6));
    if (col >= W || row >= H) return;
    const int Wc = W >> 1, Hc = H >> 1;
    const int r0 = max((row - 1) >> 1, 0), r1 = min(((row - 1) >> 1) + 1, Hc - 1);
    const int c0 = max((col - 1) >> 1, 0), c1 = min(((col - 1) >> 1) + 1, Wc - 1);
    const int wy0 = (row & 1) ? 3 : 1, wx0 = (col & 1) ? 3 : 1;
    const int at[4] = {r0 * Wc + c0, r0 * Wc + c1, r1 * Wc + c0, r1 * Wc + c1};
    const int w[4] = {wy0 * wx0, wy0 * (4 - wx0), (4 - wy0) * wx0, (4 - wy0) * (4 - wx0)};
    const size_t pix = (size_t)row * W + col;
    float z[4];
    bool valid[4], member[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        z[k] = zc[at[k]];
        valid[k] = z[k] > -1.0f && z[k] < 1.0f;   // false for NaN
        member[k] = valid[k];
    }
    if (tau < 255) {
        const int g = gf[pix];
        bool like[4];
#pragma unroll
        for (int k = 0; k < 4; k++) like[k] = valid[k] && abs((int)gc[at[k]] - g) <= tau;
        if (like[0] || like[1] || like[2] || like[3]) {
#pragma unroll
            for (int k = 0; k < 4; k++) member[k] = like[k];
        }
    }
    float num = 0.0f;
    int sw = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (member[k]) {
            const float t = (float)w[k] * z[k];
            num = sw ? num + t : t;    // the sum starts at the first member's product
            sw += w[k];
        }
    float r = MVS_BACKGROUND_DEPTH;
    if (sw) {
        const float q = num / (float)sw;
        if (q > -1.0f && q < 1.0f) r = q;
    }
    out[pix] = r;
}

// the two events of a context: [0] recorded on its stream when it is the producer, [1] behind the kernel it runs as the consumer
int pyramid_events(mvs_ctx *ctx)
{
    for (hipEvent_t &e : ctx->pyr_events)
        if (!e) MVS_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return MVS_OK;
}

// what every entry with two contexts checks first
int pyramid_pair(mvs_ctx *fine, mvs_ctx *coarse, const char *who)
{
    if (!fine || !coarse) return fail(fine ? fine : coarse, MVS_EINVAL, "%s: null context", who);
    if (fine == coarse) return fail(fine, MVS_EINVAL, "%s: fine and coarse are the same context", who);
    if (fine->device != coarse->device) return fail(fine, MVS_EINVAL, "%s: the contexts are on different devices (%d and %d)", who, fine->device, coarse->device);
    if ((fine->W | fine->H) & 1) return fail(fine, MVS_EINVAL, "%s: the fine context is %d x %d, both must be even", who, fine->W, fine->H);
    if (coarse->W != fine->W / 2 || coarse->H != fine->H / 2)
        return fail(fine, MVS_EINVAL, "%s: the coarse context is %d x %d, must be exactly %d x %d", who, coarse->W, coarse->H, fine->W / 2, fine->H / 2);
    return MVS_OK;
}

inline dim3 grid4(int Wc, int Hc, int nframes) { return dim3((unsigned)div_up(div_up(Wc, 4), 64), (unsigned)div_up(Hc, 4), (unsigned)nframes); }

}  // namespace

}  // namespace mvs

using namespace mvs;

int mvs_pyramid_downsample_device(mvs_ctx *fine, const void *src_dev, void *dst_dev, int nframes)
{
    if (!fine || !src_dev || !dst_dev) return fail(fine, MVS_EINVAL, "mvs_pyramid_downsample_device: null argument");
    if (nframes < 1 || nframes > 65535) return fail(fine, MVS_EINVAL, "mvs_pyramid_downsample_device: nframes %d out of range 1..65535", nframes);
    if ((fine->W | fine->H) & 1) return fail(fine, MVS_EINVAL, "mvs_pyramid_downsample_device: the context is %d x %d, both must be even", fine->W, fine->H);
    const size_t P = (size_t)fine->W * fine->H;
    const uintptr_t s = (uintptr_t)src_dev, d = (uintptr_t)dst_dev;
    if (s < d + (P / 4) * (size_t)nframes && d < s + P * (size_t)nframes) return fail(fine, MVS_EINVAL, "mvs_pyramid_downsample_device: source and destination overlap");
    MVS_HIP(fine, hipSetDevice(fine->device));
    {
        ProfileScope ps(fine, MVS_K_PROJECT);
        pyramid_down_raw<<<grid4(fine->W / 2, fine->H / 2, nframes), 256, 0, fine->stream>>>((const uint8_t *)src_dev, P, nullptr, (uint8_t *)dst_dev, fine->W / 2, fine->H / 2);
    }
    MVS_HIP(fine, hipGetLastError());
    return MVS_OK;
}

int mvs_pyramid_stage(mvs_ctx *fine, mvs_ctx *coarse)
{
    const char *who = "mvs_pyramid_stage";
    int rc;
    if ((rc = pyramid_pair(fine, coarse, who))) return rc;
    if (!fine->have_main || !fine->have_views || fine->V < 1) return fail(fine, MVS_ESTATE, "%s: set a main view and side views on the fine context first", who);
    if (fine->sampler != MVS_SAMPLER_FIXED || coarse->sampler != MVS_SAMPLER_FIXED)
        return fail(fine, MVS_ESTATE, "%s: implemented for MVS_SAMPLER_FIXED (the library default) on both contexts", who);
    if (fine->side_cams_host.size() != (size_t)fine->V * 16) return fail(fine, MVS_ESTATE, "%s: the fine context holds no side cameras for its %d views", who, fine->V);
    MVS_HIP(fine, hipSetDevice(fine->device));
    const int V = fine->V, Wc = coarse->W, Hc = coarse->H;
    const size_t Pc = (size_t)Wc * Hc;
    if ((rc = ensure(coarse, coarse->pyr_frames, Pc * (size_t)(V + 1)))) return fail(fine, rc, "%s: %s", who, coarse->err);
    if ((rc = pyramid_events(fine)) || (rc = pyramid_events(coarse))) return rc;
    uint8_t *frames = (uint8_t *)coarse->pyr_frames.ptr;
    // the kernels read the fine context's staged images and write the coarse context's frames: on the coarse stream, between the two events
    MVS_HIP(fine, hipEventRecord(fine->pyr_events[0], fine->stream));
    MVS_HIP(coarse, hipStreamWaitEvent(coarse->stream, fine->pyr_events[0], 0));
    {
        ProfileScope ps(coarse, MVS_K_PROJECT);
        pyramid_down_raw<<<grid4(Wc, Hc, 1), 256, 0, coarse->stream>>>(main_image_ptr(fine), 0, nullptr, frames, Wc, Hc);
        if (fine->views_in_store)
            pyramid_down_raw<<<grid4(Wc, Hc, V), 256, 0, coarse->stream>>>((const uint8_t *)fine->store_raw.ptr, (size_t)fine->W * fine->H, (const int *)fine->view_slots.ptr,
                                                                          frames + Pc, Wc, Hc);
        else
            pyramid_down_quads<<<grid4(Wc, Hc, V), 256, 0, coarse->stream>>>((const uint32_t *)fine->side_quads.ptr, fine->pad_slab, fine->pad_pitch, frames + Pc, Wc, Hc);
    }
    MVS_HIP(coarse, hipGetLastError());
    MVS_HIP(coarse, hipEventRecord(coarse->pyr_events[1], coarse->stream));
    MVS_HIP(fine, hipStreamWaitEvent(fine->stream, coarse->pyr_events[1], 0));
    // what mvs_sweep_set_main_device + mvs_sweep_set_views_device do with these frames and the fine context's cameras
    const std::vector<float> cams = fine->side_cams_host;
    std::vector<const uint8_t *> ptrs((size_t)V);
    for (int v = 0; v < V; v++) ptrs[v] = frames + Pc * (size_t)(v + 1);
    if ((rc = sweep_set_main_impl(coarse, fine->main_cam, frames, false, true)) || (rc = sweep_set_views_impl(coarse, V, cams.data(), ptrs.data(), false, false, true)))
        return fail(fine, rc, "%s: %s", who, coarse->err);
    return MVS_OK;
}

int mvs_pyramid_prior(mvs_ctx *fine, mvs_ctx *coarse, const void *coarse_depth_dev, int tau)
{
    const char *who = "mvs_pyramid_prior";
    int rc;
    if ((rc = pyramid_pair(fine, coarse, who))) return rc;
    if (tau < 0 || tau > 255) return fail(fine, MVS_EINVAL, "%s: tau %d outside 0..255", who, tau);
    if (!coarse_depth_dev && !coarse->depth.ptr) return fail(fine, MVS_ESTATE, "%s: coarse_depth_dev is null and the coarse context has no depth map", who);
    if (tau < 255 && (!fine->have_main || !coarse->have_main)) return fail(fine, MVS_ESTATE, "%s: tau < 255 needs a staged main image on both contexts (the guides)", who);
    MVS_HIP(fine, hipSetDevice(fine->device));
    if ((rc = ensure(fine, fine->band_prior, (size_t)fine->W * fine->H * sizeof(float)))) return rc;
    if ((rc = pyramid_events(fine)) || (rc = pyramid_events(coarse))) return rc;
    const float *zc = coarse_depth_dev ? (const float *)coarse_depth_dev : (const float *)coarse->depth.ptr;
    const uint8_t *gc = tau < 255 ? main_image_ptr(coarse) : nullptr, *gf = tau < 255 ? main_image_ptr(fine) : nullptr;
    // the kernel reads the coarse context's map and writes the fine context's prior: on the fine stream, between the two events
    MVS_HIP(coarse, hipEventRecord(coarse->pyr_events[0], coarse->stream));
    MVS_HIP(fine, hipStreamWaitEvent(fine->stream, coarse->pyr_events[0], 0));
    {
        ProfileScope ps(fine, MVS_K_ARGMIN);
        pyramid_prior<<<dim3((unsigned)div_up(fine->W, 64), (unsigned)div_up(fine->H, 4)), 256, 0, fine->stream>>>(zc, gc, gf, (float *)fine->band_prior.ptr, fine->W, fine->H, tau);
    }
    MVS_HIP(fine, hipGetLastError());
    note_new_prior(fine);
    MVS_HIP(fine, hipEventRecord(fine->pyr_events[1], fine->stream));
    MVS_HIP(coarse, hipStreamWaitEvent(coarse->stream, fine->pyr_events[1], 0));
    return MVS_OK;
}
