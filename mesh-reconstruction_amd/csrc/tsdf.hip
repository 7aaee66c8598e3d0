// tsdf.hip -- TSDF fusion (include/mvs.h "TSDF fusion"): every stored depth map votes a truncated signed distance
// along its own rays into one G^3 volume owned by the context; mvs_tsdf_surface meshes the averaged field's zero level set with Poisson's
// surface nets (csrc/poisson.hip: surface_nets_device).
//
// mvs_tsdf_integrate runs per chunk of up to kTsdfChunk listed slots, in list order, two launches:
//   tsdf_wmap_kernel       one thread per pixel and slot of the chunk: the slot's linear depth w where the stored pixel is valid (fusion
//                          rules 1 and 2, csrc/depth_rules.hpp, exactly as mvs_fuse_depth reads it), NaN elsewhere;
//   tsdf_integrate_kernel  one thread per node, i fastest: with blockDim 256 = 64 x 4 every wavefront is one run of 64 nodes of one
//                          (j, k) row, so the bracket (P[r][1] y + P[r][2] z) + P[r][3] is wave-uniform and a wave's depth gathers land on a
//                          few neighbouring image lines.  The chunk's rows x, y, w of P travel by value in the kernel arguments (as
//                          FuseArgs does); the node's (sum, count) is read once, updated by the chunk's slots in list order, written once.
//                          No atomics, no LDS: the result is the same bytes however the list is split into calls or chunks.
// mvs_tsdf_surface: tsdf_field_kernel turns (sum, count) into F and the cell support mask, then the shared mesher runs on ctx->stream.
// The field is kept (tsdf_ensure_field) until the volume changes; mvs_tsdf_raycast (csrc/raycast.hip) reads it too.  mvs_tsdf_upload is the
// counterpart of mvs_tsdf_fetch: it replaces both fields by the caller's.
//
// mvs_tsdf_integrate_frames is the same pair of launches with the frames' intensities carried along:
//   tsdf_wmap_frames_kernel       the w-map pass writing 8-byte records (w, intensity of that pixel in the listed frame-store slot);
//   tsdf_integrate_frames_kernel  the same loop with one 8-byte gather per (node, slot); besides (sum, count) the node's packed appearance
//                                 cell (count << 24 | sum of u8 intensities) is read once, voted into where -1 <= t < 1, written once.
// Both pairs share their bodies (wmap_value, integrate_node<bool>), so the TSDF fields come out the same bytes either way.
//
// mvs_tsdf_integrate_masked is either pair with rule 1s in the w-map pass (tsdf_wmap_masked_kernel,
// tsdf_wmap_frames_masked_kernel: w = NaN where the slot's support plane is below min_support); with min_support = 0 it launches the
// unmasked kernels.
//
// Arithmetic: f32, one rounding per operation, no contraction (the library builds with -ffp-contract=off; the pixel centres' fmaf is the
// sweep's and is written out); tests/tsdf_mirror.py restates it in numpy, bit for bit.
#include "depth_rules.hpp"
#include "mvs_internal.hpp"
#include "surface_internal.hpp"

#include <cmath>
#include <new>
#include <string>

namespace mvs {

namespace {

constexpr int kTsdfChunk = 16;               // slots per integration launch
constexpr int kTsdfMinG = 16, kTsdfMaxG = 512;
constexpr int kTsdfTX = 64, kTsdfTY = 4;     // integration block: 64 nodes along i x 4 rows along j
constexpr int kTsdfBatch = 8;                // gathers in flight per thread

struct WmapArgs {
    const float *depth[kTsdfChunk];
    const float *cost[kTsdfChunk];           // null unless max_cost is finite
    float Pw[kTsdfChunk][4];                 // row w of P
    float Pi[kTsdfChunk][16];
    float *wmap;                             // the chunk's maps, W*H apart
    int W, H, use_cost;
    float invW, invH, max_cost;
};

struct FrameArgs {
    const uint8_t *raw[kTsdfChunk];          // mvs_tsdf_integrate_frames: the raw frame (frame store) paired with each listed depth slot
};

struct IntegrateArgs {
    const float *wmap;                       // the chunk's w-maps (or 8-byte records), W*H apart, in list order
    float P[kTsdfChunk][12];                 // rows x, y, w of P
    int n, W, H, G;
    float ox, oy, oz, h, halfW, halfH, inv_tau;
};

// contract step 1 for pixel p = (r, c) of the chunk's slot s
__device__ __forceinline__ float wmap_value(const WmapArgs &a, int s, int p, int r, int c)
{
    float w = __builtin_nanf("");
    const float z = a.depth[s][p];
    if (depth_valid(z, a.cost[s], (size_t)p, a.use_cost, a.max_cost)) {
        const float xn = __builtin_fmaf((float)(2 * c + 1), a.invW, -1.0f);
        const float yn = __builtin_fmaf(-(float)(2 * r + 1), a.invH, 1.0f);
        const float ws = prow(a.Pw[s], 0, unproject(a.Pi[s], xn, yn, z));
        if (ws > 0.f) w = ws;
    }
    return w;
}

__global__ __launch_bounds__(256) void tsdf_wmap_kernel(const WmapArgs a)
{
    const int p = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= a.W * a.H) return;
    const int r = p / a.W, c = p - r * a.W;
    a.wmap[(size_t)s * a.W * a.H + p] = wmap_value(a, s, p, r, c);
}

// the same pass with the frame's intensity beside w: a.wmap holds 8-byte records (w, (float bits of) the u8 intensity), so the integration
// loop fetches both with one gather; the frame is read here, coalesced, once per pixel
__global__ __launch_bounds__(256) void tsdf_wmap_frames_kernel(const WmapArgs a, const FrameArgs f)
{
    const int p = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= a.W * a.H) return;
    const int r = p / a.W, c = p - r * a.W;
    const float w = wmap_value(a, s, p, r, c);
    reinterpret_cast<float2 *>(a.wmap)[(size_t)s * a.W * a.H + p] = make_float2(w, __uint_as_float((uint32_t)f.raw[s][p]));
}

// rule 1s in the w-map pass: the two kernels above with the chunk's support planes beside the maps -- a pixel whose
// support is below min_support (> 0 here) has w = NaN, exactly as if its stored depth were the empty value 1.0, so the integration kernels
// do not change.  mvs_tsdf_integrate_masked launches these only for min_support > 0.
struct WmapMask {
    const uint8_t *support[kTsdfChunk];
    int min_support;
};

__global__ __launch_bounds__(256) void tsdf_wmap_masked_kernel(const WmapArgs a, const WmapMask m)
{
    const int p = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= a.W * a.H) return;
    const int r = p / a.W, c = p - r * a.W;
    a.wmap[(size_t)s * a.W * a.H + p] = (int)m.support[s][p] < m.min_support ? __builtin_nanf("") : wmap_value(a, s, p, r, c);
}

__global__ __launch_bounds__(256) void tsdf_wmap_frames_masked_kernel(const WmapArgs a, const FrameArgs f, const WmapMask m)
{
    const int p = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (p >= a.W * a.H) return;
    const int r = p / a.W, c = p - r * a.W;
    const float w = (int)m.support[s][p] < m.min_support ? __builtin_nanf("") : wmap_value(a, s, p, r, c);
    reinterpret_cast<float2 *>(a.wmap)[(size_t)s * a.W * a.H + p] = make_float2(w, __uint_as_float((uint32_t)f.raw[s][p]));
}

// contract steps 2-4 for one node and the chunk's slots in list order.  APP: a.wmap holds tsdf_wmap_frames_kernel's records and the node's
// appearance cell takes the intensity wherever the update falls into the unclamped band -1 <= t < 1 (DESIGN.md section 15 rule B); the
// (sum, count) arithmetic is the same statements either way
template <bool APP>
__device__ __forceinline__ void integrate_node(const IntegrateArgs &a, float *__restrict__ sum, int *__restrict__ count, uint32_t *__restrict__ cells)
{
    const int i = blockIdx.x * kTsdfTX + (int)(threadIdx.x & (kTsdfTX - 1));
    const int j = blockIdx.y * kTsdfTY + __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kTsdfTX));  // (one wave = one row: uniform)
    const int k = blockIdx.z;
    if (i >= a.G || j >= a.G) return;
    const float x = a.ox + a.h * (float)i, y = a.oy + a.h * (float)j, z = a.oz + a.h * (float)k;
    const size_t node = ((size_t)k * a.G + j) * a.G + i;
    const size_t P = (size_t)a.W * a.H;
    float s = sum[node];
    int c = count[node];
    uint32_t cell = 0;
    if (APP) cell = cells[node];
    // kTsdfBatch slots at a time: first every gather of the batch is issued, then the updates run in list order (a slot with nothing to
    // say -- behind the camera, outside the frame, no depth there -- reads as NaN), so a wave waits for one batch of loads, not for each
    for (int e0 = 0; e0 < a.n; e0 += kTsdfBatch) {
        float qw[kTsdfBatch], wd[kTsdfBatch];
        uint32_t in[kTsdfBatch];
#pragma unroll
        for (int b = 0; b < kTsdfBatch; b++) {
            wd[b] = __builtin_nanf("");
            qw[b] = 0.f;
            in[b] = 0;
            if (e0 + b >= a.n) continue;
            const float *M = a.P[e0 + b];
            qw[b] = M[8] * x + ((M[9] * y + M[10] * z) + M[11]);
            if (!(qw[b] > 0.f)) continue;
            const float qx = M[0] * x + ((M[1] * y + M[2] * z) + M[3]);
            const float qy = M[4] * x + ((M[5] * y + M[6] * z) + M[7]);
            const float inv = 1.0f / qw[b];
            const float u = (qx * inv + 1.0f) * a.halfW - 0.5f;
            const float v = (1.0f - qy * inv) * a.halfH - 0.5f;
            const float fc = floorf(u + 0.5f), fr = floorf(v + 0.5f);
            if (!(fc >= 0.f && fc < (float)a.W && fr >= 0.f && fr < (float)a.H)) continue;  // (NaN fails too)
            const size_t at = P * (e0 + b) + (size_t)((int)fr * a.W + (int)fc);
            if (APP) {
                const float2 rec = reinterpret_cast<const float2 *>(a.wmap)[at];
                wd[b] = rec.x;
                in[b] = __float_as_uint(rec.y);
            } else {
                wd[b] = a.wmap[at];
            }
        }
#pragma unroll
        for (int b = 0; b < kTsdfBatch; b++) {
            if (wd[b] != wd[b]) continue;  // NaN: no update
            const float t = (wd[b] - qw[b]) * a.inv_tau;
            if (t >= -1.0f) {
                s = s + (t < 1.0f ? t : 1.0f);
                c = c + 1;
                if (APP && t < 1.0f && cell < 0xFF000000u) cell += 0x01000000u + in[b];  // one vote: count + 1, sum + I (sum <= 255 * 255)
            }
        }
    }
    sum[node] = s;
    count[node] = c;
    if (APP) cells[node] = cell;
}

__global__ __launch_bounds__(256) void tsdf_integrate_kernel(const IntegrateArgs a, float *__restrict__ sum, int *__restrict__ count)
{
    integrate_node<false>(a, sum, count, nullptr);
}

__global__ __launch_bounds__(256) void tsdf_integrate_frames_kernel(const IntegrateArgs a, float *__restrict__ sum, int *__restrict__ count,
                                                                    uint32_t *__restrict__ cells)
{
    integrate_node<true>(a, sum, count, cells);
}

// F = sum / count where count >= min_obs, else 1; mask[node] = 1 when the cell with that low corner has all 8 corners observed enough
__global__ __launch_bounds__(256) void tsdf_field_kernel(int G, const float *__restrict__ sum, const int *__restrict__ count, int min_obs,
                                                         float *__restrict__ F, unsigned char *__restrict__ mask)
{
    const size_t q = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t N3 = (size_t)G * G * G;
    if (q >= N3) return;
    const int i = (int)(q % G), j = (int)((q / G) % G), k = (int)(q / ((size_t)G * G));
    const int c = count[q];
    F[q] = c >= min_obs ? sum[q] / (float)c : 1.0f;
    unsigned char m = 0;
    if (i < G - 1 && j < G - 1 && k < G - 1) {
        m = 1;
#pragma unroll
        for (int d = 0; d < 8; d++)
            if (count[q + (size_t)(d & 1) + (size_t)((d >> 1) & 1) * G + (size_t)(d >> 2) * G * G] < min_obs) m = 0;
    }
    mask[q] = m;
}

}  // namespace

// F and the cell mask for min_obs in ctx->tsdf_work (5 bytes per node).  tsdf_field_key names the min_observations they were made for
// (0: stale -- the volume changed); mvs_tsdf_surface and mvs_tsdf_raycast both come through here, so neither sees the other's field.
int tsdf_ensure_field(mvs_ctx *ctx, int min_obs)
{
    const int G = ctx->tsdf_G;
    const size_t N3 = (size_t)G * G * G;
    const size_t had = ctx->tsdf_work.bytes;
    int rc;
    if ((rc = ensure(ctx, ctx->tsdf_work, 5 * N3))) {
        ctx->tsdf_field_key = ctx->tsdf_brick_key = 0;
        return rc;
    }
    if (ctx->tsdf_work.bytes != had) ctx->tsdf_field_key = ctx->tsdf_brick_key = 0;  // a new buffer
    if (ctx->tsdf_field_key == min_obs) return MVS_OK;
    ctx->tsdf_field_key = ctx->tsdf_brick_key = 0;
    const float *sum = (const float *)ctx->tsdf_vol.ptr;
    float *F = (float *)ctx->tsdf_work.ptr;
    tsdf_field_kernel<<<(unsigned)((N3 + 255) / 256), 256, 0, ctx->stream>>>(G, sum, (const int *)(sum + N3), min_obs, F, (unsigned char *)(F + N3));
    MVS_HIP(ctx, hipGetLastError());
    ctx->tsdf_field_key = min_obs;
    return MVS_OK;
}

// the appearance volume (section 15 rule A): G^3 packed cells, allocated and zeroed when it is first asked for after mvs_tsdf_volume
int tsdf_ensure_appearance(mvs_ctx *ctx)
{
    if (ctx->tsdf_app_have) return MVS_OK;
    const size_t N3 = (size_t)ctx->tsdf_G * ctx->tsdf_G * ctx->tsdf_G;
    int rc;
    if ((rc = ensure(ctx, ctx->tsdf_app, N3 * sizeof(uint32_t)))) return rc;
    MVS_HIP(ctx, hipMemsetAsync(ctx->tsdf_app.ptr, 0, N3 * sizeof(uint32_t), ctx->stream));
    ctx->tsdf_app_have = true;
    return MVS_OK;
}

namespace {

// mvs_tsdf_integrate (frames = false: frame_slots is not looked at), mvs_tsdf_integrate_frames and, with a min_support, mvs_tsdf_integrate_masked
int tsdf_integrate_impl(mvs_ctx *ctx, const char *who, int nslots, const int *slots, const int *frame_slots, bool frames, float max_cost, int min_support = 0)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "%s: null context", who);
    if (!slots || (frames && !frame_slots)) return fail(ctx, MVS_EINVAL, "%s: slots is null", who);
    if (nslots < 1) return fail(ctx, MVS_EINVAL, "%s: nslots %d < 1", who, nslots);
    if (!(max_cost >= 0.f)) return fail(ctx, MVS_EINVAL, "%s: max_cost %g must be >= 0", who, max_cost);
    if (min_support < 0 || min_support > 255) return fail(ctx, MVS_EINVAL, "%s: min_support %d out of range 0..255", who, min_support);
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "%s: no volume (mvs_tsdf_volume first)", who);
    const int cap = (int)ctx->dstore.size();
    for (int e = 0; e < nslots; e++)
        if (slots[e] < 0 || slots[e] >= cap) return fail(ctx, MVS_EINVAL, "%s: slot %d outside the depth store (capacity %d)", who, slots[e], cap);
    for (int e = 0; frames && e < nslots; e++)
        if (frame_slots[e] < 0 || frame_slots[e] >= ctx->store_cap)
            return fail(ctx, MVS_EINVAL, "%s: frame slot %d outside the frame store (capacity %d)", who, frame_slots[e], ctx->store_cap);
    const bool use_cost = max_cost < INFINITY;
    for (int e = 0; e < nslots; e++) {
        const mvs_ctx::DepthSlot &s = ctx->dstore[slots[e]];
        if (!s.have) return fail(ctx, MVS_ESTATE, "%s: slot %d holds no depth map (mvs_depth_upload)", who, slots[e]);
        if (use_cost && !s.have_cost) return fail(ctx, MVS_ESTATE, "%s: max_cost %g is finite but slot %d was stored without a cost map", who, max_cost, slots[e]);
        if (frames && !ctx->store_have[(size_t)frame_slots[e]]) return fail(ctx, MVS_ESTATE, "%s: frame slot %d holds no frame (mvs_frame_upload)", who, frame_slots[e]);
        if (min_support > 0 && !s.have_support)
            return fail(ctx, MVS_ESTATE, "%s: min_support %d > 0 but slot %d has no support plane (mvs_depth_support_upload)", who, min_support, slots[e]);
    }
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H, G = ctx->tsdf_G;
    const size_t P = (size_t)W * H, N3 = (size_t)G * G * G;
    int rc;
    if ((rc = ensure(ctx, ctx->tsdf_wmaps, (size_t)(nslots < kTsdfChunk ? nslots : kTsdfChunk) * P * (frames ? sizeof(float2) : sizeof(float))))) return rc;
    if (frames && (rc = tsdf_ensure_appearance(ctx))) return rc;
    float *wmaps = (float *)ctx->tsdf_wmaps.ptr;
    float *sum = (float *)ctx->tsdf_vol.ptr;
    int *count = (int *)(sum + N3);
    WmapArgs wa;
    FrameArgs fa;
    IntegrateArgs ia;
    WmapMask wm;
    memset(&wm, 0, sizeof(wm));
    wm.min_support = min_support;
    memset(&wa, 0, sizeof(wa));
    memset(&fa, 0, sizeof(fa));
    memset(&ia, 0, sizeof(ia));
    wa.wmap = wmaps;
    wa.W = W;
    wa.H = H;
    wa.use_cost = use_cost ? 1 : 0;
    wa.invW = 1.0f / (float)W;
    wa.invH = 1.0f / (float)H;
    wa.max_cost = max_cost;
    ia.wmap = wmaps;
    ia.W = W;
    ia.H = H;
    ia.G = G;
    ia.ox = ctx->tsdf_origin[0];
    ia.oy = ctx->tsdf_origin[1];
    ia.oz = ctx->tsdf_origin[2];
    ia.h = ctx->tsdf_h;
    ia.halfW = (float)W * 0.5f;
    ia.halfH = (float)H * 0.5f;
    ia.inv_tau = ctx->tsdf_inv_tau;
    const dim3 igrid((unsigned)div_up(G, kTsdfTX), (unsigned)div_up(G, kTsdfTY), (unsigned)G);
    ctx->tsdf_field_key = ctx->tsdf_brick_key = 0;  // the field of the old volume is stale
    ProfileScope ps(ctx, MVS_K_TSDF);
    for (int e0 = 0; e0 < nslots; e0 += kTsdfChunk) {
        const int n = nslots - e0 < kTsdfChunk ? nslots - e0 : kTsdfChunk;
        for (int e = 0; e < n; e++) {
            const int slot = slots[e0 + e];
            const mvs_ctx::DepthSlot &s = ctx->dstore[slot];
            wa.depth[e] = (const float *)ctx->dstore_depth.ptr + P * slot;
            wa.cost[e] = use_cost ? (const float *)ctx->dstore_cost.ptr + P * slot : nullptr;
            memcpy(wa.Pw[e], s.P + 12, 4 * sizeof(float));
            memcpy(wa.Pi[e], s.Pi, sizeof(s.Pi));
            memcpy(ia.P[e], s.P, 8 * sizeof(float));           // rows x, y
            memcpy(ia.P[e] + 8, s.P + 12, 4 * sizeof(float));  // row w
            if (frames) fa.raw[e] = (const uint8_t *)ctx->store_raw.ptr + P * frame_slots[e0 + e];
            if (min_support > 0) wm.support[e] = (const uint8_t *)ctx->dstore_support.ptr + P * slot;
        }
        ia.n = n;
        const dim3 wgrid((unsigned)div_up((int)P, 256), (unsigned)n);
        if (frames) {
            if (min_support > 0) tsdf_wmap_frames_masked_kernel<<<wgrid, 256, 0, ctx->stream>>>(wa, fa, wm);
            else tsdf_wmap_frames_kernel<<<wgrid, 256, 0, ctx->stream>>>(wa, fa);
            MVS_HIP(ctx, hipGetLastError());
            tsdf_integrate_frames_kernel<<<igrid, kTsdfTX * kTsdfTY, 0, ctx->stream>>>(ia, sum, count, (uint32_t *)ctx->tsdf_app.ptr);
        } else {
            if (min_support > 0) tsdf_wmap_masked_kernel<<<wgrid, 256, 0, ctx->stream>>>(wa, wm);
            else tsdf_wmap_kernel<<<wgrid, 256, 0, ctx->stream>>>(wa);
            MVS_HIP(ctx, hipGetLastError());
            tsdf_integrate_kernel<<<igrid, kTsdfTX * kTsdfTY, 0, ctx->stream>>>(ia, sum, count);
        }
        MVS_HIP(ctx, hipGetLastError());
    }
    return MVS_OK;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_tsdf_volume(mvs_ctx *ctx, int nodes_per_axis, const float origin3[3], float node_spacing, float truncation)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_volume: null context");
    if (!origin3) return fail(ctx, MVS_EINVAL, "mvs_tsdf_volume: origin is null");
    const int G = nodes_per_axis;
    if (G < kTsdfMinG || G > kTsdfMaxG) return fail(ctx, MVS_EINVAL, "mvs_tsdf_volume: nodes_per_axis %d out of range %d..%d", G, kTsdfMinG, kTsdfMaxG);
    for (int c = 0; c < 3; c++)
        if (!std::isfinite(origin3[c])) return fail(ctx, MVS_EINVAL, "mvs_tsdf_volume: origin is not finite");
    if (!(node_spacing > 0.f && node_spacing < INFINITY) || !(truncation > 0.f && truncation < INFINITY))
        return fail(ctx, MVS_EINVAL, "mvs_tsdf_volume: node_spacing %g and truncation %g must be finite and > 0", node_spacing, truncation);
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N3 = (size_t)G * G * G;
    ctx->tsdf_G = 0;  // no volume until the new one is allocated and cleared
    ctx->tsdf_field_key = ctx->tsdf_brick_key = 0;
    ctx->tsdf_app_have = false;  // and no appearance: the first mvs_tsdf_integrate_frames / mvs_tsdf_appearance_upload makes a zeroed one
    int rc;
    if ((rc = ensure(ctx, ctx->tsdf_vol, 8 * N3))) return rc;
    MVS_HIP(ctx, hipMemsetAsync(ctx->tsdf_vol.ptr, 0, 8 * N3, ctx->stream));
    ctx->tsdf_G = G;
    for (int c = 0; c < 3; c++) ctx->tsdf_origin[c] = origin3[c];
    ctx->tsdf_h = node_spacing;
    ctx->tsdf_inv_tau = 1.0f / truncation;  // rounded once (contract step 4)
    return MVS_OK;
}

int mvs_tsdf_integrate(mvs_ctx *ctx, int nslots, const int *slots, float max_cost)
{
    return tsdf_integrate_impl(ctx, "mvs_tsdf_integrate", nslots, slots, nullptr, false, max_cost);
}

int mvs_tsdf_integrate_frames(mvs_ctx *ctx, int n, const int *depth_slots, const int *frame_slots, float max_cost)
{
    return tsdf_integrate_impl(ctx, "mvs_tsdf_integrate_frames", n, depth_slots, frame_slots, true, max_cost);
}

int mvs_tsdf_integrate_masked(mvs_ctx *ctx, int n, const int *depth_slots, const int *frame_slots, float max_cost, int min_support)
{
    return tsdf_integrate_impl(ctx, "mvs_tsdf_integrate_masked", n, depth_slots, frame_slots, frame_slots != nullptr, max_cost, min_support);
}

int mvs_tsdf_fetch(mvs_ctx *ctx, float *sdf_sum, int32_t *count)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_fetch: null context");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_fetch: no volume (mvs_tsdf_volume first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N3 = (size_t)ctx->tsdf_G * ctx->tsdf_G * ctx->tsdf_G;
    const float *sum = (const float *)ctx->tsdf_vol.ptr;
    if (sdf_sum) MVS_HIP(ctx, hipMemcpyAsync(sdf_sum, sum, N3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (count) MVS_HIP(ctx, hipMemcpyAsync(count, sum + N3, N3 * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_tsdf_upload(mvs_ctx *ctx, const float *sdf_sum, const int32_t *count)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_upload: null context");
    if (!sdf_sum || !count) return fail(ctx, MVS_EINVAL, "mvs_tsdf_upload: null array");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_upload: no volume (mvs_tsdf_volume first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N3 = (size_t)ctx->tsdf_G * ctx->tsdf_G * ctx->tsdf_G;
    float *sum = (float *)ctx->tsdf_vol.ptr;
    ctx->tsdf_field_key = ctx->tsdf_brick_key = 0;
    MVS_HIP(ctx, hipMemcpyAsync(sum, sdf_sum, N3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    MVS_HIP(ctx, hipMemcpyAsync(sum + N3, count, N3 * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_tsdf_appearance_fetch(mvs_ctx *ctx, uint32_t *cells)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_appearance_fetch: null context");
    if (!cells) return fail(ctx, MVS_EINVAL, "mvs_tsdf_appearance_fetch: cells is null");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_appearance_fetch: no volume (mvs_tsdf_volume first)");
    if (!ctx->tsdf_app_have) return fail(ctx, MVS_ESTATE, "mvs_tsdf_appearance_fetch: no appearance volume (mvs_tsdf_integrate_frames or mvs_tsdf_appearance_upload first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N3 = (size_t)ctx->tsdf_G * ctx->tsdf_G * ctx->tsdf_G;
    MVS_HIP(ctx, hipMemcpyAsync(cells, ctx->tsdf_app.ptr, N3 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_tsdf_appearance_upload(mvs_ctx *ctx, const uint32_t *cells)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_appearance_upload: null context");
    if (!cells) return fail(ctx, MVS_EINVAL, "mvs_tsdf_appearance_upload: cells is null");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_appearance_upload: no volume (mvs_tsdf_volume first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t N3 = (size_t)ctx->tsdf_G * ctx->tsdf_G * ctx->tsdf_G;
    int rc;
    if ((rc = tsdf_ensure_appearance(ctx))) return rc;
    MVS_HIP(ctx, hipMemcpyAsync(ctx->tsdf_app.ptr, cells, N3 * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

int mvs_tsdf_surface(mvs_ctx *ctx, int min_observations, mvs_surface **out)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_surface: null context");
    if (!out) return fail(ctx, MVS_EINVAL, "mvs_tsdf_surface: out is null");
    *out = nullptr;
    if (min_observations < 1) return fail(ctx, MVS_EINVAL, "mvs_tsdf_surface: min_observations %d < 1", min_observations);
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_surface: no volume (mvs_tsdf_volume first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int G = ctx->tsdf_G;
    const size_t N3 = (size_t)G * G * G;
    int rc;
    if ((rc = tsdf_ensure_field(ctx, min_observations))) return rc;
    float *F = (float *)ctx->tsdf_work.ptr;
    unsigned char *mask = (unsigned char *)(F + N3);
    mvs_surface *res = new (std::nothrow) mvs_surface;
    if (!res) return fail(ctx, MVS_ENOMEM, "mvs_tsdf_surface: host allocation failed");
    res->grid.G = G;
    res->grid.ox = ctx->tsdf_origin[0];
    res->grid.oy = ctx->tsdf_origin[1];
    res->grid.oz = ctx->tsdf_origin[2];
    res->grid.h = ctx->tsdf_h;
    res->iso = 0.0f;
    res->spacing = ctx->tsdf_h;
    res->ratio_kept = 1;
    res->support_cells = 0;
    std::string why;
    const int mrc = surface_nets_device(res->grid, F, 0.0f, mask, ctx->stream, res, "mvs_tsdf_surface", why);
    if (mrc != MVS_OK) {
        delete res;
        return fail(ctx, mrc, "%s", why.c_str());
    }
    *out = res;
    return MVS_OK;
}

}  // extern "C"
