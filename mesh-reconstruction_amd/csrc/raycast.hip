// raycast.hip -- ray-cast of the TSDF volume (include/mvs.h "ray-cast of the TSDF volume"): the zero level set of the
// averaged field as a depth map and a normal map of any camera, from the volume itself -- sub-voxel depth by trilinear interpolation,
// normals from the interpolant's gradient, nothing leaves HBM.
//
// mvs_tsdf_raycast queues up to three launches on ctx->stream:
//   tsdf_field_kernel     (tsdf.hip, through tsdf_ensure_field) F and the cell mask for this call's min_observations, unless they are
//                         there already: the field is kept until the volume changes
//   tsdf_brick_kernel     one bit per brick of 8^3 cells: set when the brick holds a masked cell at which a sample can come out <= 0
//                         (brick_cell_flag below); one workgroup per 32-bit word of the mask, no atomics; kept like the field
//   tsdf_raycast_kernel   one ray per lane, a wavefront is an 8 x 8 pixel tile (a compact bundle: its 8 corner gathers land on a few
//                         lines), a workgroup 16 x 16 pixels.  The sample position comes from the product t_in + delta k, the previous
//                         sample is carried in registers, a lane leaves the loop at its hit.  With the brick mask (copied into LDS by every
//                         workgroup) a sample whose brick bit is clear costs one LDS read instead of 9 gathers; the samples that are
//                         evaluated, and so every output bit, are the plain march's: see the comment at the loop.
//
// Arithmetic: f32, one rounding per operation, no contraction (-ffp-contract=off); tests/raycast_mirror.py restates it in numpy, bit for bit.
#include "depth_rules.hpp"
#include "mvs_internal.hpp"
#include "volume_rules.hpp"   // rule 3's cell_axis

#include <cmath>

namespace mvs {

namespace {

constexpr int kRayTile = 16;    // workgroup: 16 x 16 pixels = 4 wavefronts of 8 x 8
constexpr int kBrickShift = 3;  // a brick is 8^3 cells

struct RayArgs {
    float P[16], Pi[16];
    float C[3], o[3], hi[3];
    float inv_h, delta, invW, invH;
    int G, W, H, kmax;
    int nb, nwx;                 // bricks per axis; 32-bit words per brick row
    const float *F;
    const unsigned char *mask;
    const uint32_t *bricks;
    float *depth, *normals;
};

struct Cell {
    int ix, iy, iz, base;
    float fx, fy, fz;
};

__device__ __forceinline__ float3 ray_point(const RayArgs &a, float3 d, float t) { return make_float3(a.C[0] + t * d.x, a.C[1] + t * d.y, a.C[2] + t * d.z); }

__device__ __forceinline__ Cell locate(const RayArgs &a, float3 X)
{
    Cell c;
    c.ix = cell_axis((X.x - a.o[0]) * a.inv_h, a.G, c.fx);
    c.iy = cell_axis((X.y - a.o[1]) * a.inv_h, a.G, c.fy);
    c.iz = cell_axis((X.z - a.o[2]) * a.inv_h, a.G, c.fz);
    c.base = (c.iz * a.G + c.iy) * a.G + c.ix;   // < 2^27 at G = 512
    return c;
}

__device__ __forceinline__ float lerp1(float a, float b, float f) { return a + f * (b - a); }

// the cell's 8 corners, c[dk * 4 + dj * 2 + di] (the cell index is at most G - 2 on every axis: all 8 lie inside the volume)
__device__ __forceinline__ void corners(const RayArgs &a, const Cell &c, float v[8])
{
    const float *q = a.F + c.base;
    const int G = a.G, GG = a.G * a.G;
    v[0] = q[0];
    v[1] = q[1];
    v[2] = q[G];
    v[3] = q[G + 1];
    v[4] = q[GG];
    v[5] = q[GG + 1];
    v[6] = q[GG + G];
    v[7] = q[GG + G + 1];
}

// rule 3: the sample at X: valid (the cell's mask) and the trilinear value, lerps along i, then j, then k
__device__ __forceinline__ bool sample(const RayArgs &a, float3 X, float &value)
{
    const Cell c = locate(a, X);
    const unsigned char m = a.mask[c.base];
    float v[8];
    corners(a, c, v);
    const float c00 = lerp1(v[0], v[1], c.fx), c10 = lerp1(v[2], v[3], c.fx), c01 = lerp1(v[4], v[5], c.fx), c11 = lerp1(v[6], v[7], c.fx);
    value = lerp1(lerp1(c00, c10, c.fy), lerp1(c01, c11, c.fy), c.fz);
    return m != 0;
}

// A masked cell is flagged when a sample inside it can come out <= 0.  "Some corner <= 0" alone is not that test: a + f (b - a) with
// a, b > 0 rounds to 0 when f = 1 and b is below half an ulp of a (b - a rounds to -a).  With every corner in [m, M], m > 0, one lerp
// of values in [m', M'] is at least m' - M' (2u + u^2) before its last rounding (u = 2^-24: one rounding of the difference, one of the
// product) and at most M' (1 + 3u), so the three stages give at least m - 6.1 u M > 0 whenever m > 2^-21 M.  The test below keeps a
// factor 2 on that and an absolute floor of 2^-100 (below it products underflow); any corner that is NaN, infinite or <= 0 flags the cell.
__device__ __forceinline__ bool brick_cell_flag(const float v[8])
{
    bool pos = true;
    float m = v[0], M = 0.f;
#pragma unroll
    for (int d = 0; d < 8; d++) {
        pos = pos && (v[d] > 0.f);
        m = v[d] < m ? v[d] : m;
        const float av = fabsf(v[d]);
        M = av > M ? av : M;
    }
    float bound = M * 9.5367431640625e-07f;   // 2^-20 M
    if (!(bound > 7.888609052210118e-31f)) bound = 7.888609052210118e-31f;   // 2^-100
    return !pos || !(m > bound);
}

// one workgroup per 32-bit word of the brick mask: word (bz, by, wx) holds bricks bx = 32 wx .. 32 wx + 31 of row (by, bz); each of the 4
// wavefronts takes 8 of them in turn, a lane one (i, j) column of the brick's 8 x 8 x 8 cells
__global__ __launch_bounds__(256) void tsdf_brick_kernel(int G, int nb, int nwx, const float *__restrict__ F, const unsigned char *__restrict__ mask,
                                                         uint32_t *__restrict__ bricks)
{
    __shared__ uint32_t part[4];
    const int word = blockIdx.x;
    const int wx = word % nwx, by = (word / nwx) % nb, bz = word / (nwx * nb);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int GG = G * G;
    uint32_t bits = 0;
    for (int b = 0; b < 8; b++) {
        const int bx = wx * 32 + wave * 8 + b;
        if (bx >= nb) break;
        const int ix = (bx << kBrickShift) + (lane & 7), iy = (by << kBrickShift) + (lane >> 3);
        bool any = false;
        for (int lk = 0; lk < 8 && !any; lk++) {
            const int iz = (bz << kBrickShift) + lk;
            bool flag = false;
            if (ix <= G - 2 && iy <= G - 2 && iz <= G - 2) {
                const int base = (iz * G + iy) * G + ix;
                if (mask[base]) {
                    const float *q = F + base;
                    const float v[8] = {q[0], q[1], q[G], q[G + 1], q[GG], q[GG + 1], q[GG + G], q[GG + G + 1]};
                    flag = brick_cell_flag(v);
                }
            }
            any = __ballot(flag) != 0ull;
        }
        if (any) bits |= 1u << (wave * 8 + b);
    }
    if (lane == 0) part[wave] = bits;
    __syncthreads();
    if (threadIdx.x == 0) bricks[word] = part[0] | part[1] | part[2] | part[3];
}

template <bool SKIP>
__device__ __forceinline__ bool cast_ray(const RayArgs &a, const uint32_t *s_bricks, int row, int col, float &zout, float3 &nout)
{
    // rule 1: the pixel's ray
    const float xn = __builtin_fmaf((float)(2 * col + 1), a.invW, -1.0f);
    const float yn = __builtin_fmaf(-(float)(2 * row + 1), a.invH, 1.0f);
    const float3 X1 = unproject(a.Pi, xn, yn, 0.0f);
    if (!(prow(a.P, 3, X1) > 0.f)) return false;
    float3 d = make_float3(X1.x - a.C[0], X1.y - a.C[1], X1.z - a.C[2]);
    const float len = sqrtf((d.x * d.x + d.y * d.y) + d.z * d.z);
    if (!(len > 0.f && len < INFINITY)) return false;
    d = make_float3(d.x / len, d.y / len, d.z / len);
    // rule 2: the box
    float t_in = 0.f, t_out = INFINITY;
    const float dd[3] = {d.x, d.y, d.z};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        if (dd[c] != 0.f) {
            const float t1 = (a.o[c] - a.C[c]) / dd[c], t2 = (a.hi[c] - a.C[c]) / dd[c];
            const float tn = t1 < t2 ? t1 : t2, tf = t1 < t2 ? t2 : t1;
            if (tn > t_in) t_in = tn;
            if (tf < t_out) t_out = tf;
        } else if (!(a.o[c] <= a.C[c] && a.C[c] <= a.hi[c])) {
            return false;
        }
    }
    if (!(t_in <= t_out)) return false;
    // rules 3 and 4.  A hit at k needs sample k valid and <= 0 and sample k - 1 valid and > 0.  A sample in a brick whose bit is clear is
    // either invalid or > 0 (brick_cell_flag), so it cannot be the current sample of a hit and is not evaluated; it can still be the
    // previous one, so when an evaluated sample is valid and <= 0 and its predecessor was passed over, the predecessor is evaluated then.
    // A sample's value depends on k alone: the march with the mask sees exactly the values the plain march sees wherever they matter.
    bool prev_known = false, prev_ok = false;
    float prev_F = 0.f, t_prev = t_in;
    float t_hit = 0.f;
    bool hit = false;
    for (int k = 0; k <= a.kmax; k++) {
        const float t = t_in + a.delta * (float)k;
        if (!(t <= t_out)) break;
        const float3 X = ray_point(a, d, t);
        float Fk;
        bool ok;
        if (SKIP) {
            const Cell c = locate(a, X);
            const int bx = c.ix >> kBrickShift, by = c.iy >> kBrickShift, bz = c.iz >> kBrickShift;
            if (!((s_bricks[(bz * a.nb + by) * a.nwx + (bx >> 5)] >> (bx & 31)) & 1u)) {
                prev_known = false;
                t_prev = t;
                continue;
            }
        }
        ok = sample(a, X, Fk);
        if (k >= 1 && ok && Fk <= 0.f) {
            if (SKIP && !prev_known) prev_ok = sample(a, ray_point(a, d, t_prev), prev_F);
            if (prev_ok && prev_F > 0.f) {
                t_hit = t_prev + a.delta * (prev_F / (prev_F - Fk));
                hit = true;
                break;
            }
        }
        prev_known = true;
        prev_ok = ok;
        prev_F = Fk;
        t_prev = t;
    }
    if (!hit) return false;
    // rule 5: depth and normal at the crossing
    const float3 Xs = ray_point(a, d, t_hit);
    const Cell c = locate(a, Xs);
    if (!a.mask[c.base]) return false;
    float v[8];
    corners(a, c, v);
    const float gx = lerp1(lerp1(v[1] - v[0], v[3] - v[2], c.fy), lerp1(v[5] - v[4], v[7] - v[6], c.fy), c.fz);
    const float gy = lerp1(lerp1(v[2] - v[0], v[3] - v[1], c.fx), lerp1(v[6] - v[4], v[7] - v[5], c.fx), c.fz);
    const float gz = lerp1(lerp1(v[4] - v[0], v[5] - v[1], c.fx), lerp1(v[6] - v[2], v[7] - v[3], c.fx), c.fy);
    const float gl = sqrtf((gx * gx + gy * gy) + gz * gz);
    if (!(gl > 0.f && gl < INFINITY)) return false;
    const float z = prow(a.P, 2, Xs) / prow(a.P, 3, Xs);
    if (!(z > -1.0f && z < 1.0f)) return false;
    zout = z;
    nout = make_float3(gx / gl, gy / gl, gz / gl);
    return true;
}

template <bool SKIP>
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const RayArgs a)
{
    extern __shared__ uint32_t s_bricks[];
    if (SKIP) {
        const int nw = a.nb * a.nb * a.nwx;
        for (int w = threadIdx.x; w < nw; w += 256) s_bricks[w] = a.bricks[w];
        __syncthreads();
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int col = blockIdx.x * kRayTile + (wave & 1) * 8 + (lane & 7);
    const int row = blockIdx.y * kRayTile + (wave >> 1) * 8 + (lane >> 3);
    if (col >= a.W || row >= a.H) return;
    float z = 1.0f;
    float3 n = make_float3(0.f, 0.f, 0.f);
    if (!cast_ray<SKIP>(a, s_bricks, row, col, z, n)) {   // (empty: the values above, whatever the ray had reached)
        z = 1.0f;
        n = make_float3(0.f, 0.f, 0.f);
    }
    const size_t p = (size_t)row * a.W + col;
    a.depth[p] = z;
    a.normals[3 * p] = n.x;
    a.normals[3 * p + 1] = n.y;
    a.normals[3 * p + 2] = n.z;
}

}  // namespace

}  // namespace mvs

using namespace mvs;

extern "C" {

int mvs_tsdf_raycast(mvs_ctx *ctx, const float cam[16], int min_observations, float step_nodes)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_raycast: null context");
    if (!cam) return fail(ctx, MVS_EINVAL, "mvs_tsdf_raycast: cam is null");
    if (min_observations < 1) return fail(ctx, MVS_EINVAL, "mvs_tsdf_raycast: min_observations %d < 1", min_observations);
    if (!(step_nodes >= 0.0625f && step_nodes <= 4.0f)) return fail(ctx, MVS_EINVAL, "mvs_tsdf_raycast: step_nodes %g outside 1/16 .. 4", step_nodes);
    mvs_ctx::DepthSlot s;
    if (!slot_matrices(cam, s)) return fail(ctx, MVS_EINVAL, "mvs_tsdf_raycast: the camera is not finite, is singular or has no finite centre");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_raycast: no volume (mvs_tsdf_volume first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const int W = ctx->W, H = ctx->H, G = ctx->tsdf_G;
    const size_t N3 = (size_t)G * G * G, P = (size_t)W * H;
    int rc;
    if ((rc = ensure(ctx, ctx->ray_depth, P * sizeof(float)))) return rc;
    if ((rc = ensure(ctx, ctx->ray_normals, 3 * P * sizeof(float)))) return rc;
    RayArgs a;
    memset(&a, 0, sizeof(a));
    memcpy(a.P, s.P, sizeof(a.P));
    memcpy(a.Pi, s.Pi, sizeof(a.Pi));
    for (int c = 0; c < 3; c++) {
        a.C[c] = s.C[c];
        a.o[c] = ctx->tsdf_origin[c];
        a.hi[c] = ctx->tsdf_origin[c] + ctx->tsdf_h * (float)(G - 1);
    }
    a.inv_h = 1.0f / ctx->tsdf_h;
    a.delta = step_nodes * ctx->tsdf_h;
    a.invW = 1.0f / (float)W;
    a.invH = 1.0f / (float)H;
    a.G = G;
    a.W = W;
    a.H = H;
    a.kmax = (int)std::floor(1.75 * (double)(G - 1) / (double)step_nodes) + 2;  // bounds the loop even when t_in + delta k stops growing
    a.nb = div_up(G - 1, 1 << kBrickShift);
    a.nwx = div_up(a.nb, 32);
    const int nwords = a.nb * a.nb * a.nwx;   // at most 64 * 64 * 2 words = 32 KiB
    const bool skip = !ctx->ray_plain;
    const size_t had = ctx->tsdf_bricks.bytes;
    if (skip && (rc = ensure(ctx, ctx->tsdf_bricks, (size_t)nwords * sizeof(uint32_t)))) return rc;
    if (ctx->tsdf_bricks.bytes != had) ctx->tsdf_brick_key = 0;  // a new buffer
    ProfileScope ps(ctx, MVS_K_TSDF);
    if ((rc = tsdf_ensure_field(ctx, min_observations))) return rc;
    a.F = (const float *)ctx->tsdf_work.ptr;
    a.mask = (const unsigned char *)(a.F + N3);
    a.bricks = (const uint32_t *)ctx->tsdf_bricks.ptr;
    a.depth = (float *)ctx->ray_depth.ptr;
    a.normals = (float *)ctx->ray_normals.ptr;
    if (skip && ctx->tsdf_brick_key != min_observations) {
        ctx->tsdf_brick_key = 0;
        tsdf_brick_kernel<<<(unsigned)nwords, 256, 0, ctx->stream>>>(G, a.nb, a.nwx, a.F, a.mask, (uint32_t *)ctx->tsdf_bricks.ptr);
        MVS_HIP(ctx, hipGetLastError());
        ctx->tsdf_brick_key = min_observations;
    }
    const dim3 grid((unsigned)div_up(W, kRayTile), (unsigned)div_up(H, kRayTile));
    if (skip)
        tsdf_raycast_kernel<true><<<grid, 256, (size_t)nwords * sizeof(uint32_t), ctx->stream>>>(a);
    else
        tsdf_raycast_kernel<false><<<grid, 256, 0, ctx->stream>>>(a);
    MVS_HIP(ctx, hipGetLastError());
    ctx->ray_have = true;
    return MVS_OK;
}

void *mvs_tsdf_raycast_depth_device(mvs_ctx *ctx) { return ctx && ctx->ray_have ? ctx->ray_depth.ptr : nullptr; }
void *mvs_tsdf_raycast_normals_device(mvs_ctx *ctx) { return ctx && ctx->ray_have ? ctx->ray_normals.ptr : nullptr; }

int mvs_tsdf_raycast_fetch(mvs_ctx *ctx, float *depth_hw, float *normals_hw3)
{
    if (!ctx) return fail(nullptr, MVS_EINVAL, "mvs_tsdf_raycast_fetch: null context");
    if (!ctx->tsdf_G) return fail(ctx, MVS_ESTATE, "mvs_tsdf_raycast_fetch: no volume (mvs_tsdf_volume first)");
    if (!ctx->ray_have) return fail(ctx, MVS_ESTATE, "mvs_tsdf_raycast_fetch: no raycast yet (mvs_tsdf_raycast first)");
    MVS_HIP(ctx, hipSetDevice(ctx->device));
    const size_t P = (size_t)ctx->W * ctx->H;
    if (depth_hw) MVS_HIP(ctx, hipMemcpyAsync(depth_hw, ctx->ray_depth.ptr, P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    if (normals_hw3) MVS_HIP(ctx, hipMemcpyAsync(normals_hw3, ctx->ray_normals.ptr, 3 * P * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    MVS_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return MVS_OK;
}

// test hook, not part of mvs.h: 1 = march without the brick mask (the plain kernel: tools/time_raycast.py's A/B, the tests' cross-check)
int mvs_test_raycast_plain(mvs_ctx *ctx, int plain)
{
    if (!ctx) return MVS_EINVAL;
    ctx->ray_plain = plain != 0;
    return MVS_OK;
}

}  // extern "C"
