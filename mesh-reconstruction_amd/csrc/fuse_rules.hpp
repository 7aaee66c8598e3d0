// fuse_rules.hpp -- the per-pixel contract of the depth-map fusion (include/mvs.h "depth store + fusion", DESIGN.md sections 11 and 28) as
// device functions: ref_point (rules 1 / 1s and 2 for a reference pixel), tangent (the normal's two axes) and fuse_pixel (rules 3 to 5).
// Shared by csrc/fuse.hip (mvs_fuse_depth, mvs_fuse_depth_masked), csrc/fuse_sequence.hip (mvs_fuse_sequence) and csrc/normals.hip
// (mvs_fuse_depth_normals), so that all of them compile the same statements.  The functions are templates over the argument block: FuseArgs
// reads rule 1, FuseMaskedArgs adds the support planes of rule 1s, FuseNormalArgs the normal planes of rules 3n and 5n (section 31)
// (`if constexpr`: the kernels of the smaller blocks hold no trace of the larger ones').  f32, one rounding per operation (-ffp-contract=off).
#pragma once

#include "depth_rules.hpp"
#include "mvs_internal.hpp"

#include <cmath>
#include <cstdint>

namespace mvs {

constexpr int kFuseMaxNeighbours = 16;
constexpr int kFuseTX = 64, kFuseTY = 4;  // tile = 4 wave-wide rows

// Everything the kernels read besides the maps: passed by value, so the matrices sit in the kernel-argument segment and every lane reads
// them with the same (scalar) loads.  Index 0 is the reference view, 1..K the neighbours in the caller's order.
struct FuseArgs {
    static constexpr bool kMasked = false;
    static constexpr bool kNormals = false;
    const float *depth[kFuseMaxNeighbours + 1];
    const float *cost[kFuseMaxNeighbours + 1];  // null unless the cost threshold is finite
    float P[kFuseMaxNeighbours + 1][16];
    float Pi[kFuseMaxNeighbours + 1][16];
    float C[3];                                 // reference camera centre
    int W, H, K, min_consistent, ntx, use_cost;
    float invW, invH, halfW, halfH, max_reproj2, max_rel, max_cost;
};

// rule 1s: the support plane of every view beside its maps (null while min_support is 0: the planes are not read then)
struct FuseMaskedArgs : FuseArgs {
    static constexpr bool kMasked = true;
    const uint8_t *support[kFuseMaxNeighbours + 1];
    int min_support;
};

// rules 3n / 5n: the normal plane (H*W*3 f32, interleaved) of every view that has one (null: none) and the least cosine of rule 3n
struct FuseNormalArgs : FuseMaskedArgs {
    static constexpr bool kNormals = true;
    const float *normals[kFuseMaxNeighbours + 1];
    float min_cos;
};

// section 31: the stored normal of pixel p of view j and whether it is usable (false for no plane, zeros, NaN and infinities)
template <class A>
__device__ __forceinline__ bool stored_normal(const A &a, int j, size_t p, float &x, float &y, float &z)
{
    const float *n = a.normals[j];
    if (!n) return false;
    x = n[3 * p];
    y = n[3 * p + 1];
    z = n[3 * p + 2];
    const float s = (x * x + y * y) + z * z;
    return s > 0.5f && s < 2.0f;
}

// rule 1 / rule 1s for pixel p of view j
template <class A>
__device__ __forceinline__ bool stored_valid(const A &a, int j, float z, size_t p)
{
    if (!depth_valid(z, a.cost[j], p, a.use_cost, a.max_cost)) return false;
    if constexpr (A::kMasked) {
        if (a.min_support > 0 && (int)a.support[j][p] < a.min_support) return false;
    }
    return true;
}

// (x, y, z, w_r) of reference pixel (r, c); w = 0 marks a pixel that is not valid (rule 1 / 1s, or w_r <= 0)
template <class A>
__device__ __forceinline__ float4 ref_point(const A &a, int r, int c)
{
    const size_t p = (size_t)r * a.W + c;
    const float z = a.depth[0][p];
    if (!stored_valid(a, 0, z, p)) return make_float4(0.f, 0.f, 0.f, 0.f);
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

// rule 3's pixel of X in neighbour j, false when X is behind that camera or projects outside its frame: the first statements of fuse_pixel's
// vote loop again, for the claims of the sequence fusion (the loop keeps them written out: the row kernel's registers)
template <class A>
__device__ __forceinline__ bool vote_pixel(const A &a, int j, float3 X, int &rj, int &cj)
{
    const float qw = prow(a.P[j], 3, X);
    if (!(qw > 0.f)) return false;
    const float u = (prow(a.P[j], 0, X) / qw + 1.0f) * a.halfW - 0.5f;
    const float v = (1.0f - prow(a.P[j], 1, X) / qw) * a.halfH - 0.5f;
    const float fc = floorf(u + 0.5f), fr = floorf(v + 0.5f);
    if (!(fc >= 0.f && fc < (float)a.W && fr >= 0.f && fr < (float)a.H)) return false;
    cj = (int)fc;
    rj = (int)fr;
    return true;
}

// the whole per-pixel contract; tile holds ref_point of the tile plus a one-pixel halo, (ty, tx) is this pixel's entry.  agreed: bit j - 1
// is set for every listed neighbour j that agreed in rule 3 (a caller that does not look at it pays nothing for it)
template <class A>
__device__ __forceinline__ bool fuse_pixel(const A &a, const float4 (*tile)[kFuseTX + 2], int ty, int tx, int row, int col, float out[7], unsigned &agreed)
{
    agreed = 0u;
    const float4 c = tile[ty][tx];
    if (!(c.w > 0.f)) return false;
    float nx, ny, nz;
    [[maybe_unused]] bool have_nr = false;   // rule 5n: the reference pixel's stored normal is usable (rx, ry, rz)
    [[maybe_unused]] float rx = 0.f, ry = 0.f, rz = 0.f;
    if constexpr (A::kNormals) have_nr = stored_normal(a, 0, (size_t)row * a.W + col, rx, ry, rz);
    if (!have_nr) {
        // normal from the reference map alone (before the votes: a pixel without one is dropped anyway)
        float3 tc, tr;
        if (!tangent(tile[ty][tx - 1], c, tile[ty][tx + 1], a.max_rel, tc)) return false;
        if (!tangent(tile[ty - 1][tx], c, tile[ty + 1][tx], a.max_rel, tr)) return false;
        nx = tc.y * tr.z - tc.z * tr.y;
        ny = tc.z * tr.x - tc.x * tr.z;
        nz = tc.x * tr.y - tc.y * tr.x;
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
    } else {
        nx = rx;   // the sum of rule 5n starts at n_r
        ny = ry;
        nz = rz;
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
        if (!stored_valid(a, j, zj, p)) continue;
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
        if constexpr (A::kNormals) {   // rule 3n, then the voter's share of rule 5n's sum
            float jx, jy, jz;
            if (have_nr && stored_normal(a, j, p, jx, jy, jz)) {
                if (!((rx * jx + ry * jy) + rz * jz >= a.min_cos)) continue;
                nx = nx + jx;
                ny = ny + jy;
                nz = nz + jz;
            }
        }
        sx = sx + Xj.x;
        sy = sy + Xj.y;
        sz = sz + Xj.z;
        agree++;
        agreed |= 1u << (j - 1);
    }
    if (agree < a.min_consistent) return false;
    if constexpr (A::kNormals) {
        if (have_nr) {   // rule 5n: the summed normals over their length, turned to the camera by rule 5's test
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
        }
    }
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

// the tile of fuse_pixel: ref_point of the 64 x 4 pixels at (row0, col0) plus a one-pixel halo, zero outside the image; 256 threads
template <class A>
__device__ __forceinline__ void fuse_load_tile(const A &a, float4 (*tile)[kFuseTX + 2], int row0, int col0)
{
    for (int e = threadIdx.x; e < (kFuseTY + 2) * (kFuseTX + 2); e += kFuseTX * kFuseTY) {
        const int er = e / (kFuseTX + 2), ec = e - er * (kFuseTX + 2);
        const int r = row0 + er - 1, c = col0 + ec - 1;
        tile[er][ec] = (r >= 0 && r < a.H && c >= 0 && c < a.W) ? ref_point(a, r, c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    __syncthreads();
}

// One 64 x 4 tile of the order-preserving compaction (fuse.hip's head comment).  WRITE = false: keep count per segment (row * ntx + tile
// column) and counts[H * ntx] = 0; WRITE = true: rows at the scanned offsets.  A = FuseArgs: mvs_fuse_depth; A = FuseMaskedArgs:
// mvs_fuse_depth_masked with min_support > 0 (rule 1s); A = FuseNormalArgs: mvs_fuse_depth_normals (rules 3n, 5n)
template <bool WRITE, class A>
__device__ __forceinline__ void fuse_body(const A &a, int *__restrict__ counts, const int *__restrict__ offsets, float *__restrict__ rows)
{
    __shared__ float4 tile[kFuseTY + 2][kFuseTX + 2];
    const int tx = threadIdx.x & (kFuseTX - 1), ty = threadIdx.x / kFuseTX;
    const int col0 = blockIdx.x * kFuseTX, row0 = blockIdx.y * kFuseTY;
    fuse_load_tile(a, tile, row0, col0);
    const int row = row0 + ty, col = col0 + tx;
    float out[7];
    unsigned agreed;
    const bool keep = row < a.H && col < a.W && fuse_pixel(a, tile, ty + 1, tx + 1, row, col, out, agreed);
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

// the host half shared by the three entry points (fuse.hip): the checks of one (reference, neighbours) list against the depth store and
// the thresholds, and the argument block of one reference
int fuse_check_thresholds(mvs_ctx *ctx, const char *who, int nneighbours, const int *neighbour_slots, int min_consistent, float max_reproj_px, float max_rel_depth, float max_cost, int min_support);
int fuse_check_slots(mvs_ctx *ctx, const char *who, int ref_slot, int n, const int *slots, float max_cost, int min_support);
void fuse_fill_args(mvs_ctx *ctx, FuseMaskedArgs &a, int ref_slot, int n, const int *slots, int min_consistent, float max_reproj_px, float max_rel_depth,
                    float max_cost, int min_support);

}  // namespace mvs
