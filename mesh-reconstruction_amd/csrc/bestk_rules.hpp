// bestk_rules.hpp -- what the two best-K sweeps (bestk.hip: the global plane table; band_bestk.hip: planes in a band around a per-pixel
// prior) have in common on the device: the absolute difference's window element, a cost's window arithmetic (BkCost) and the list of the
// KMAX smallest per-view costs (BkList).  DESIGN.md section 22 rules 1-2 are the contract of all three.
#pragma once
#include "sweep_shared.hpp"

namespace mvs {

constexpr uint32_t BK_NONE = 0xffffffffu;   // the cost of a view that does not count: above every cost, sinks to the end of the list

// band.hip's sample (sweep_fx.hip: sample_global_fx) -> the absolute difference's window element e | ok << 24; a position outside the main
// frame carries NaN in its affine part (zncc_sample)
__device__ __forceinline__ uint32_t absdiff_sample(const Affine &A, float bx, float by, float bw, float z, const uint32_t *__restrict__ quads, uint32_t pitch, float hix,
                                                   float hiy, const uint32_t *__restrict__ lut, uint32_t Im255)
{
    const float sx = __builtin_fmaf(z, bx, A.ax), sy = __builtin_fmaf(z, by, A.ay), sw = __builtin_fmaf(z, bw, A.aw);
    const float r256 = rcp_rn(sw) * 256.0f;
    const float tx = __builtin_fmaf(sx, r256, ZN_MAGIC + 4.0f), ty = __builtin_fmaf(sy, r256, ZN_MAGIC + 4.0f);
    const bool ok = sw > 0.0f && tx > ZN_MAGIC + 132.0f && tx < hix && ty > ZN_MAGIC + 132.0f && ty < hiy;  // false for NaN
    const uint32_t ux = __builtin_bit_cast(uint32_t, tx) & 0x3fffffu, uy = __builtin_bit_cast(uint32_t, ty) & 0x3fffffu;  // t - magic
    const uint32_t quad = quads[ok ? (uy >> 8) * pitch + (ux >> 8) : 0u];   // in frame: column <= W, row <= H of the (H + 2) x pitch quad image
    const uint32_t w = lut[(((uy >> 3) & 31u) << 5) | ((ux >> 3) & 31u)];
    // (the builtin, not inline asm: sweep_fx.hip, sad_u16)
    const uint32_t cell = __builtin_amdgcn_sad_u16(__builtin_amdgcn_udot4(quad, w, 0u, false), Im255, 1u << 24);
    return ok ? cell : 0u;
}

template <int COST>
struct BkCost;

template <>
struct BkCost<MVS_COST_ZNCC> {
    typedef uint4 Elem;
    static __device__ __forceinline__ Elem add(Elem a, Elem b) { return add4(a, b); }
    static __device__ __forceinline__ uint32_t ok(Elem e) { return e.y >> 24; }
    // the window's sums -> the view's cost, BK_NONE if it does not count (zncc_cell: (1 << 24) + c, c <= 65024, or 0)
    static __device__ __forceinline__ uint32_t cost(Elem s, uint32_t centre_ok)
    {
        const uint32_t cell = zncc_cell(s, centre_ok);
        return cell ? cell & 0xffffffu : BK_NONE;
    }
};

template <>
struct BkCost<MVS_COST_ABSDIFF> {
    typedef uint32_t Elem;
    static __device__ __forceinline__ Elem add(Elem a, Elem b) { return a + b; }
    static __device__ __forceinline__ uint32_t ok(Elem e) { return e >> 24; }
    // N << 24 | S -> S / N; the centre is a member of its own window, so N >= 1 wherever the view counts
    static __device__ __forceinline__ uint32_t cost(Elem s, uint32_t centre_ok) { return centre_ok ? (s & 0xffffffu) / max(s >> 24, 1u) : BK_NONE; }
};

// the KMAX smallest costs seen so far, ascending; KMAX = 0: count << 24 | sum of every counted view
template <int KMAX>
struct BkList {
    uint32_t top[KMAX ? KMAX : 1];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < (KMAX ? KMAX : 1); j++) top[j] = KMAX ? BK_NONE : 0u;
    }
    __device__ __forceinline__ void insert(uint32_t c)
    {
        if (KMAX == 0) {
            top[0] += c == BK_NONE ? 0u : (1u << 24) + c;
        } else {
#pragma unroll
            for (int j = 0; j < KMAX; j++) {
                const uint32_t lo = min(top[j], c);
                c = max(top[j], c);
                top[j] = lo;
            }
        }
    }
    // k << 24 | the sum of the k smallest, k = min(keep, counted views); 0 without a counted view
    __device__ __forceinline__ uint32_t cell(int keep) const
    {
        if (KMAX == 0) return top[0];
        uint32_t cell = 0u;
#pragma unroll
        for (int j = 0; j < KMAX; j++) cell += (j < keep && top[j] != BK_NONE) ? (1u << 24) + top[j] : 0u;
        return cell;
    }
};

}  // namespace mvs
