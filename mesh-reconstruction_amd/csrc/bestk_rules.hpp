// bestk_rules.hpp -- what the best-K kernels (bestk.hip: the plane table or a band around a per-pixel prior; the guide-gated sweep;
// propagate.hip) have in common.  On the device: a cost's window arithmetic (BkCost) and the list of the KMAX smallest per-view costs
// (BkList); DESIGN.md section 22 rules 1-2 are the contract of both.  On the host: the one place where (cost, radius, keep) choose an
// instantiation (with_bestk_shape).  The window elements themselves, zncc_sample and absdiff_sample, are sweep_shared.hpp's.
#pragma once
#include "sweep_shared.hpp"

namespace mvs {

constexpr uint32_t BK_NONE = 0xffffffffu;   // the cost of a view that does not count: above every cost, sinks to the end of the list

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

// host: what the best-K entries (`who`: the two sweeps of bestk.hip, mvs_propagate_init) refuse alike
inline int bestk_arguments(mvs_ctx *ctx, const char *who, int cost, int radius, int keep)
{
    if (cost != MVS_COST_ABSDIFF && cost != MVS_COST_ZNCC) return fail(ctx, MVS_EINVAL, "%s: unknown cost %d", who, cost);
    const int rmin = cost == MVS_COST_ZNCC ? 1 : 0;
    if (radius < rmin || radius > 4) return fail(ctx, MVS_EINVAL, "%s: radius %d outside %d..4", who, radius, rmin);
    if (keep < 0 || keep > 8) return fail(ctx, MVS_EINVAL, "%s: keep %d outside 1..8 and not MVS_KEEP_ALL", who, keep);
    return MVS_OK;
}

// host: calls f(std::integral_constant<int, COST>, <int, R>, <int, KMAX>) for arguments the entry has checked (cost one of the two, radius
// RMIN..4 and not 0 with ZNCC, keep 0..8), so that a launcher names its kernel once.  KMAX is the smallest of 0 (MVS_KEEP_ALL), 2, 4, 8
// that holds `keep`.  ZNCC at radius 0 and the radii below RMIN are never instantiated.
template <int RMIN, class F>
inline void with_bestk_shape(int cost, int radius, int keep, F &&f)
{
    const auto with_kmax = [&](auto c, auto r) {
        if constexpr (decltype(r)::value >= RMIN && !(decltype(c)::value == MVS_COST_ZNCC && decltype(r)::value == 0)) {
            if (keep == MVS_KEEP_ALL)
                f(c, r, std::integral_constant<int, 0>{});
            else if (keep <= 2)
                f(c, r, std::integral_constant<int, 2>{});
            else if (keep <= 4)
                f(c, r, std::integral_constant<int, 4>{});
            else
                f(c, r, std::integral_constant<int, 8>{});
        }
    };
    const auto with_radius = [&](auto c) {
        switch (radius) {
        case 0: with_kmax(c, std::integral_constant<int, 0>{}); break;
        case 1: with_kmax(c, std::integral_constant<int, 1>{}); break;
        case 2: with_kmax(c, std::integral_constant<int, 2>{}); break;
        case 3: with_kmax(c, std::integral_constant<int, 3>{}); break;
        default: with_kmax(c, std::integral_constant<int, 4>{}); break;
        }
    };
    if (cost == MVS_COST_ZNCC)
        with_radius(std::integral_constant<int, MVS_COST_ZNCC>{});
    else
        with_radius(std::integral_constant<int, MVS_COST_ABSDIFF>{});
}

}  // namespace mvs
