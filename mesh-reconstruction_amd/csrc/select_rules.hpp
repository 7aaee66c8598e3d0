// select_rules.hpp -- the rules of depth selection over packed cells as device functions: the cell layout, the running best plane, a
// cell's mean cost and the sub-plane refinement (oracle/sweep_oracle.c: orc_refine_depth states its arithmetic).  Shared by every kernel
// that writes the depth / cost / index maps (select.hip, the sweep kernels' epilogues, window.hip, aggregate.hip), so that they select
// and refine the same way.  f32, one rounding per operation (the library builds with -ffp-contract=off and every FMA is spelled).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mvs.h"

namespace mvs {

// Cells are  count << CS | sum  with CS = 16 (exact sampler: sum of |u8 - u8|, <= 257 views) or CS = 24 (fixed sampler: sum of
// |weights.texels - 255 I_main|, <= 255 views).
constexpr int CS_EXACT = 16, CS_FIXED = 24;

// HIP declares __umul24 as returning int: compared as such, products >= 2^31 (fixed sampler, > 181 views at maximal cost) would order wrongly
__device__ __forceinline__ uint32_t umul24u(uint32_t a, uint32_t b) { return (uint32_t)__umul24(a, b); }

// running best plane: s/c < bs/bc  <=>  s*bc < bs*c; the products stay below 2^32 (s < 2^16, c < 2^16 or s < 2^24, c < 2^8)
template <int CS = CS_EXACT>
__device__ __forceinline__ void argmin_update(uint32_t cell, int d, uint32_t &bs, uint32_t &bc, int &bi)
{
    const uint32_t s = cell & ((1u << CS) - 1u), c = cell >> CS;  // s < 2^24, c < 2^16: the 24-bit multiplies below are exact
    const bool better = (c != 0u) && (bi < 0 || umul24u(s, bc) < umul24u(bs, c));
    bs = better ? s : bs;
    bc = better ? c : bc;
    bi = better ? d : bi;
}

// the same with the best (count, sum) kept as one packed cell: two registers of state per pixel
template <int CS = CS_EXACT>
__device__ __forceinline__ void argmin_update_packed(uint32_t cell, int d, uint32_t &best, int &bi)
{
    constexpr uint32_t M = (1u << CS) - 1u;
    const uint32_t s = cell & M, c = cell >> CS, bs = best & M, bc = best >> CS;
    const bool better = (c != 0u) && (bi < 0 || umul24u(s, bc) < umul24u(bs, c));
    best = better ? cell : best;
    bi = better ? d : bi;
}

// mean cost in grey levels: sum / count (exact sampler) or sum / (255 count) (fixed sampler: sums are in 1/255 grey levels)
template <int CS = CS_EXACT>
__device__ __forceinline__ float cell_cost(uint32_t bs, uint32_t bc)
{
    return CS == CS_EXACT ? (float)bs / (float)bc : (float)bs / (float)(255u * bc);
}

// sum / count of a cell with count != 0, in the sum's own unit: what the refinement compares (the unit cancels in the parabola)
template <int CS>
__device__ __forceinline__ float cell_mean(uint32_t c)
{
    return (float)(c & ((1u << CS) - 1u)) / (float)(c >> CS);
}

// Sub-plane refinement of the selected plane i: the vertex of the parabola through the costs ca, cb, cc of
// planes i - 1, i, i + 1, at most half a plane step away from z[i]; z[i] itself at the ends of the table and where the three costs do not
// curve upwards.  Whether the neighbours' costs are valid is the caller's test.
__device__ __forceinline__ float refine_parabola(float ca, float cb, float cc, const float *__restrict__ z, int i, int D)
{
    if (!(i > 0 && i < D - 1)) return z[i];
    const float den = (ca - 2.0f * cb) + cc;
    if (!(den > 0.0f)) return z[i];
    float t = (0.5f * (ca - cc)) / den;
    t = t < -0.5f ? -0.5f : (t > 0.5f ? 0.5f : t);
    return t >= 0.0f ? __builtin_fmaf(t, z[i + 1] - z[i], z[i]) : __builtin_fmaf(-t, z[i - 1] - z[i], z[i]);
}

}  // namespace mvs
