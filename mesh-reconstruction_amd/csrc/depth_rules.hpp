// depth_rules.hpp -- fusion rules 1 and 2 (include/mvs.h "depth store + fusion") as device functions: the validity
// test of a stored depth and the back-projection of a pixel.  Shared by csrc/fuse.hip (mvs_fuse_depth) and csrc/tsdf.hip (the w-maps of
// mvs_tsdf_integrate), so both read a stored map the same way.  f32, one rounding per operation (the library builds with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace mvs {

__device__ __forceinline__ bool depth_valid(float z, const float *cost, size_t p, int use_cost, float max_cost)
{
    if (!(z > -1.0f && z < 1.0f)) return false;  // NaN and the empty value 1.0 are out
    return !use_cost || cost[p] <= max_cost;
}

// h = Pi (xn, yn, z, 1), X = h.xyz / h.w
__device__ __forceinline__ float3 unproject(const float *Pi, float xn, float yn, float z)
{
    const float h0 = ((Pi[0] * xn + Pi[1] * yn) + Pi[2] * z) + Pi[3];
    const float h1 = ((Pi[4] * xn + Pi[5] * yn) + Pi[6] * z) + Pi[7];
    const float h2 = ((Pi[8] * xn + Pi[9] * yn) + Pi[10] * z) + Pi[11];
    const float h3 = ((Pi[12] * xn + Pi[13] * yn) + Pi[14] * z) + Pi[15];
    return make_float3(h0 / h3, h1 / h3, h2 / h3);
}

// row i of P (X, 1)
__device__ __forceinline__ float prow(const float *P, int i, float3 X) { return ((P[4 * i] * X.x + P[4 * i + 1] * X.y) + P[4 * i + 2] * X.z) + P[4 * i + 3]; }

}  // namespace mvs
