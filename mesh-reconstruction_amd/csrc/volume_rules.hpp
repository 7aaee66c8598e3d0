// volume_rules.hpp -- where a point falls in the TSDF volume's grid (DESIGN.md section 14 rule 3) as a device function, shared by
// csrc/raycast.hip (the march's samples) and csrc/appearance.hip (the appearance at a point), so both address a cell the same way.
// f32, one rounding per operation (the library builds with -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>

namespace mvs {

// rule 3: cell index clamp(floor(g), 0, G - 2) and fraction clamp(g - (float)i, 0, 1); a NaN gives 0 for both
__device__ __forceinline__ int cell_axis(float g, int G, float &f)
{
    const float fl = floorf(g);
    const int i = fl >= 0.f ? (fl <= (float)(G - 2) ? (int)fl : G - 2) : 0;
    const float r = g - (float)i;
    f = r > 0.f ? (r < 1.f ? r : 1.f) : 0.f;
    return i;
}

}  // namespace mvs
