// normals_rules.hpp -- rule N1 of DESIGN.md section 31 (include/mvs.h "normals"): a pixel's hypothesis (z, gx, gy) -> the world-space unit
// normal of its plane, turned to the camera's side.  One body for the two kernels that apply it: hypothesis_normals_kernel (normals.hip, the
// propagation's maps) and depth_fit_normals_kernel (depth_fit.hip, the plane fit's maps).  f32, one rounding per operation, no FMA but the
// pixel centres'; tests/normals_mirror.py restates it.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace mvs {

struct NormalCam {
    float P[16];  // the main camera, row-major
    float C[3];   // its centre (slot_matrices)
};

// zeros when the pixel holds no hypothesis or the plane's length is 0, infinite or NaN
__device__ __forceinline__ void rule_n1(const NormalCam &k, int row, int col, float z, float gx, float gy, float invW, float invH, float halfW, float halfH, float &nx,
                                        float &ny, float &nz)
{
    nx = 0.f, ny = 0.f, nz = 0.f;
    if (z > -1.0f && z < 1.0f) {
        const float xn = __builtin_fmaf((float)(2 * col + 1), invW, -1.0f);
        const float yn = __builtin_fmaf(-(float)(2 * row + 1), invH, 1.0f);
        const float a = -gx * halfW, b = gy * halfH;
        const float d = -((z + a * xn) + b * yn);
        float m[4];
        for (int c = 0; c < 4; c++) m[c] = ((a * k.P[c] + b * k.P[4 + c]) + k.P[8 + c]) + d * k.P[12 + c];
        const float len = sqrtf((m[0] * m[0] + m[1] * m[1]) + m[2] * m[2]);
        if (len > 0.f && len < INFINITY) {
            nx = m[0] / len;
            ny = m[1] / len;
            nz = m[2] / len;
            if (((m[0] * k.C[0] + m[1] * k.C[1]) + m[2] * k.C[2]) + m[3] < 0.f) {
                nx = -nx;
                ny = -ny;
                nz = -nz;
            }
        }
    }
}

}  // namespace mvs
