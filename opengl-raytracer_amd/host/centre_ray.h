// centre_ray.h -- the primary ray through a pixel's centre, as the CPU statements of the feature pass (host/features.cpp) and of the reprojection
// (host/reproject.cpp) form it: one function, as csrc/features.hip.h's centre_ray is one function for both kernels.  Callers run under MXCSR FTZ | DAZ and are
// compiled with -ffp-contract=off.
#pragma once
#include <cmath>

namespace glrt_detail {

constexpr float kEps = 1.0e-4f;    // PT_EPS: a primary ray's tmin
constexpr float kInfty = 1.0e8f;   // PT_INFTY: its search limit

inline float rsq(float x) { return 1.0f / std::sqrt(x); }

// camera_ray (csrc/pt_kernel.hip.h) at the pixel centre: fcx + r0 = (x + 0.5) + 0.5, the lens offset (lox, loy) = (0, 0) kept in the expressions
inline void centre_ray(const float *C, const float *S, float W, float H, int x, int y, float *ray) {
    const float fcx = (float)x + 0.5f, fcy = (float)y + 0.5f;
    const float nx = ((fcx + 0.5f) / W) * 2.0f + -1.0f;
    const float ny = ((fcy + 0.5f) / H) * 2.0f + -1.0f;
    const float tx = (S[0] * nx + S[12]) + S[4] * ny;
    const float ty = (S[1] * nx + S[13]) + S[5] * ny;
    const float tz = (S[2] * nx + S[14]) + S[6] * ny;
    const float tw = (S[3] * nx + S[15]) + S[7] * ny;
    const float cx = tx / tw, cy = ty / tw, cz = tz / tw;
    const float rn = rsq((cz * cz + cy * cy) + cx * cx);
    const float dx = cx * rn, dy = cy * rn, dz = cz * rn;
    const float lox = 0.0f, loy = 0.0f;
    const float wx = (C[0] * lox + C[12]) + C[4] * loy;
    const float wy = (C[1] * lox + C[13]) + C[5] * loy;
    const float wz = (C[2] * lox + C[14]) + C[6] * loy;
    const float ww = (C[3] * lox + C[15]) + C[7] * loy;
    const float ex = (C[0] * dx + C[4] * dy) + C[8] * dz;
    const float ey = (C[1] * dx + C[5] * dy) + C[9] * dz;
    const float ez = (C[2] * dx + C[6] * dy) + C[10] * dz;
    const float re = rsq((ez * ez + ey * ey) + ex * ex);
    ray[0] = wx / ww; ray[1] = wy / ww; ray[2] = wz / ww; ray[3] = kEps;
    ray[4] = ex * re; ray[5] = ey * re; ray[6] = ez * re; ray[7] = kInfty;
}

}  // namespace glrt_detail
