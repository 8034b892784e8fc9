// reproject_setup.h -- what the host computes once per reprojection, as source that both libraries compile (glrtx_reproject / glrtx_debug_reproject in
// csrc/glrtx.hip, glrt_reproject in host/reproject.cpp): the inverses of the previous camera's matrices, by the host library's own routine
// (host/mat4_inverse.h), the previous camera's origin by centre_ray's expressions, and the configuration's ranges.  The origin's five operations flush
// denormal operands and results by hand, so that the value does not depend on the caller's denormal mode.
#pragma once
#include <cstdint>
#include <cstring>

#include "mat4_inverse.h"

namespace glrt_detail {

inline float flush(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    if ((b & 0x7F800000u) == 0u) { b &= 0x80000000u; std::memcpy(&x, &b, 4); }
    return x;
}

struct ReprojectSetup {
    float W[16], S[16];  // inverse(c2w_prev), inverse(s2c_prev)
    float o_prev[3];     // centre_ray's origin for the previous camera: (C[0] * 0 + C[12 + k]) + C[4] * 0 per row, divided by the w row
    float max_history, depth_tolerance, normal_tolerance;  // max_history as a float; the tolerances with denormals flushed
};

// 0, or which argument is refused: 1 max_history < 1, 2 depth_tolerance not a positive finite number, 3 normal_tolerance not finite, 4 / 5 c2w_prev / s2c_prev singular
inline int reproject_setup(const float *c2w_prev, const float *s2c_prev, int max_history, float depth_tolerance, float normal_tolerance, ReprojectSetup &out) {
    if (max_history < 1) return 1;
    if (!(depth_tolerance > 0.0f) || !(depth_tolerance <= 3.4028234663852886e38f)) return 2;
    if (!(normal_tolerance >= -3.4028234663852886e38f && normal_tolerance <= 3.4028234663852886e38f)) return 3;
    if (mat4_inverse(c2w_prev, out.W) != GLRT_HOST_OK) return 4;
    if (mat4_inverse(s2c_prev, out.S) != GLRT_HOST_OK) return 5;
    const float *C = c2w_prev;
    float w[4];
    for (int k = 0; k < 4; k++) w[k] = flush(flush(flush(flush(C[k]) * 0.0f) + flush(C[12 + k])) + flush(flush(C[4 + k]) * 0.0f));
    for (int k = 0; k < 3; k++) out.o_prev[k] = flush(w[k] / w[3]);
    out.max_history = (float)max_history;
    out.depth_tolerance = flush(depth_tolerance);
    out.normal_tolerance = flush(normal_tolerance);
    return 0;
}

}  // namespace glrt_detail
