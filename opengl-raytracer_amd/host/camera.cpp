// camera.cpp -- the camera matrices the reference builds with GLM (GLM is not
// vendored in the reference tree; these are the standard right-handed,
// depth -1..1 definitions):
//   viewM = lookAt(origin, target, up)                       scene.cpp:93
//   projM = perspective(radians(fov), W/H, near, far)        scene.cpp:113
//   c2w = inverse(viewM * modelM), s2c = inverse(projM)      window.cpp:230-233
// Column-major float[16]: m[col*4 + row].
#include <cmath>
#include <cstring>

#include "glrt_host.h"
#include "mat4_inverse.h"

namespace {
inline void cross(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
inline float dot(const float a[3], const float b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
inline void normalize(float v[3]) {
    float r = 1.0f / std::sqrt(dot(v, v));
    v[0] *= r; v[1] *= r; v[2] *= r;
}
}  // namespace

extern "C" {

void glrt_look_at(const float eye[3], const float center[3], const float up[3], float out[16]) {
    float f[3] = {center[0] - eye[0], center[1] - eye[1], center[2] - eye[2]};
    normalize(f);
    float s[3];
    cross(f, up, s);
    normalize(s);
    float u[3];
    cross(s, f, u);
    float m[16] = {s[0], u[0], -f[0], 0.f,  //
                   s[1], u[1], -f[1], 0.f,  //
                   s[2], u[2], -f[2], 0.f,  //
                   -dot(s, eye), -dot(u, eye), dot(f, eye), 1.f};
    std::memcpy(out, m, sizeof m);
}

void glrt_perspective(float fovy_deg, float aspect, float z_near, float z_far, float out[16]) {
    const float fovy = fovy_deg * 0.01745329251994329576923690768489f;
    const float t = std::tan(fovy / 2.0f);
    std::memset(out, 0, 16 * sizeof(float));
    out[0] = 1.0f / (aspect * t);
    out[5] = 1.0f / t;
    out[10] = -(z_far + z_near) / (z_far - z_near);
    out[11] = -1.0f;
    out[14] = -(2.0f * z_far * z_near) / (z_far - z_near);
}

void glrt_mat4_mul(const float a[16], const float b[16], float out[16]) {
    float r[16];
    for (int c = 0; c < 4; c++)
        for (int row = 0; row < 4; row++) {
            float acc = 0.f;
            for (int k = 0; k < 4; k++) acc += a[k * 4 + row] * b[c * 4 + k];
            r[c * 4 + row] = acc;
        }
    std::memcpy(out, r, sizeof r);
}

// Cofactor expansion in float, like glm::inverse (host/mat4_inverse.h).
int glrt_mat4_inverse(const float m[16], float out[16]) { return glrt_detail::mat4_inverse(m, out); }

void glrt_frame_seed(uint32_t frame, float out[2]) {
    double a = 0.137 + 0.6180340 * (double)frame;
    double b = 0.731 + 0.3819660 * (double)frame;
    out[0] = (float)(a - std::floor(a));
    out[1] = (float)(b - std::floor(b));
}

}  // extern "C"
