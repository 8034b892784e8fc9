// maps.cpp -- glrt_map_decode / glrt_map_normal / glrt_map_alpha (include/glrt_host.h): the CPU statement of the device's material maps (include/glrtx.h
// "Material maps"; csrc/maps.hip.h), bit for bit.  Compiled with -ffp-contract=off and run under MXCSR FTZ | DAZ like the other statements: every operation is
// one rounded fp32 operation in the order the header writes it.  Dots are (x x' + y y') + z z' -- not statement_math.h's dot3.  Words that are kept are moved as
// integers.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "centre_ray.h"
#include "glrt_host.h"
#include "statement_math.h"

namespace {

using glrt_detail::bits;
using glrt_detail::bits_f;
using glrt_detail::FlushDenormals;
using glrt_detail::pos_finite;
using glrt_detail::rsq;
using glrt_detail::tiny;

float dot(const float *a, const float *b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
float neg(float x) { return bits_f(bits(x) ^ 0x80000000u); }
bool finite(float x) { return (bits(x) & 0x7F800000u) != 0x7F800000u; }

// out = n', or n's words where the contract keeps them
void map_normal(const float *r, float scale, float *out) {
    const float *n = r, *e1 = r + 3, *e2 = r + 6, *st0 = r + 9, *st1 = r + 11, *st2 = r + 13, *m = r + 15;
    std::memcpy(out, n, 12);
    const float a = m[0] * scale, b = m[1] * scale;
    if (tiny(a) && tiny(b)) return;
    const float ds1 = st1[0] - st0[0], ds2 = st2[0] - st0[0], dt1 = st1[1] - st0[1], dt2 = st2[1] - st0[1];
    const float det = ds1 * dt2 - ds2 * dt1;
    if (tiny(det) || !finite(det)) return;
    float Tr[3], Br[3];
    for (int c = 0; c < 3; c++) {
        Tr[c] = e1[c] * dt2 - e2[c] * dt1;
        Br[c] = e2[c] * ds1 - e1[c] * ds2;
        if (det < 0.0f) { Tr[c] = neg(Tr[c]); Br[c] = neg(Br[c]); }
    }
    const float k = dot(n, Tr);
    float Tp[3];
    for (int c = 0; c < 3; c++) Tp[c] = Tr[c] - k * n[c];
    const float l2 = dot(Tp, Tp);
    if (!pos_finite(l2)) return;
    const float rl = rsq(l2);
    const float T[3] = {Tp[0] * rl, Tp[1] * rl, Tp[2] * rl};
    float B[3] = {n[1] * T[2] - n[2] * T[1], n[2] * T[0] - n[0] * T[2], n[0] * T[1] - n[1] * T[0]};
    if (dot(B, Br) < 0.0f)
        for (int c = 0; c < 3; c++) B[c] = neg(B[c]);
    float p[3];
    for (int c = 0; c < 3; c++) p[c] = (a * T[c] + b * B[c]) + m[2] * n[c];
    const float q = dot(p, p);
    if (!pos_finite(q)) return;
    const float rq = rsq(q);
    for (int c = 0; c < 3; c++) out[c] = p[c] * rq;
}

}  // namespace

int glrt_map_decode(const float *rgb, size_t n, float *m_out) {
    if (n && (!rgb || !m_out)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    for (size_t i = 0; i < 3 * n; i++) m_out[i] = rgb[i] * 2.0f + -1.0f;
    return GLRT_HOST_OK;
}

int glrt_map_normal(const float *records, size_t n, float scale, float *normal_out) {
    if (n && (!records || !normal_out)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++) map_normal(records + GLRT_MAP_RECORD_FLOATS * i, scale, normal_out + 3 * i);
    return GLRT_HOST_OK;
}

int glrt_map_alpha(const float *rgb, size_t n, float *alpha_out) {
    if (n && (!rgb || !alpha_out)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++)
        for (int c = 0; c < 2; c++) alpha_out[2 * i + c] = rgb[3 * i + c] > GLRT_MAP_ALPHA_MIN ? rgb[3 * i + c] : GLRT_MAP_ALPHA_MIN;
    return GLRT_HOST_OK;
}
