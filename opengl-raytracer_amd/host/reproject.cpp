// reproject.cpp -- glrt_reproject (include/glrt_host.h): the CPU statement of the device's temporal reprojection (glrtx_reproject, include/glrtx.h;
// csrc/reproject.hip.h).  The contract is the text in include/glrtx.h ("Reprojection"); tests/reproject_math.py restates it in numpy.  Every fp32 operation below
// is one correctly rounded IEEE operation in the order written (-ffp-contract=off), under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstdint>
#include <cstring>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

#include "centre_ray.h"
#include "glrt_host.h"
#include "reproject_moments.h"
#include "reproject_setup.h"

namespace {

struct FlushDenormals {
#if defined(__SSE__)
    unsigned csr = _mm_getcsr();
    FlushDenormals() { _mm_setcsr(csr | 0x8040u); }
    ~FlushDenormals() { _mm_setcsr(csr); }
#endif
};

inline uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
inline float bits_f(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }
inline float canon(float x) { return x != x ? bits_f(0x7FC00000u) : x; }
inline bool tiny(float x) { return (bits(x) & 0x7F800000u) == 0u; }                     // a zero or a denormal
inline bool pos_finite(float x) { return (bits(x) - 0x00800000u) < 0x7F000000u; }       // sign clear, exponent neither 0 nor 255
inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (az * bz + ay * by) + ax * bx; }

constexpr float kMinWeight = 1.0e-6f;

}  // namespace

// glrt_reproject, and with mom / mom_out glrt_reproject_moments: the same pass, the moments riding the same taps.
static int reproject_impl(const float *accum, const float *mom, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev,
                          const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows, int max_history, float depth_tolerance,
                          float normal_tolerance, float *out, float *mom_out, int *carried_out, int *hit_pixels_out) {
    if (!accum || !n0 || !a0 || !n1 || !a1 || !c2w_prev || !s2c_prev || !c2w_cur || !s2c_cur || !out) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return GLRT_HOST_EINVAL;
    glrt_detail::ReprojectSetup st;
    if (glrt_detail::reproject_setup(c2w_prev, s2c_prev, max_history, depth_tolerance, normal_tolerance, st) != 0) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const float *W = st.W, *S = st.S;
    const float Wf = (float)width, Hf = (float)rows;
    int carried = 0, hits = 0;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            float *o = out + 4 * p;
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            if (mom_out) { float *mo = mom_out + 4 * p; mo[0] = mo[1] = mo[2] = mo[3] = 0.0f; }
            const float *N1 = n1 + 4 * p;
            int32_t id;
            std::memcpy(&id, a1 + 4 * p + 3, 4);
            if (id < 0) continue;  // (the reserved id INT32_MIN is negative)
            hits++;
            const float t = N1[3];
            if (!pos_finite(t)) continue;
            float ray[8];
            glrt_detail::centre_ray(c2w_cur, s2c_cur, Wf, Hf, x, y, ray);
            const float Px = ray[0] + t * ray[4], Py = ray[1] + t * ray[5], Pz = ray[2] + t * ray[6];
            const float qx = ((W[0] * Px + W[4] * Py) + W[8] * Pz) + W[12];
            const float qy = ((W[1] * Px + W[5] * Py) + W[9] * Pz) + W[13];
            const float qz = ((W[2] * Px + W[6] * Py) + W[10] * Pz) + W[14];
            const float qw = ((W[3] * Px + W[7] * Py) + W[11] * Pz) + W[15];
            const float sx = ((S[0] * qx + S[4] * qy) + S[8] * qz) + S[12] * qw;
            const float sy = ((S[1] * qx + S[5] * qy) + S[9] * qz) + S[13] * qw;
            const float sw4 = ((S[3] * qx + S[7] * qy) + S[11] * qz) + S[15] * qw;
            const float u = ((sx / sw4 + 1.0f) * 0.5f) * Wf + -1.0f;
            const float v = ((sy / sw4 + 1.0f) * 0.5f) * Hf + -1.0f;
            if (!(pos_finite(sw4) && u >= -1.0f && u < Wf && v >= -1.0f && v < Hf)) continue;  // no tap inside the image (a NaN fails)
            const float ex = Px - st.o_prev[0], ey = Py - st.o_prev[1], ez = Pz - st.o_prev[2];
            const float e = std::sqrt((ez * ez + ey * ey) + ex * ex);
            const float lim = st.depth_tolerance * e;
            const float fx0 = std::floor(u), fy0 = std::floor(v);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const float fx = u - fx0, fy = v - fy0;
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
            float sw = 0.0f, sc = 0.0f, sI[3] = {0.0f, 0.0f, 0.0f};
            glrt_detail::MomSum ms;
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 2; i++) {
                    const int tx = x0 + i, ty = y0 + j;
                    if (tx < 0 || tx >= width || ty < 0 || ty >= rows) continue;
                    const size_t q = (size_t)ty * width + tx;
                    const float *C = accum + 4 * q, *N0 = n0 + 4 * q;
                    int32_t id0;
                    std::memcpy(&id0, a0 + 4 * q + 3, 4);
                    if (id0 != id || tiny(C[3])) continue;
                    if (!(dot3(N1[0], N1[1], N1[2], N0[0], N0[1], N0[2]) >= st.normal_tolerance)) continue;
                    if (!(std::fabs(N0[3] - e) <= lim)) continue;
                    const float w = wx[i] * wy[j];
                    sw = sw + w;
                    sc = sc + w * C[3];
                    for (int k = 0; k < 3; k++) sI[k] = sI[k] + w * (C[k] / C[3]);
                    if (mom) glrt_detail::moments_tap(ms, w, mom + 4 * q);
                }
            if (!(sw > kMinWeight)) continue;
            const float r = std::nearbyint(sc / sw);
            const float n = r > st.max_history ? st.max_history : r;
            if (!(n >= 1.0f)) continue;
            for (int k = 0; k < 3; k++) o[k] = canon((sI[k] / sw) * n);
            o[3] = n;
            carried++;
            if (mom_out) glrt_detail::moments_out(ms, st.max_history, mom_out + 4 * p);
        }
    if (carried_out) *carried_out = carried;
    if (hit_pixels_out) *hit_pixels_out = hits;
    return GLRT_HOST_OK;
}

int glrt_reproject(const float *accum, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev, const float *s2c_prev,
                   const float *c2w_cur, const float *s2c_cur, int width, int rows, int max_history, float depth_tolerance, float normal_tolerance, float *out,
                   int *carried_out, int *hit_pixels_out) {
    return reproject_impl(accum, nullptr, n0, a0, n1, a1, c2w_prev, s2c_prev, c2w_cur, s2c_cur, width, rows, max_history, depth_tolerance, normal_tolerance, out,
                          nullptr, carried_out, hit_pixels_out);
}

int glrt_reproject_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev,
                           const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows, int max_history, float depth_tolerance,
                           float normal_tolerance, float *out, float *moments_out, int *carried_out, int *hit_pixels_out) {
    if (!moments || !moments_out) return GLRT_HOST_EINVAL;
    return reproject_impl(accum, moments, n0, a0, n1, a1, c2w_prev, s2c_prev, c2w_cur, s2c_cur, width, rows, max_history, depth_tolerance, normal_tolerance, out,
                          moments_out, carried_out, hit_pixels_out);
}
