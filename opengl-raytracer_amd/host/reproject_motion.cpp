// reproject_motion.cpp -- glrt_reproject_motion (include/glrt_host.h): the CPU statement of the device's motion-aware reprojection (glrtx_reproject_motion,
// include/glrtx.h "Reprojection across a geometry move"; csrc/reproject_motion.hip.h).  The contract is the text in include/glrtx.h;
// tests/reproject_motion_math.py restates it in numpy.  Every fp32 operation of the per-pixel arithmetic is one correctly rounded IEEE operation in the order
// written (-ffp-contract=off), under MXCSR FTZ | DAZ.  The previous triangles' edges are formed BEFORE that mode is set, as pack_scene (csrc/glrtx.hip) and the
// device refit form a leaf record's edges: one IEEE subtraction each, denormals kept.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

#include "centre_ray.h"
#include "glrt_host.h"
#include "reproject_moments.h"
#include "reproject_setup.h"

namespace {

using glrt_detail::rsq;

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

// glrt_reproject_motion, and with mom / mom_out glrt_reproject_motion_moments: the same pass, the moments riding the same taps.
static int reproject_motion_impl(const float *accum, const float *mom, const float *n0, const float *a0, const float *g1, const float *a1, const float *vert_prev,
                                 size_t n_vert, const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width, int rows, int max_history,
                                 float depth_tolerance, float normal_tolerance, float *out, float *mom_out, int *carried_out, int *hit_pixels_out) {
    if (!accum || !n0 || !a0 || !g1 || !a1 || !c2w_prev || !s2c_prev || !out) return GLRT_HOST_EINVAL;
    if ((n_tri && (!tri || !vert_prev)) || n_tri > (size_t)INT32_MAX) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return GLRT_HOST_EINVAL;
    glrt_detail::ReprojectSetup st;
    if (glrt_detail::reproject_setup(c2w_prev, s2c_prev, max_history, depth_tolerance, normal_tolerance, st) != 0) return GLRT_HOST_EINVAL;
    // the previous triangles: {p0, e1, e2} and {n0, n1, n2}, the edges with denormals kept (the caller's mode is restored around them)
    std::vector<float> rec(18 * n_tri);
    {
#if defined(__SSE__)
        const unsigned csr = _mm_getcsr();
        _mm_setcsr(csr & ~0x8040u);
#endif
        int rc = GLRT_HOST_OK;
        for (size_t t = 0; t < n_tri && rc == GLRT_HOST_OK; t++) {
            const float *v[3];
            for (int k = 0; k < 3; k++) {
                const float f = tri[4 * t + k];
                if (!(f >= 0.0f) || (size_t)f >= n_vert) { rc = GLRT_HOST_EINDEX; break; }
                v[k] = vert_prev + GLRT_VERTEX_FLOATS * (size_t)f;
            }
            if (rc != GLRT_HOST_OK) break;
            float *r = &rec[18 * t];
            for (int j = 0; j < 3; j++) {
                r[j] = v[0][j];
                r[3 + j] = v[1][j] - v[0][j];
                r[6 + j] = v[2][j] - v[0][j];
                for (int k = 0; k < 3; k++) r[9 + 3 * k + j] = v[k][3 + j];
            }
        }
#if defined(__SSE__)
        _mm_setcsr(csr);
#endif
        if (rc != GLRT_HOST_OK) return rc;
    }
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
            const float *G1 = g1 + 4 * p;
            int32_t id, tr;
            std::memcpy(&id, a1 + 4 * p + 3, 4);
            std::memcpy(&tr, G1, 4);
            if (id < 0) continue;  // (the reserved id INT32_MIN is negative)
            hits++;
            if (tr < 0 || (size_t)tr >= n_tri) continue;
            const float *r = &rec[18 * (size_t)tr];
            const float u = G1[1], v = G1[2];
            const float Px = (r[0] + u * r[3]) + v * r[6], Py = (r[1] + u * r[4]) + v * r[7], Pz = (r[2] + u * r[5]) + v * r[8];
            // surf_tri (csrc/pt_kernel.hip.h) on the previous vertex normals
            const float *m0 = r + 9, *m1 = r + 12, *m2 = r + 15;
            const float w0 = (1.0f - u) - v;
            const float tx = (w0 * m0[0] + u * m1[0]) + v * m2[0];
            const float ty = (w0 * m0[1] + u * m1[1]) + v * m2[1];
            const float tz = (w0 * m0[2] + u * m1[2]) + v * m2[2];
            const float rn = rsq(dot3(tx, ty, tz, tx, ty, tz));
            const float mx = tx * rn, my = ty * rn, mz = tz * rn;
            const float qx = ((W[0] * Px + W[4] * Py) + W[8] * Pz) + W[12];
            const float qy = ((W[1] * Px + W[5] * Py) + W[9] * Pz) + W[13];
            const float qz = ((W[2] * Px + W[6] * Py) + W[10] * Pz) + W[14];
            const float qw = ((W[3] * Px + W[7] * Py) + W[11] * Pz) + W[15];
            const float sx = ((S[0] * qx + S[4] * qy) + S[8] * qz) + S[12] * qw;
            const float sy = ((S[1] * qx + S[5] * qy) + S[9] * qz) + S[13] * qw;
            const float sw4 = ((S[3] * qx + S[7] * qy) + S[11] * qz) + S[15] * qw;
            const float ui = ((sx / sw4 + 1.0f) * 0.5f) * Wf + -1.0f;
            const float vi = ((sy / sw4 + 1.0f) * 0.5f) * Hf + -1.0f;
            if (!(pos_finite(sw4) && ui >= -1.0f && ui < Wf && vi >= -1.0f && vi < Hf)) continue;  // no tap inside the image (a NaN fails)
            const float ex = Px - st.o_prev[0], ey = Py - st.o_prev[1], ez = Pz - st.o_prev[2];
            const float e = std::sqrt((ez * ez + ey * ey) + ex * ex);
            const float lim = st.depth_tolerance * e;
            const float fx0 = std::floor(ui), fy0 = std::floor(vi);
            const int x0 = (int)fx0, y0 = (int)fy0;
            const float fx = ui - fx0, fy = vi - fy0;
            const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
            float sw = 0.0f, sc = 0.0f, sI[3] = {0.0f, 0.0f, 0.0f};
            glrt_detail::MomSum ms;
            for (int j = 0; j < 2; j++)
                for (int i = 0; i < 2; i++) {
                    const int tx0 = x0 + i, ty0 = y0 + j;
                    if (tx0 < 0 || tx0 >= width || ty0 < 0 || ty0 >= rows) continue;
                    const size_t q = (size_t)ty0 * width + tx0;
                    const float *C = accum + 4 * q, *N0 = n0 + 4 * q;
                    int32_t id0;
                    std::memcpy(&id0, a0 + 4 * q + 3, 4);
                    if (id0 != id || tiny(C[3])) continue;
                    if (!(dot3(mx, my, mz, N0[0], N0[1], N0[2]) >= st.normal_tolerance)) continue;
                    if (!(std::fabs(N0[3] - e) <= lim)) continue;
                    const float w = wx[i] * wy[j];
                    sw = sw + w;
                    sc = sc + w * C[3];
                    for (int k = 0; k < 3; k++) sI[k] = sI[k] + w * (C[k] / C[3]);
                    if (mom) glrt_detail::moments_tap(ms, w, mom + 4 * q);
                }
            if (!(sw > kMinWeight)) continue;
            const float rr = std::nearbyint(sc / sw);
            const float n = rr > st.max_history ? st.max_history : rr;
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

int glrt_reproject_motion(const float *accum, const float *n0, const float *a0, const float *g1, const float *a1, const float *vert_prev, size_t n_vert,
                          const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width, int rows, int max_history,
                          float depth_tolerance, float normal_tolerance, float *out, int *carried_out, int *hit_pixels_out) {
    return reproject_motion_impl(accum, nullptr, n0, a0, g1, a1, vert_prev, n_vert, tri, n_tri, c2w_prev, s2c_prev, width, rows, max_history, depth_tolerance,
                                 normal_tolerance, out, nullptr, carried_out, hit_pixels_out);
}

int glrt_reproject_motion_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *g1, const float *a1,
                                  const float *vert_prev, size_t n_vert, const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width,
                                  int rows, int max_history, float depth_tolerance, float normal_tolerance, float *out, float *moments_out, int *carried_out,
                                  int *hit_pixels_out) {
    if (!moments || !moments_out) return GLRT_HOST_EINVAL;
    return reproject_motion_impl(accum, moments, n0, a0, g1, a1, vert_prev, n_vert, tri, n_tri, c2w_prev, s2c_prev, width, rows, max_history, depth_tolerance,
                                 normal_tolerance, out, moments_out, carried_out, hit_pixels_out);
}
