// reproject_motion.cpp -- glrt_reproject_motion (include/glrt_host.h): the CPU statement of the device's motion-aware reprojection (glrtx_reproject_motion,
// include/glrtx.h "Reprojection across a geometry move"; csrc/reproject_motion.hip.h).  The contract is the text in include/glrtx.h;
// tests/reproject_motion_math.py restates it in numpy.  Every fp32 operation of the per-pixel arithmetic is one correctly rounded IEEE operation in the order
// written (-ffp-contract=off), under MXCSR FTZ | DAZ.  The previous triangles' edges are formed BEFORE that mode is set, as pack_scene (csrc/glrtx.hip) and the
// device refit form a leaf record's edges: one IEEE subtraction each, denormals kept.
#include <cstdint>
#include <cstring>
#include <vector>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

#include "centre_ray.h"
#include "glrt_host.h"
#include "reproject_lookup.h"

using glrt_detail::dot3;
using glrt_detail::FlushDenormals;
using glrt_detail::rsq;

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
    const glrt_detail::OldView old{accum, mom, n0, a0, width, rows};
    int carried = 0, hits = 0;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            float *o = out + 4 * p, *mo = mom_out ? mom_out + 4 * p : nullptr;
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            if (mo) mo[0] = mo[1] = mo[2] = mo[3] = 0.0f;
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
            if (glrt_detail::history_lookup(st, old, Px, Py, Pz, tx * rn, ty * rn, tz * rn, id, o, mo)) carried++;
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
