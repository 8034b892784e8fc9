// reproject.cpp -- glrt_reproject (include/glrt_host.h): the CPU statement of the device's temporal reprojection (glrtx_reproject, include/glrtx.h;
// csrc/reproject.hip.h).  The contract is the text in include/glrtx.h ("Reprojection"); tests/reproject_math.py restates it in numpy.  Every fp32 operation below
// is one correctly rounded IEEE operation in the order written (-ffp-contract=off), under MXCSR FTZ | DAZ.
#include <cstdint>
#include <cstring>

#include "centre_ray.h"
#include "glrt_host.h"
#include "reproject_lookup.h"

using glrt_detail::FlushDenormals;
using glrt_detail::pos_finite;

// glrt_reproject, and with mom / mom_out glrt_reproject_moments: the same pass, the moments riding the same taps.
static int reproject_impl(const float *accum, const float *mom, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev,
                          const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows, int max_history, float depth_tolerance,
                          float normal_tolerance, float *out, float *mom_out, int *carried_out, int *hit_pixels_out) {
    if (!accum || !n0 || !a0 || !n1 || !a1 || !c2w_prev || !s2c_prev || !c2w_cur || !s2c_cur || !out) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return GLRT_HOST_EINVAL;
    glrt_detail::ReprojectSetup st;
    if (glrt_detail::reproject_setup(c2w_prev, s2c_prev, max_history, depth_tolerance, normal_tolerance, st) != 0) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const glrt_detail::OldView old{accum, mom, n0, a0, width, rows};
    const float Wf = (float)width, Hf = (float)rows;
    int carried = 0, hits = 0;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            float *o = out + 4 * p, *mo = mom_out ? mom_out + 4 * p : nullptr;
            o[0] = o[1] = o[2] = o[3] = 0.0f;
            if (mo) mo[0] = mo[1] = mo[2] = mo[3] = 0.0f;
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
            if (glrt_detail::history_lookup(st, old, Px, Py, Pz, N1[0], N1[1], N1[2], id, o, mo)) carried++;
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
