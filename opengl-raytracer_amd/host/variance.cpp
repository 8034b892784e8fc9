// variance.cpp -- glrt_fold_moments, glrt_variance_estimate and glrt_adaptive_select_moments (include/glrt_host.h): the CPU statements of the device's moments fold,
// variance pass and selection from M (glrtx_render_moments, glrtx_denoise_variance, glrtx_render_adaptive_moments, include/glrtx.h "Variance guidance" and
// "Adaptive sampling by variance"; csrc/variance.hip.h).  The variance-guided filter that reads V0 is
// host/denoise.cpp's.  The contract is the text in include/glrtx.h; tests/variance_math.py restates it in numpy.  Every fp32 operation below is one correctly
// rounded IEEE operation in the order written (-ffp-contract=off; the only fused operations are lp_exp's own fmaf calls), under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "glrt_host.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

inline float max0(float x) { return x > 0.0f ? x : 0.0f; }

constexpr float kAdaptLumFloor = 1.0e-3f;  // csrc/pt_kernel.hip.h: kAdaptLumFloor

bool sigma_ok(float v) { return v > 0.0f && !std::isinf(v); }

void ids_of(const float *accum, const float *albedo_id, size_t n, std::vector<int32_t> &id) {
    id.resize(n);
    for (size_t i = 0; i < n; i++) {
        int32_t m;
        std::memcpy(&m, &albedo_id[4 * i + 3], 4);
        id[i] = tiny(accum[4 * i + 3]) ? kNoPixel : m;
    }
}

void estimate(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, const std::vector<int32_t> &id, int width, int rows,
              float sigma_normal, float sigma_depth, int demodulate, float *v0) {
    const size_t n = (size_t)width * rows;
    std::vector<float> mu(2 * n);
    for (size_t i = 0; i < n; i++) {
        const float *s = accum + 4 * i, *m = moments + 4 * i;
        if (!tiny(m[3])) { mu[2 * i] = m[0] / m[3]; mu[2 * i + 1] = m[1] / m[3]; }
        else {
            const float l = lum(s[0] / s[3], s[1] / s[3], s[2] / s[3]);
            mu[2 * i] = l; mu[2 * i + 1] = l * l;
        }
    }
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            if (id[p] == kNoPixel) { v0[p] = 0.0f; continue; }
            const float mw = moments[4 * p + 3];
            float v;
            if (mw >= 4.0f) v = max0(mu[2 * p + 1] - mu[2 * p] * mu[2 * p]) / mw;
            else {
                const float *gp = normal_depth + 4 * p;
                const float tden = gp[3] > 1.0e-6f ? gp[3] : 1.0e-6f;
                float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
                for (int dy = -3; dy <= 3; dy++)
                    for (int dx = -3; dx <= 3; dx++) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (id[q] != id[p]) continue;
                        float dd;
                        const float tn = geometry_terms(gp, normal_depth + 4 * q, tden, sigma_normal, sigma_depth, dd);
                        const float w = lp_exp(-(tn + dd));
                        sw = sw + w;
                        s1 = s1 + w * mu[2 * q];
                        s2 = s2 + w * mu[2 * q + 1];
                    }
                const float den = sw > 1.0e-20f ? sw : 1.0e-20f;
                const float S1 = s1 / den, S2 = s2 / den;
                v = max0(S2 - S1 * S1);
            }
            if (demodulate) {
                const float *al = albedo_id + 4 * p;
                const float la = lum(albedo_of(al[0]), albedo_of(al[1]), albedo_of(al[2]));
                v = v / (la * la);
            }
            v0[p] = canon(v);
        }
}

}  // namespace

int glrt_fold_moments(float *moments, const float *planes, int n_planes, int width, int rows) {
    if (!moments || (n_planes > 0 && !planes) || n_planes < 0 || width < 1 || rows < 1 || width > 65536 || rows > 65536) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const size_t n = (size_t)width * rows;
    for (int k = 0; k < n_planes; k++)
        for (size_t i = 0; i < n; i++) {
            const float *s = planes + 4 * ((size_t)k * n + i);
            float *m = moments + 4 * i;
            const float l = lum(s[0], s[1], s[2]);
            m[0] = m[0] + l; m[1] = m[1] + l * l; m[3] = m[3] + 1.0f;
        }
    return GLRT_HOST_OK;
}

int glrt_variance_estimate(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows, float sigma_normal,
                           float sigma_depth, int demodulate, float *out_v0) {
    if (!accum || !moments || !normal_depth || !albedo_id || !out_v0) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || !sigma_ok(sigma_normal) || !sigma_ok(sigma_depth)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    std::vector<int32_t> id;
    ids_of(accum, albedo_id, (size_t)width * rows, id);
    estimate(accum, moments, normal_depth, albedo_id, id, width, rows, sigma_normal, sigma_depth, demodulate, out_v0);
    return GLRT_HOST_OK;
}

int glrt_adaptive_select_moments(const float *moments, int width, int rows, float threshold, int min_samples, uint8_t *mask_out, float *err_out) {
    if (!moments || !mask_out || width < 1 || rows < 1 || width > 65536 || rows > 65536) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const int tiles_x = (width + 7) / 8, tiles_y = (rows + 7) / 8;
    for (int ty = 0; ty < tiles_y; ty++)
        for (int tx = 0; tx < tiles_x; tx++) {
            float s[64];
            int n_in = 0;
            bool force = false;
            for (int k = 0; k < 64; k++) {  // lane k of the tile's wave: pixel (k & 7, k >> 3)
                const int x = tx * 8 + (k & 7), y = ty * 8 + (k >> 3);
                s[k] = 0.0f;
                if (x >= width || y >= rows) continue;
                n_in++;
                const float *m = moments + 4 * ((size_t)y * width + x);
                if (!(m[3] >= (float)min_samples)) force = true;
                const float mu1 = m[0] / m[3], mu2 = m[1] / m[3];
                const float v = max0(mu2 - mu1 * mu1) / m[3];
                s[k] = std::sqrt(v) / std::sqrt(mu1 + kAdaptLumFloor);
            }
            for (int h = 32; h >= 1; h >>= 1)
                for (int k = 0; k < h; k++) s[k] = s[k] + s[k ^ h];
            const float e = s[0] / (float)n_in;
            const size_t t = (size_t)ty * tiles_x + tx;
            mask_out[t] = (force || threshold < 0.0f || !(e <= threshold)) ? 1 : 0;
            if (err_out) err_out[t] = canon(e);
        }
    return GLRT_HOST_OK;
}
