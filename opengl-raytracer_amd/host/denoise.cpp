// denoise.cpp -- glrt_denoise_atrous and glrt_denoise_variance (include/glrt_host.h): the CPU statements of the device's edge-avoiding a-trous filter and of its
// variance-guided form (glrtx_denoise, glrtx_denoise_variance, include/glrtx.h; csrc/denoise.hip.h), one prep, one iteration and one re-modulation for both.
// The contract is the text in include/glrtx.h ("Denoising", "Variance guidance"); tests/denoise_math.py and tests/variance_math.py restate it in numpy.  Every
// fp32 operation below is one correctly rounded IEEE operation in the order written (-ffp-contract=off; the only fused operations are lp_exp's own fmaf calls),
// under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "glrt_host.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

bool sigma_ok(float v) { return v > 0.0f && !std::isinf(v); }

// Both filters.  v0 null: the plain one, the colour term |c_q - c_p|^2 / (sigma_c * 4^-it).  v0 the variance plane V0 (host/variance.cpp): the guided one, the
// colour term |lum(c_q) - lum(c_p)| / (sigma_c * sqrt(g_p) + 1e-6), g_p the 3x3 Gaussian of the variance around p, the variance filtered alongside with the
// squared weights.  The caller has checked the arguments and flushes denormals.
void filter(const float *accum, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations, float sigma_c, float sigma_normal,
            float sigma_depth, int demodulate, const float *v0, float *out) {
    const bool var = v0 != nullptr;
    const size_t n = (size_t)width * rows;
    // c: {r, g, b, id}; a pixel with a count of zero (or a denormal one) gets the reserved id and the colour 0
    std::vector<float> a(4 * n), b(4 * n), va, vb(var ? n : 0), l(var ? n : 0);
    if (var) va.assign(v0, v0 + n);
    std::vector<int32_t> id(n);
    for (size_t i = 0; i < n; i++) {
        const float *s = accum + 4 * i, *al = albedo_id + 4 * i;
        int32_t m;
        std::memcpy(&m, &al[3], 4);
        if (tiny(s[3]) || m == kNoPixel) { id[i] = kNoPixel; a[4 * i] = a[4 * i + 1] = a[4 * i + 2] = 0.0f; continue; }
        id[i] = m;
        for (int k = 0; k < 3; k++) {
            float v = s[k] / s[3];
            if (demodulate) v = v / albedo_of(al[k]);
            a[4 * i + k] = canon(v);
        }
    }
    static const float kern[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
    static const float kern3[3] = {0.25f, 0.5f, 0.25f};
    float *src = a.data(), *dst = b.data(), *vsrc = va.data(), *vdst = vb.data();
    for (int it = 0; it < iterations; it++) {
        const int sp = 1 << it;
        float sc = sigma_c;  // the colour term's divisor: per iteration here, per pixel in the guided form
        if (var)
            for (size_t i = 0; i < n; i++) l[i] = lum(src[4 * i], src[4 * i + 1], src[4 * i + 2]);
        else {
            sc = sigma_c * bits_f((uint32_t)(127 - 2 * it) << 23);  // sigma_color * 4^-it
            if (tiny(sc)) sc = 0.0f;
        }
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < width; x++) {
                const size_t p = (size_t)y * width + x;
                float *o = dst + 4 * p;
                if (id[p] == kNoPixel) {
                    o[0] = o[1] = o[2] = 0.0f;
                    if (var) vdst[p] = 0.0f;
                    continue;
                }
                if (var) {
                    float gs = 0.0f, gw = 0.0f;
                    for (int dy = -1; dy <= 1; dy++)
                        for (int dx = -1; dx <= 1; dx++) {
                            const int qx = x + dx, qy = y + dy;
                            if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                            const size_t q = (size_t)qy * width + qx;
                            if (id[q] != id[p]) continue;
                            const float kw = kern3[dy + 1] * kern3[dx + 1];
                            gs = gs + kw * vsrc[q];
                            gw = gw + kw;
                        }
                    sc = sigma_c * std::sqrt(gs / gw) + 1.0e-6f;
                }
                const float *cp = src + 4 * p, *gp = normal_depth + 4 * p;
                const float tden = gp[3] > 1.0e-6f ? gp[3] : 1.0e-6f;
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const int qx = x + sp * dx, qy = y + sp * dy;
                        if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (id[q] != id[p]) continue;  // (also: a pixel without samples)
                        const float *cq = src + 4 * q;
                        float dc;
                        if (var) dc = std::fabs(l[q] - l[p]);
                        else {
                            const float cx = cq[0] - cp[0], cy = cq[1] - cp[1], cz = cq[2] - cp[2];
                            dc = (cx * cx + cy * cy) + cz * cz;
                        }
                        float dd;
                        const float tn = geometry_terms(gp, normal_depth + 4 * q, tden, sigma_normal, sigma_depth, dd);
                        const float e = (dc / sc + tn) + dd;
                        const float w = (kern[dy + 2] * kern[dx + 2]) * lp_exp(-e);
                        sw = sw + w;
                        sx = sx + w * cq[0]; sy = sy + w * cq[1]; sz = sz + w * cq[2];
                        if (var) sv = sv + (w * w) * vsrc[q];
                    }
                const float den = sw > 1.0e-20f ? sw : 1.0e-20f;
                o[0] = canon(sx / den); o[1] = canon(sy / den); o[2] = canon(sz / den);
                if (var) vdst[p] = canon(sv / (den * den));
            }
        std::swap(src, dst);
        std::swap(vsrc, vdst);
    }
    for (size_t i = 0; i < n; i++) {
        float *o = out + 4 * i;
        const float *al = albedo_id + 4 * i;
        o[3] = 1.0f;
        for (int k = 0; k < 3; k++) {
            float v = src[4 * i + k];
            if (demodulate && id[i] != kNoPixel) v = canon(v * albedo_of(al[k]));
            o[k] = v;
        }
    }
}

}  // namespace

int glrt_denoise_atrous(const float *accum, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations, float sigma_color,
                        float sigma_normal, float sigma_depth, int demodulate, float *out) {
    if (!accum || !normal_depth || !albedo_id || !out) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || iterations < 1 || iterations > 6) return GLRT_HOST_EINVAL;
    if (!sigma_ok(sigma_color) || !sigma_ok(sigma_normal) || !sigma_ok(sigma_depth)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    filter(accum, normal_depth, albedo_id, width, rows, iterations, sigma_color, sigma_normal, sigma_depth, demodulate, nullptr, out);
    return GLRT_HOST_OK;
}

int glrt_denoise_variance(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations,
                          float sigma_lum, float sigma_normal, float sigma_depth, int demodulate, float *out, float *out_v0) {
    if (!accum || !moments || !normal_depth || !albedo_id || !out) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || iterations < 1 || iterations > 6) return GLRT_HOST_EINVAL;
    if (!sigma_ok(sigma_lum) || !sigma_ok(sigma_normal) || !sigma_ok(sigma_depth)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const size_t n = (size_t)width * rows;
    std::vector<float> v0(n);  // the variance pass (host/variance.cpp)
    if (const int rc = glrt_variance_estimate(accum, moments, normal_depth, albedo_id, width, rows, sigma_normal, sigma_depth, demodulate, v0.data())) return rc;
    if (out_v0) std::memcpy(out_v0, v0.data(), n * sizeof(float));
    filter(accum, normal_depth, albedo_id, width, rows, iterations, sigma_lum, sigma_normal, sigma_depth, demodulate, v0.data(), out);
    return GLRT_HOST_OK;
}
