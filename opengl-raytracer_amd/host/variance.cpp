// variance.cpp -- glrt_fold_moments, glrt_variance_estimate, glrt_denoise_variance (include/glrt_host.h): the CPU statements of the device's moments fold, variance
// pass and variance-guided a-trous filter (glrtx_render_moments, glrtx_denoise_variance, include/glrtx.h "Variance guidance"; csrc/variance.hip.h,
// csrc/denoise.hip.h).  The contract is the text in include/glrtx.h; tests/variance_math.py restates it in numpy.  Every fp32 operation below is one correctly
// rounded IEEE operation in the order written (-ffp-contract=off; the only fused operations are lp_exp's own fmaf calls), under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

#include "glrt_host.h"

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
inline bool tiny(float x) { return (bits(x) & 0x7F800000u) == 0u; }  // a zero or a denormal
inline float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
inline float max0(float x) { return x > 0.0f ? x : 0.0f; }

// csrc/pt_kernel.hip.h: lp_exp, as host/denoise.cpp states it.
inline float lp_exp(float x) {
    float t = x * bits_f(0x3fb8aa3bu);
    t = 128.0f < t ? 128.0f : t;
    t = bits_f(0xc2fdffffu) > t ? bits_f(0xc2fdffffu) : t;
    const float fl = std::floor(t);
    const float f = t - fl;
    const float p2 = bits_f((uint32_t)((fl == fl ? (int)fl : 0) + 127) << 23);
    const float z = f * f;
    const float a = std::fmaf(z, bits_f(0x3af61905u), bits_f(0x3d64aa23u));
    const float b = std::fmaf(z, bits_f(0x3c134806u), bits_f(0x3e75ead4u));
    const float c = std::fmaf(z, a, bits_f(0x3f31727bu));
    const float d = std::fmaf(z, b, 1.0f);
    return p2 * std::fmaf(c, f, d);
}

constexpr int32_t kNoPixel = INT32_MIN;
constexpr float kAlbedoFloor = 1.0e-3f;

bool sigma_ok(float v) { return v > 0.0f && !std::isinf(v); }

// dn / sigma_normal + min(dd, 80) of glrtx_denoise's tap
inline float geometry_terms(const float *gp, const float *gq, float tden, float sigma_normal, float sigma_depth, float &dd_out) {
    const float nx = gq[0] - gp[0], ny = gq[1] - gp[1], nz = gq[2] - gp[2];
    const float dn = (nx * nx + ny * ny) + nz * nz;
    const float rt = (gq[3] - gp[3]) / tden;
    const float dd = (rt * rt) / sigma_depth;
    dd_out = dd < 80.0f ? dd : 80.0f;
    return dn / sigma_normal;
}

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
                const float la = lum(al[0] > kAlbedoFloor ? al[0] : kAlbedoFloor, al[1] > kAlbedoFloor ? al[1] : kAlbedoFloor, al[2] > kAlbedoFloor ? al[2] : kAlbedoFloor);
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

int glrt_denoise_variance(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations,
                          float sigma_lum, float sigma_normal, float sigma_depth, int demodulate, float *out, float *out_v0) {
    if (!accum || !moments || !normal_depth || !albedo_id || !out) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || iterations < 1 || iterations > 6) return GLRT_HOST_EINVAL;
    if (!sigma_ok(sigma_lum) || !sigma_ok(sigma_normal) || !sigma_ok(sigma_depth)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const size_t n = (size_t)width * rows;
    std::vector<int32_t> id;
    ids_of(accum, albedo_id, n, id);
    std::vector<float> a(4 * n), b(4 * n), va(n), vb(n), l(n);
    estimate(accum, moments, normal_depth, albedo_id, id, width, rows, sigma_normal, sigma_depth, demodulate, va.data());
    if (out_v0) std::memcpy(out_v0, va.data(), n * sizeof(float));
    for (size_t i = 0; i < n; i++) {
        const float *s = accum + 4 * i, *al = albedo_id + 4 * i;
        if (id[i] == kNoPixel) { a[4 * i] = a[4 * i + 1] = a[4 * i + 2] = 0.0f; continue; }
        for (int k = 0; k < 3; k++) {
            float v = s[k] / s[3];
            if (demodulate) v = v / (al[k] > kAlbedoFloor ? al[k] : kAlbedoFloor);
            a[4 * i + k] = canon(v);
        }
    }
    static const float kern[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
    static const float kern3[3] = {0.25f, 0.5f, 0.25f};
    float *src = a.data(), *dst = b.data(), *vsrc = va.data(), *vdst = vb.data();
    for (int it = 0; it < iterations; it++) {
        const int sp = 1 << it;
        for (size_t i = 0; i < n; i++) l[i] = lum(src[4 * i], src[4 * i + 1], src[4 * i + 2]);
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < width; x++) {
                const size_t p = (size_t)y * width + x;
                float *o = dst + 4 * p;
                if (id[p] == kNoPixel) { o[0] = o[1] = o[2] = 0.0f; vdst[p] = 0.0f; continue; }
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
                const float sdl = sigma_lum * std::sqrt(gs / gw) + 1.0e-6f;
                const float *gp = normal_depth + 4 * p;
                const float tden = gp[3] > 1.0e-6f ? gp[3] : 1.0e-6f;
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const int qx = x + sp * dx, qy = y + sp * dy;
                        if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (id[q] != id[p]) continue;
                        const float *cq = src + 4 * q;
                        const float dl = std::fabs(l[q] - l[p]);
                        float dd;
                        const float tn = geometry_terms(gp, normal_depth + 4 * q, tden, sigma_normal, sigma_depth, dd);
                        const float e = (dl / sdl + tn) + dd;
                        const float w = (kern[dy + 2] * kern[dx + 2]) * lp_exp(-e);
                        sw = sw + w;
                        sx = sx + w * cq[0]; sy = sy + w * cq[1]; sz = sz + w * cq[2];
                        sv = sv + (w * w) * vsrc[q];
                    }
                const float den = sw > 1.0e-20f ? sw : 1.0e-20f;
                o[0] = canon(sx / den); o[1] = canon(sy / den); o[2] = canon(sz / den);
                vdst[p] = canon(sv / (den * den));
            }
        float *t = src; src = dst; dst = t;
        t = vsrc; vsrc = vdst; vdst = t;
    }
    for (size_t i = 0; i < n; i++) {
        float *o = out + 4 * i;
        const float *al = albedo_id + 4 * i;
        o[3] = 1.0f;
        for (int k = 0; k < 3; k++) {
            float v = src[4 * i + k];
            if (demodulate && id[i] != kNoPixel) v = canon(v * (al[k] > kAlbedoFloor ? al[k] : kAlbedoFloor));
            o[k] = v;
        }
    }
    return GLRT_HOST_OK;
}
