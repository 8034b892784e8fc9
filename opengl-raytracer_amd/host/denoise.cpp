// denoise.cpp -- glrt_denoise_atrous (include/glrt_host.h): the CPU statement of the device's edge-avoiding a-trous filter (glrtx_denoise, include/glrtx.h;
// csrc/denoise.hip.h).  The contract is the text in include/glrtx.h ("Denoising"); tests/denoise_math.py restates it in numpy.  Every fp32 operation below is
// one correctly rounded IEEE operation in the order written (-ffp-contract=off; the only fused operations are lp_exp's own fmaf calls), under MXCSR FTZ | DAZ.
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

// csrc/pt_kernel.hip.h: lp_exp.  (A NaN operand: the integer conversion is whatever it is, the result is NaN either way.)
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

constexpr int32_t kNoPixel = INT32_MIN;  // the id of a pixel without samples
constexpr float kAlbedoFloor = 1.0e-3f;

}  // namespace

int glrt_denoise_atrous(const float *accum, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations, float sigma_color,
                        float sigma_normal, float sigma_depth, int demodulate, float *out) {
    if (!accum || !normal_depth || !albedo_id || !out) return GLRT_HOST_EINVAL;
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || iterations < 1 || iterations > 6) return GLRT_HOST_EINVAL;
    if (!(sigma_color > 0.0f) || !(sigma_normal > 0.0f) || !(sigma_depth > 0.0f) || std::isinf(sigma_color) || std::isinf(sigma_normal) || std::isinf(sigma_depth))
        return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const size_t n = (size_t)width * rows;
    // c: {r, g, b, id}; a pixel with a count of zero (or a denormal one) gets the reserved id and the colour 0
    std::vector<float> a(4 * n), b(4 * n);
    std::vector<int32_t> id(n);
    for (size_t i = 0; i < n; i++) {
        const float *s = accum + 4 * i, *al = albedo_id + 4 * i;
        int32_t m;
        std::memcpy(&m, &al[3], 4);
        if (tiny(s[3]) || m == kNoPixel) { id[i] = kNoPixel; a[4 * i] = a[4 * i + 1] = a[4 * i + 2] = 0.0f; continue; }
        id[i] = m;
        for (int k = 0; k < 3; k++) {
            float v = s[k] / s[3];
            if (demodulate) v = v / (al[k] > kAlbedoFloor ? al[k] : kAlbedoFloor);
            a[4 * i + k] = canon(v);
        }
    }
    static const float kern[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
    float *src = a.data(), *dst = b.data();
    for (int it = 0; it < iterations; it++) {
        const int sp = 1 << it;
        float sc = sigma_color * bits_f((uint32_t)(127 - 2 * it) << 23);  // sigma_color * 4^-it
        if (tiny(sc)) sc = 0.0f;
        for (int y = 0; y < rows; y++)
            for (int x = 0; x < width; x++) {
                const size_t p = (size_t)y * width + x;
                float *o = dst + 4 * p;
                if (id[p] == kNoPixel) { o[0] = o[1] = o[2] = 0.0f; continue; }
                const float *cp = src + 4 * p, *gp = normal_depth + 4 * p;
                const float tden = gp[3] > 1.0e-6f ? gp[3] : 1.0e-6f;
                float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f;
                for (int dy = -2; dy <= 2; dy++)
                    for (int dx = -2; dx <= 2; dx++) {
                        const int qx = x + sp * dx, qy = y + sp * dy;
                        if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (id[q] != id[p]) continue;  // (also: a pixel without samples)
                        const float *cq = src + 4 * q, *gq = normal_depth + 4 * q;
                        const float cx = cq[0] - cp[0], cy = cq[1] - cp[1], cz = cq[2] - cp[2];
                        const float dc = (cx * cx + cy * cy) + cz * cz;
                        const float nx = gq[0] - gp[0], ny = gq[1] - gp[1], nz = gq[2] - gp[2];
                        const float dn = (nx * nx + ny * ny) + nz * nz;
                        const float rt = (gq[3] - gp[3]) / tden;
                        const float dd = (rt * rt) / sigma_depth;
                        const float e = (dc / sc + dn / sigma_normal) + (dd < 80.0f ? dd : 80.0f);
                        const float w = (kern[dy + 2] * kern[dx + 2]) * lp_exp(-e);
                        sw = sw + w;
                        sx = sx + w * cq[0]; sy = sy + w * cq[1]; sz = sz + w * cq[2];
                    }
                const float den = sw > 1.0e-20f ? sw : 1.0e-20f;
                o[0] = canon(sx / den); o[1] = canon(sy / den); o[2] = canon(sz / den);
            }
        float *t = src; src = dst; dst = t;
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
