// tonemap.cpp -- glrt_exposure_measure and glrt_tonemap (include/glrt_host.h): the CPU statements of the device's exposure measurement and tone curve
// (glrtx_exposure_measure, glrtx_tonemap, glrtx_resolve_tonemapped_rgba8, include/glrtx.h "Tone mapping"; csrc/tonemap.hip.h).  The contract is the text in
// include/glrtx.h; tests/tonemap_math.py restates it in numpy.  Every fp32 operation below is one correctly rounded IEEE operation in the order written
// (-ffp-contract=off; the only fused operations are the fmaf calls of lp_exp and of the resolve's log2 / exp2), under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "glrt_host.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

bool positive(float v) { return v > 0.0f && !std::isinf(v); }
bool dead(float w) { return tiny(w) || w != w; }

float curve(float I, float s, int op, float ww) {
    float x = I * s;
    x = x > 0.0f ? x : 0.0f;
    x = x < 65504.0f ? x : 65504.0f;
    if (op == 1) return (x * (1.0f + x / ww)) / (1.0f + x);
    if (op == 2) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return x;
}

// The resolve's channel (csrc/pt_kernel.hip.h: rs_channel, the plain statement) on a mean y with the count 1: clamp, pow(L, 1 / gamma) = exp2(log2(L) / gamma)
// by the resolve's own polynomials, round to nearest even to a byte.
float rs_exp2(float t) {
    t = (128.0f < t) ? 128.0f : t;
    t = (-0x1.fbfffep+6f > t) ? -0x1.fbfffep+6f : t;
    const float fl = std::floor(t);
    const float f = t - fl;
    const float scale = bits_f((uint32_t)((int)fl + 127) << 23);
    const float z = f * f;
    const float a = std::fmaf(z, 0x1.ec320ap-10f, 0x1.c95446p-5f);
    const float b = std::fmaf(z, 0x1.26900cp-7f, 0x1.ebd5a8p-3f);
    const float c = std::fmaf(z, a, 0x1.62e4f6p-1f);
    const float d = std::fmaf(z, b, 1.0f);
    return scale * std::fmaf(c, f, d);
}
unsigned char rs_channel(float v, float count, float inv_gamma) {
    float L = v / count;
    L = (L > 0.0f) ? L : 0.0f;
    L = (L < 1.0f) ? L : 1.0f;
    float r = 0.0f;
    if (L != 0.0f) {
        const uint32_t i = bits(L);
        const float ef = (float)((int)((i & 0x7f800000u) >> 23) - 127);
        const float m = bits_f((i & 0x007fffffu) | 0x3f800000u);
        const float t = (m - 1.0f) / (m + 1.0f);
        const float z = t * t, z2 = z * z;
        const float a = std::fmaf(z2, 0x1.a07ab2p-2f, 0x1.27a642p-1f);
        const float b = std::fmaf(z2, 0x1.9d062cp-2f, 0x1.ec6ff2p-1f);
        const float c = std::fmaf(z2, a, 0x1.715476p+1f);
        const float d = std::fmaf(b, z, c);
        r = rs_exp2(std::fmaf(t, d, ef) * inv_gamma);
    }
    r = (1.0f < r) ? 1.0f : r;
    const int q = (int)std::nearbyint(r * 255.0f);  // (the default rounding mode: to nearest even)
    return (unsigned char)(q < 0 ? 0 : (q > 255 ? 255 : q));
}

}  // namespace

int glrt_exposure_measure(const float *src, int width, int rows, float key, int low_permille, int high_permille, float adapt, const float *exposure_in,
                          uint32_t *hist_out, uint64_t *counted, uint64_t *kept, float *mean_log2, float *target, float *exposure_out) {
    if (!src || !hist_out || width < 1 || rows < 1 || width > 65536 || rows > 65536) return GLRT_HOST_EINVAL;
    if (!positive(key) || !(adapt > 0.0f && adapt <= 1.0f) || low_permille < 0 || low_permille >= high_permille || high_permille > 1000) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    std::memset(hist_out, 0, 256 * sizeof(uint32_t));
    const size_t n = (size_t)width * rows;
    for (size_t i = 0; i < n; i++) {
        const float *s = src + 4 * i;
        if (dead(s[3])) continue;
        const float l = lum(s[0] / s[3], s[1] / s[3], s[2] / s[3]);
        if (!(l > 0.0f) || std::isinf(l)) continue;
        const int k = (int)(bits(l) >> 20) - 888;
        hist_out[k < 0 ? 0 : (k > 255 ? 255 : k)]++;
    }
    uint64_t N = 0;
    for (int k = 0; k < 256; k++) N += hist_out[k];
    const uint64_t lo = N * (uint64_t)low_permille / 1000u, hi = N * (uint64_t)high_permille / 1000u;
    uint64_t c = 0, K = 0, S = 0;
    for (int k = 0; k < 256; k++) {
        const uint64_t c1 = c + hist_out[k];
        const uint64_t top = c1 < hi ? c1 : hi, bot = c > lo ? c : lo;
        const uint64_t kk = top > bot ? top - bot : 0;
        K += kk;
        S += kk * (uint64_t)(2 * k + 1);
        c = c1;
    }
    float mean = 0.0f, tgt = exposure_in ? *exposure_in : 1.0f;
    if (K != 0) {
        mean = (float)((double)S / (double)(16 * K) - 16.0);
        tgt = key * lp_exp((0.0f - mean) * 0x1.62e430p-1f);
    }
    const float E = exposure_in ? *exposure_in + (tgt - *exposure_in) * adapt : tgt;
    if (counted) *counted = N;
    if (kept) *kept = K;
    if (mean_log2) *mean_log2 = mean;
    if (target) *target = tgt;
    if (exposure_out) *exposure_out = E;
    return GLRT_HOST_OK;
}

int glrt_tonemap(const float *src, int width, int rows, int op, int auto_exposure, float exposure, float E, float white, float gamma, int flip_y, float *t_out,
                 uint8_t *rgba8_out) {
    if (!src || width < 1 || rows < 1 || width > 65536 || rows > 65536 || op < 0 || op > 2) return GLRT_HOST_EINVAL;
    if (!positive(exposure) || !positive(white) || !std::isnormal(white * white) || !positive(gamma)) return GLRT_HOST_EINVAL;
    const float inv_gamma = 1.0f / gamma;  // (as the device's host side forms it)
    FlushDenormals ftz;
    const float s = auto_exposure ? E * exposure : exposure, ww = white * white;
    for (int y = 0; y < rows; y++) {
        const int oy = flip_y ? rows - 1 - y : y;
        for (int x = 0; x < width; x++) {
            const float *p = src + 4 * ((size_t)y * width + x);
            float T[4] = {0.0f, 0.0f, 0.0f, 1.0f};
            if (!dead(p[3]))
                for (int k = 0; k < 3; k++) T[k] = curve(p[k] / p[3], s, op, ww);
            if (t_out) std::memcpy(t_out + 4 * ((size_t)y * width + x), T, sizeof T);
            if (rgba8_out) {
                uint8_t *o = rgba8_out + 4 * ((size_t)oy * width + x);
                for (int k = 0; k < 3; k++) o[k] = rs_channel(T[k], T[3], inv_gamma);
                o[3] = 255;
            }
        }
    }
    return GLRT_HOST_OK;
}
