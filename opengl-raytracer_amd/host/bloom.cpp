// bloom.cpp -- glrt_bloom (include/glrt_host.h): the CPU statement of the device's bloom pass (glrtx_bloom, glrtx_debug_bloom, include/glrtx.h "Bloom";
// csrc/bloom.hip.h).  The contract is the text in include/glrtx.h; tests/bloom_math.py restates it in numpy.  Every fp32 operation below is one correctly
// rounded IEEE operation in the order written (-ffp-contract=off; there is no fused operation here), under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "glrt_host.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

struct Plane {
    int w = 0, h = 0;
    std::vector<float> v;  // w * h * 3
    Plane(int w_, int h_) : w(w_), h(h_), v((size_t)w_ * h_ * 3) {}
    float *at(int x, int y) { return v.data() + 3 * ((size_t)y * w + x); }
    const float *at(int x, int y) const { return v.data() + 3 * ((size_t)y * w + x); }
};

bool dead(float w) { return tiny(w) || w != w; }
int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
float c5(float a, float b, float c, float d, float e) { return ((a + e) + 4.0f * (b + d)) + 6.0f * c; }

// x: the pixel's value in front of the bright pass and of B
void pixel_value(const float *s, float x[3]) {
    for (int k = 0; k < 3; k++) {
        if (dead(s[3])) { x[k] = 0.0f; continue; }
        const float I = s[k] / s[3];
        float v = I > 0.0f ? I : 0.0f;  // (a NaN: 0)
        x[k] = v < 65504.0f ? v : 65504.0f;
    }
}

Plane down(const Plane &D) {
    Plane out((D.w + 1) >> 1, (D.h + 1) >> 1);
    for (int y = 0; y < out.h; y++)
        for (int x = 0; x < out.w; x++) {
            float r[5][3];
            for (int j = -2; j <= 2; j++) {
                const int yy = clampi(2 * y + j, 0, D.h - 1);
                const float *t[5];
                for (int i = -2; i <= 2; i++) t[i + 2] = D.at(clampi(2 * x + i, 0, D.w - 1), yy);
                for (int k = 0; k < 3; k++) r[j + 2][k] = c5(t[0][k], t[1][k], t[2][k], t[3][k], t[4][k]);
            }
            for (int k = 0; k < 3; k++) out.at(x, y)[k] = c5(r[0][k], r[1][k], r[2][k], r[3][k], r[4][k]) * 0x1p-8f;
        }
    return out;
}

// up(C, w, h) at (x, y), channel k
float up_at(const Plane &C, int x, int y, int k) {
    const int nx = clampi(x >> 1, 0, C.w - 1), fx = clampi((x & 1) ? (x >> 1) + 1 : (x >> 1) - 1, 0, C.w - 1);
    const int ny = clampi(y >> 1, 0, C.h - 1), fy = clampi((y & 1) ? (y >> 1) + 1 : (y >> 1) - 1, 0, C.h - 1);
    const float hn = 0.75f * C.at(nx, ny)[k] + 0.25f * C.at(fx, ny)[k];
    const float hf = 0.75f * C.at(nx, fy)[k] + 0.25f * C.at(fx, fy)[k];
    return 0.75f * hn + 0.25f * hf;
}

}  // namespace

int glrt_bloom(const float *src, int width, int rows, float threshold, float strength, int levels, float *d_out, float *b_out) {
    if (!src || width < 1 || rows < 1 || width > 65536 || rows > 65536 || levels < 1 || levels > 8) return GLRT_HOST_EINVAL;
    if (!(threshold >= 0.0f) || std::isinf(threshold) || !(strength >= 0.0f && strength <= 1.0e4f)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    std::vector<Plane> D;
    D.emplace_back(width, rows);
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            float v[3];
            pixel_value(src + 4 * ((size_t)y * width + x), v);
            const float l = lum(v[0], v[1], v[2]);
            float n = l - threshold;
            n = n > 0.0f ? n : 0.0f;
            const float m = l > 1.0e-4f ? l : 1.0e-4f;
            const float g = n / m;
            for (int k = 0; k < 3; k++) D[0].at(x, y)[k] = v[k] * g;
        }
    for (int k = 0; k < levels; k++) {
        D.push_back(down(D[(size_t)k]));
        if (d_out) {
            const Plane &p = D.back();
            for (size_t i = 0; i < (size_t)p.w * p.h; i++) {
                d_out[0] = p.v[3 * i]; d_out[1] = p.v[3 * i + 1]; d_out[2] = p.v[3 * i + 2]; d_out[3] = 0.0f;
                d_out += 4;
            }
        }
    }
    if (!b_out) return GLRT_HOST_OK;
    for (int k = levels - 1; k >= 1; k--) {  // U_k = D_k + up(U_{k+1}), in place
        Plane &P = D[(size_t)k];
        const Plane &C = D[(size_t)k + 1];
        for (int y = 0; y < P.h; y++)
            for (int x = 0; x < P.w; x++)
                for (int c = 0; c < 3; c++) P.at(x, y)[c] = P.at(x, y)[c] + up_at(C, x, y, c);
    }
    const float inv_levels = 1.0f / (float)levels;
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            float v[3];
            pixel_value(src + 4 * ((size_t)y * width + x), v);
            float *o = b_out + 4 * ((size_t)y * width + x);
            for (int c = 0; c < 3; c++) o[c] = v[c] + strength * (up_at(D[1], x, y, c) * inv_levels);
            o[3] = 1.0f;
        }
    return GLRT_HOST_OK;
}
