// reweight.cpp -- glrt_fold_cascades and glrt_reweight (include/glrt_host.h): the CPU statements of the device's cascade fold and of its resolve
// (glrtx_render_cascades, glrtx_reweight, include/glrtx.h "Firefly re-weighting"; csrc/reweight.hip.h; Zirr, Hanika and Dachsbacher 2018).  The contract is the
// text in include/glrtx.h; tests/reweight_math.py restates it in numpy.  Every fp32 operation below is one correctly rounded IEEE operation in the order written
// (-ffp-contract=off), under MXCSR FTZ | DAZ.
#include <cmath>
#include <vector>

#include "glrt_host.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

constexpr int kCascades = GLRT_CASCADES;

bool start_ok(float s) { return s >= 0x1p-20f && s <= 0x1p20f; }  // (a NaN fails both)

}  // namespace

int glrt_fold_cascades(float *cascades, float *accum, const float *planes, int n_planes, int width, int rows, float start) {
    if (!cascades || (n_planes > 0 && !planes) || n_planes < 0 || width < 1 || rows < 1 || width > 65536 || rows > 65536 || !start_ok(start)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const size_t n = (size_t)width * rows;
    float b[kCascades];
    b[0] = start;
    for (int k = 1; k < kCascades; k++) b[k] = b[k - 1] * 8.0f;
    for (int f = 0; f < n_planes; f++)
        for (size_t i = 0; i < n; i++) {
            const float *v = planes + 4 * ((size_t)f * n + i);
            const float l = lum(v[0], v[1], v[2]);
            int j = 0;
            for (int k = 1; k <= 4; k++)
                if (l >= b[k]) j = k;
            const float lower = b[j], upper = b[j + 1];
            float wl, wu;
            int jc = j;
            if (!(l > lower)) { wl = 1.0f; wu = 0.0f; }
            else if (l >= upper) { wl = 0.0f; wu = 1.0f; jc = 5; }
            else {
                const float q = lower / l;
                wl = (q - 0.125f) / 0.875f;
                wl = wl > 0.0f ? wl : 0.0f;
                wl = wl < 1.0f ? wl : 1.0f;
                wu = 1.0f - wl;
            }
            float *cl = cascades + 4 * ((size_t)j * n + i), *cu = cascades + 4 * ((size_t)(j + 1) * n + i), *cc = cascades + 4 * ((size_t)jc * n + i);
            for (int ch = 0; ch < 3; ch++) cl[ch] = cl[ch] + wl * v[ch];
            for (int ch = 0; ch < 3; ch++) cu[ch] = cu[ch] + wu * v[ch];
            cc[3] = cc[3] + 1.0f;
            if (accum) {
                float *a = accum + 4 * i;
                a[0] = a[0] + v[0]; a[1] = a[1] + v[1]; a[2] = a[2] + v[2];
                a[3] = a[3] + 1.0f;
            }
        }
    return GLRT_HOST_OK;
}

int glrt_reweight(const float *cascades, int width, int rows, float kappa, float *out) {
    if (!cascades || !out || width < 1 || rows < 1 || width > 65536 || rows > 65536 || !(kappa > 0.0f) || std::isinf(kappa)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    const size_t n = (size_t)width * rows;
    std::vector<float> T((kCascades - 1) * n);  // T_0 .. T_4
    for (size_t i = 0; i < n; i++) {
        float t = cascades[4 * (5 * n + i) + 3];
        for (int k = 4; k >= 0; k--) { t = t + cascades[4 * ((size_t)k * n + i) + 3]; T[(size_t)k * n + i] = t; }
    }
    for (int y = 0; y < rows; y++)
        for (int x = 0; x < width; x++) {
            const size_t p = (size_t)y * width + x;
            float *o = out + 4 * p;
            o[0] = o[1] = o[2] = 0.0f; o[3] = 1.0f;
            const float cnt = T[p];
            if (tiny(cnt) || cnt != cnt) continue;
            float a[3] = {cascades[4 * p], cascades[4 * p + 1], cascades[4 * p + 2]};
            for (int j = 1; j < kCascades; j++) {
                const float *Tj = T.data() + (size_t)(j - 1) * n;
                float s = 0.0f;
                for (int dy = -1; dy <= 1; dy++)
                    for (int dx = -1; dx <= 1; dx++) {
                        const int qx = x + dx, qy = y + dy;
                        if (qx < 0 || qx >= width || qy < 0 || qy >= rows) continue;
                        s = s + Tj[(size_t)qy * width + qx];
                    }
                s = s - 1.0f;
                s = s > 0.0f ? s : 0.0f;
                float r = s / kappa;
                r = r < 1.0f ? r : 1.0f;
                const float *cj = cascades + 4 * ((size_t)j * n + p);
                for (int ch = 0; ch < 3; ch++) a[ch] = a[ch] + r * cj[ch];
            }
            for (int ch = 0; ch < 3; ch++) o[ch] = canon(a[ch] / cnt);
        }
    return GLRT_HOST_OK;
}
