// skin.cpp -- glrt_skin_vertices (include/glrt_host.h): the CPU statement of the device's skinning pass (glrtx_pose, glrtx_debug_skin, include/glrtx.h
// "Posing"; csrc/skin.hip.h).  The contract is the text in include/glrtx.h; tests/skin_math.py restates it in numpy.  Every fp32 operation below is one correctly
// rounded IEEE operation in the order written (-ffp-contract=off), under MXCSR FTZ | DAZ.
#include <cmath>
#include <cstring>

#include "glrt_host.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

constexpr int kV = GLRT_VERTEX_FLOATS;

float blend(const float *w, const float *const m[4], int e) { return ((w[0] * m[0][e] + w[1] * m[1][e]) + w[2] * m[2][e]) + w[3] * m[3][e]; }

}  // namespace

int glrt_skin_vertices(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *matrices, int n_bones,
                       float *vert_out) {
    if (n_bones < 1 || n_bones > GLRT_MAX_BONES || !matrices || (n_vert > 0 && (!rest_vert || !bones4 || !weights4 || !vert_out))) return GLRT_HOST_EINVAL;
    for (size_t k = 0; k < 4 * n_vert; k++)
        if (bones4[k] < 0 || bones4[k] >= n_bones) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    for (size_t i = 0; i < n_vert; i++) {
        const float *in = rest_vert + kV * i, *w = weights4 + 4 * i;
        const int32_t *b = bones4 + 4 * i;
        const float *const m[4] = {matrices + 12 * (size_t)b[0], matrices + 12 * (size_t)b[1], matrices + 12 * (size_t)b[2], matrices + 12 * (size_t)b[3]};
        float B[3][4];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) B[r][c] = blend(w, m, 4 * r + c);
        float *o = vert_out + kV * i;
        const float *p = in, *n = in + 3, *t = in + 9, *bn = in + 12;
        float pos[3], v[3], tg[3], bi[3];
        for (int r = 0; r < 3; r++) {
            pos[r] = dot3(B[r][0], B[r][1], B[r][2], p[0], p[1], p[2]) + B[r][3];
            tg[r] = dot3(B[r][0], B[r][1], B[r][2], t[0], t[1], t[2]);
            bi[r] = dot3(B[r][0], B[r][1], B[r][2], bn[0], bn[1], bn[2]);
        }
        // the cofactor matrix of L = B[:, 0..2], row r from rows r + 1 and r + 2 (cyclically)
        for (int r = 0; r < 3; r++) {
            const float *x = B[(r + 1) % 3], *y = B[(r + 2) % 3];
            const float c0 = x[1] * y[2] - x[2] * y[1], c1 = x[2] * y[0] - x[0] * y[2], c2 = x[0] * y[1] - x[1] * y[0];
            v[r] = dot3(c0, c1, c2, n[0], n[1], n[2]);
        }
        const float s = dot3(v[0], v[1], v[2], v[0], v[1], v[2]);
        const float l = std::sqrt(s);
        const bool unit = l > 0.0f;
        std::memcpy(o + 6, in + 6, 3 * sizeof(float));  // uv: moved as integers
        for (int r = 0; r < 3; r++) {
            const float nr = unit ? v[r] / l : v[r];
            o[r] = canon(pos[r]);
            o[3 + r] = canon(nr);
            o[9 + r] = canon(tg[r]);
            o[12 + r] = canon(bi[r]);
        }
    }
    return GLRT_HOST_OK;
}
