// reproject_lookup.h -- the history of one world point in the old view, shared by glrt_reproject and glrt_reproject_motion (host/reproject.cpp,
// host/reproject_motion.cpp) as csrc/reproject.hip.h's history_lookup is shared by the two kernels: the callers differ in where the point and the normal to
// test come from, and in nothing else.  One correctly rounded fp32 operation at a time in the order written; the caller runs with denormals flushed.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "reproject_moments.h"
#include "reproject_setup.h"
#include "statement_math.h"

namespace glrt_detail {

constexpr float kMinWeight = 1.0e-6f;  // a pixel whose taps weigh less than this in sum has no history

// The old view: accumulator, moments plane M (or null) and the planes N0 / A0, packed rows of `width`.
struct OldView {
    const float *accum, *mom, *n0, *a0;
    int width, rows;
};

// P through W and S to the old image; the four taps around it that show material `id` with a count, a normal within normal_tolerance of N and a depth within
// depth_tolerance of P's distance to the old camera; their weighted mean times the rounded, capped count.  True: o (and, with mo, the moments) are written.
// False: no history, nothing is written (the callers have stored zeros).
inline bool history_lookup(const ReprojectSetup &st, const OldView &v, float Px, float Py, float Pz, float Nx, float Ny, float Nz, int32_t id, float *o, float *mo) {
    const float *W = st.W, *S = st.S;
    const float Wf = (float)v.width, Hf = (float)v.rows;
    const float qx = ((W[0] * Px + W[4] * Py) + W[8] * Pz) + W[12];
    const float qy = ((W[1] * Px + W[5] * Py) + W[9] * Pz) + W[13];
    const float qz = ((W[2] * Px + W[6] * Py) + W[10] * Pz) + W[14];
    const float qw = ((W[3] * Px + W[7] * Py) + W[11] * Pz) + W[15];
    const float sx = ((S[0] * qx + S[4] * qy) + S[8] * qz) + S[12] * qw;
    const float sy = ((S[1] * qx + S[5] * qy) + S[9] * qz) + S[13] * qw;
    const float sw4 = ((S[3] * qx + S[7] * qy) + S[11] * qz) + S[15] * qw;
    const float ui = ((sx / sw4 + 1.0f) * 0.5f) * Wf + -1.0f;
    const float vi = ((sy / sw4 + 1.0f) * 0.5f) * Hf + -1.0f;
    if (!(pos_finite(sw4) && ui >= -1.0f && ui < Wf && vi >= -1.0f && vi < Hf)) return false;  // no tap inside the image (a NaN fails)
    const float ex = Px - st.o_prev[0], ey = Py - st.o_prev[1], ez = Pz - st.o_prev[2];
    const float e = std::sqrt((ez * ez + ey * ey) + ex * ex);
    const float lim = st.depth_tolerance * e;
    const float fx0 = std::floor(ui), fy0 = std::floor(vi);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = ui - fx0, fy = vi - fy0;
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    float sw = 0.0f, sc = 0.0f, sI[3] = {0.0f, 0.0f, 0.0f};
    MomSum ms;
    for (int j = 0; j < 2; j++)
        for (int i = 0; i < 2; i++) {
            const int tx = x0 + i, ty = y0 + j;
            if (tx < 0 || tx >= v.width || ty < 0 || ty >= v.rows) continue;
            const size_t q = (size_t)ty * v.width + tx;
            const float *C = v.accum + 4 * q, *N0 = v.n0 + 4 * q;
            int32_t id0;
            std::memcpy(&id0, v.a0 + 4 * q + 3, 4);
            if (id0 != id || tiny(C[3])) continue;
            if (!(dot3(Nx, Ny, Nz, N0[0], N0[1], N0[2]) >= st.normal_tolerance)) continue;
            if (!(std::fabs(N0[3] - e) <= lim)) continue;
            const float w = wx[i] * wy[j];
            sw = sw + w;
            sc = sc + w * C[3];
            for (int k = 0; k < 3; k++) sI[k] = sI[k] + w * (C[k] / C[3]);
            if (v.mom) moments_tap(ms, w, v.mom + 4 * q);
        }
    if (!(sw > kMinWeight)) return false;
    const float r = std::nearbyint(sc / sw);
    const float n = r > st.max_history ? st.max_history : r;
    if (!(n >= 1.0f)) return false;
    for (int k = 0; k < 3; k++) o[k] = canon((sI[k] / sw) * n);
    o[3] = n;
    if (mo) moments_out(ms, st.max_history, mo);
    return true;
}

}  // namespace glrt_detail
