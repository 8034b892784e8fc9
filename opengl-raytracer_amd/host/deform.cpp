// deform.cpp -- the CPU statements of the device's pose kernels (include/glrt_host.h; csrc/skin.hip.h), and glrt_dualquat_from_matrix.  glrt_skin_vertices
// states the skinning pass (glrtx_pose, glrtx_debug_skin, include/glrtx.h "Posing": skin_kernel), glrt_deform_vertices the deform pass (glrtx_pose_morph,
// glrtx_pose_dualquat, glrtx_debug_deform, "Deforming": deform_kernel), glrt_deform_vertices_sparse the same over a sparse set (deform_sparse_kernel);
// glrt_morph_sparsify makes a sparse set from dense deltas.  The contract is the text in include/glrtx.h; tests/skin_math.py, tests/deform_math.py and
// tests/deform_sparse_math.py restate it in numpy.  Every fp32 operation of the statements is one correctly rounded IEEE operation in the order written
// (-ffp-contract=off), under MXCSR FTZ | DAZ.  The three share skin_stage: from B = [L | t] on, a vertex is Posing's whichever call made B.
#include <cmath>
#include <cstring>

#include <vector>

#include "glrt_host.h"
#include "morph_sparse.h"
#include "statement_math.h"

namespace {

using namespace glrt_detail;

constexpr int kV = GLRT_VERTEX_FLOATS;

float blend(const float *w, const float *const m[4], int e) { return ((w[0] * m[0][e] + w[1] * m[1][e]) + w[2] * m[2][e]) + w[3] * m[3][e]; }
float dot4(const float *a, const float *b) { return ((a[3] * b[3] + a[2] * b[2]) + a[1] * b[1]) + a[0] * b[0]; }

// B of a vertex from dual quaternions: sign, blend, normalise, rotation, translation
void dualquat_matrix(const float *w, const float *const q[4], float B[3][4]) {
    float s[4] = {w[0], w[1], w[2], w[3]};
    for (int k = 1; k < 4; k++)
        if (dot4(q[0], q[k]) < 0.0f) s[k] = -w[k];
    float Q[8];
    for (int e = 0; e < 8; e++) Q[e] = blend(s, q, e);
    const float l = std::sqrt(dot4(Q, Q));
    if (l > 0.0f)
        for (int e = 0; e < 8; e++) Q[e] = Q[e] / l;
    const float *R = Q, *D = Q + 4;
    const float xx = R[0] * R[0], yy = R[1] * R[1], zz = R[2] * R[2], xy = R[0] * R[1], xz = R[0] * R[2], yz = R[1] * R[2];
    const float wx = R[3] * R[0], wy = R[3] * R[1], wz = R[3] * R[2];
    B[0][0] = 1.0f - 2.0f * (yy + zz); B[0][1] = 2.0f * (xy - wz); B[0][2] = 2.0f * (xz + wy);
    B[1][0] = 2.0f * (xy + wz); B[1][1] = 1.0f - 2.0f * (xx + zz); B[1][2] = 2.0f * (yz - wx);
    B[2][0] = 2.0f * (xz - wy); B[2][1] = 2.0f * (yz + wx); B[2][2] = 1.0f - 2.0f * (xx + yy);
    for (int i = 0; i < 3; i++) {
        const int j = (i + 1) % 3, k = (i + 2) % 3;
        B[i][3] = 2.0f * (((R[3] * D[i] - D[3] * R[i]) + R[j] * D[k]) - R[k] * D[j]);
    }
}

// The skinning stage of one vertex: B from matrices or dual quaternions, then Posing from B on.  p, n: the (morphed) position and normal.
void skin_stage(const float *in, const int32_t *b, const float *w, const float *bone_data, int stride, int mode, const float p[3], const float n[3], float *o) {
    const float *const m[4] = {bone_data + stride * (size_t)b[0], bone_data + stride * (size_t)b[1], bone_data + stride * (size_t)b[2],
                               bone_data + stride * (size_t)b[3]};
    float B[3][4];
    if (mode) dualquat_matrix(w, m, B);
    else
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 4; c++) B[r][c] = blend(w, m, 4 * r + c);
    const float *t = in + 9, *bn = in + 12;
    float pos[3], v[3], tg[3], bi[3];
    for (int r = 0; r < 3; r++) {
        pos[r] = dot3(B[r][0], B[r][1], B[r][2], p[0], p[1], p[2]) + B[r][3];
        tg[r] = dot3(B[r][0], B[r][1], B[r][2], t[0], t[1], t[2]);
        bi[r] = dot3(B[r][0], B[r][1], B[r][2], bn[0], bn[1], bn[2]);
    }
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

// What the three statements refuse alike: the bone count, a missing buffer, a vertex that names a bone outside the rig
bool rig_ok(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, const float *vert_out) {
    if (n_bones < 1 || n_bones > GLRT_MAX_BONES || !bone_data || (n_vert > 0 && (!rest_vert || !bones4 || !weights4 || !vert_out))) return false;
    for (size_t k = 0; k < 4 * n_vert; k++)
        if (bones4[k] < 0 || bones4[k] >= n_bones) return false;
    return true;
}

}  // namespace

int glrt_skin_vertices(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *matrices, int n_bones,
                       float *vert_out) {
    if (!rig_ok(rest_vert, n_vert, bones4, weights4, matrices, n_bones, vert_out)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    for (size_t i = 0; i < n_vert; i++) {
        const float *in = rest_vert + kV * i;
        skin_stage(in, bones4 + 4 * i, weights4 + 4 * i, matrices, 12, 0, in, in + 3, vert_out + kV * i);
    }
    return GLRT_HOST_OK;
}

int glrt_deform_vertices(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                         const float *deltas, const float *morph_weights, int n_targets, float *vert_out) {
    if (!rig_ok(rest_vert, n_vert, bones4, weights4, bone_data, n_bones, vert_out)) return GLRT_HOST_EINVAL;
    if ((mode != 0 && mode != 1) || n_targets < 0 || n_targets > GLRT_MAX_MORPH_TARGETS) return GLRT_HOST_EINVAL;
    if (n_targets > 0 && (!morph_weights || (n_vert > 0 && !deltas))) return GLRT_HOST_EINVAL;
    for (int k = 0; k < n_targets; k++)
        if (!std::isfinite(morph_weights[k])) return GLRT_HOST_EINVAL;
    // the active targets: a weight that is not a zero after the flush
    int active[GLRT_MAX_MORPH_TARGETS], n_active = 0;
    for (int k = 0; k < n_targets; k++)
        if (!tiny(morph_weights[k])) active[n_active++] = k;
    FlushDenormals ftz;
    const int stride = mode ? 8 : 12;
    for (size_t i = 0; i < n_vert; i++) {
        const float *in = rest_vert + kV * i, *w = weights4 + 4 * i;
        const int32_t *b = bones4 + 4 * i;
        // Morph
        float p[3] = {in[0], in[1], in[2]}, n[3] = {in[3], in[4], in[5]};
        for (int a = 0; a < n_active; a++) {
            const float wk = morph_weights[active[a]];
            const float *d = deltas + ((size_t)active[a] * n_vert + i) * 6;
            for (int r = 0; r < 3; r++) {
                p[r] = p[r] + wk * d[r];
                n[r] = n[r] + wk * d[3 + r];
            }
        }
        skin_stage(in, b, w, bone_data, stride, mode, p, n, vert_out + kV * i);
    }
    return GLRT_HOST_OK;
}

int glrt_deform_vertices_sparse(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                                const uint64_t *offsets, const uint32_t *vertex, const float *deltas, const float *morph_weights, int n_targets, float *vert_out) {
    if (!rig_ok(rest_vert, n_vert, bones4, weights4, bone_data, n_bones, vert_out)) return GLRT_HOST_EINVAL;
    if (mode != 0 && mode != 1) return GLRT_HOST_EINVAL;
    SparseFault fault;
    if (!morph_sparse_check(offsets, vertex, deltas, n_targets, n_vert, fault)) return GLRT_HOST_EINVAL;
    if (n_targets > 0 && !morph_weights) return GLRT_HOST_EINVAL;
    for (int k = 0; k < n_targets; k++)
        if (!std::isfinite(morph_weights[k])) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    // Morph: the targets in ascending index, each active one's entries onto the vertices they list -- per vertex that is the entries that list it, in ascending
    // target index.  A vertex no active target lists keeps the rest words.
    std::vector<float> pn(6 * n_vert);
    for (size_t i = 0; i < n_vert; i++) std::memcpy(&pn[6 * i], rest_vert + kV * i, 6 * sizeof(float));
    for (int k = 0; k < n_targets; k++) {
        const float wk = morph_weights[k];
        if (tiny(wk)) continue;  // inactive: its entries never enter the arithmetic
        for (uint64_t e = offsets[k]; e < offsets[k + 1]; e++) {
            float *q = &pn[6 * (size_t)vertex[e]];
            const float *d = deltas + 6 * e;
            for (int r = 0; r < 6; r++) q[r] = q[r] + wk * d[r];
        }
    }
    const int stride = mode ? 8 : 12;
    for (size_t i = 0; i < n_vert; i++)
        skin_stage(rest_vert + kV * i, bones4 + 4 * i, weights4 + 4 * i, bone_data, stride, mode, &pn[6 * i], &pn[6 * i + 3], vert_out + kV * i);
    return GLRT_HOST_OK;
}

int glrt_morph_sparsify(const float *dense_deltas, int n_targets, size_t n_vert, uint64_t *offsets, uint32_t *vertex_out, float *deltas_out) {
    if (n_targets < 0 || n_targets > GLRT_MAX_SPARSE_MORPH_TARGETS || !offsets || n_vert >= ((size_t)1 << 32)) return GLRT_HOST_EINVAL;
    if (n_targets > 0 && n_vert > 0 && !dense_deltas) return GLRT_HOST_EINVAL;
    if (vertex_out && !deltas_out) return GLRT_HOST_EINVAL;
    uint64_t nnz = 0;
    offsets[0] = 0;
    for (int k = 0; k < n_targets; k++) {
        for (size_t i = 0; i < n_vert; i++) {
            const float *d = dense_deltas + ((size_t)k * n_vert + i) * 6;
            if (!morph_entry_kept(d)) continue;
            if (vertex_out) {
                vertex_out[nnz] = (uint32_t)i;
                std::memcpy(deltas_out + 6 * nnz, d, 6 * sizeof(float));
            }
            nnz++;
        }
        offsets[k + 1] = nnz;
    }
    return GLRT_HOST_OK;
}

void glrt_dualquat_from_matrix(const float m[12], float dq[8]) {
    const double m00 = m[0], m01 = m[1], m02 = m[2], m10 = m[4], m11 = m[5], m12 = m[6], m20 = m[8], m21 = m[9], m22 = m[10];
    const double t[3] = {m[3], m[7], m[11]};
    double q[4];  // x, y, z, w: the largest of the four is taken from the diagonal, the others from the off-diagonal sums (Shepperd)
    const double tr = m00 + m11 + m22;
    if (tr > 0.0) {
        const double s = 2.0 * std::sqrt(tr + 1.0);
        q[3] = 0.25 * s; q[0] = (m21 - m12) / s; q[1] = (m02 - m20) / s; q[2] = (m10 - m01) / s;
    } else if (m00 > m11 && m00 > m22) {
        const double s = 2.0 * std::sqrt(1.0 + m00 - m11 - m22);
        q[3] = (m21 - m12) / s; q[0] = 0.25 * s; q[1] = (m01 + m10) / s; q[2] = (m02 + m20) / s;
    } else if (m11 > m22) {
        const double s = 2.0 * std::sqrt(1.0 + m11 - m00 - m22);
        q[3] = (m02 - m20) / s; q[0] = (m01 + m10) / s; q[1] = 0.25 * s; q[2] = (m12 + m21) / s;
    } else {
        const double s = 2.0 * std::sqrt(1.0 + m22 - m00 - m11);
        q[3] = (m10 - m01) / s; q[0] = (m02 + m20) / s; q[1] = (m12 + m21) / s; q[2] = 0.25 * s;
    }
    const double len = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const double sign = q[3] < 0.0 ? -1.0 : 1.0;
    for (double &v : q) v = sign * v / len;
    // d = 1/2 (t, 0) * r: vector part r.w t + t x r.xyz, scalar part -t . r.xyz
    const double d[4] = {0.5 * (q[3] * t[0] + (t[1] * q[2] - t[2] * q[1])), 0.5 * (q[3] * t[1] + (t[2] * q[0] - t[0] * q[2])),
                         0.5 * (q[3] * t[2] + (t[0] * q[1] - t[1] * q[0])), -0.5 * (t[0] * q[0] + t[1] * q[1] + t[2] * q[2])};
    for (int k = 0; k < 4; k++) {
        dq[k] = (float)q[k];
        dq[4 + k] = (float)d[k];
    }
}
