// skin.hip.h -- posing: linear-blend skinning of the uploaded scene's vertices (glrtx_upload_rig, glrtx_pose, glrtx_debug_skin, include/glrtx.h "Posing").  A
// rigid object is the one-bone case {obj, 0, 0, 0} / {1, 0, 0, 0}.  The pass runs in front of the refit (refit.hip.h): rest pose + rig + pose matrices -> wire
// vertices in the context's vertex buffer, which the refit then reads exactly as it reads uploaded ones.
//
// No reference counterpart.  The arithmetic is the header's text: host/deform.cpp (glrt_skin_vertices) and tests/skin_math.py state it again, and all three agree
// bit for bit under denoise.hip.h's rules (one correctly rounded fp32 operation at a time in the order written, -ffp-contract=off; denormals flushed; a stored
// NaN is 0x7FC00000).  All four blend terms are formed whatever the weights are, so the operation sequence does not depend on the data.
//
//   skin_kernel  one thread per vertex, 256-thread workgroups.  Per vertex: the 60-byte rest record as 15 dword loads (a record is 60 bytes, so a lane's record is
//       not 16-byte aligned; the 64 records of a wave are 3840 contiguous bytes, so every cache line a wave touches is used whole), the 32-byte rig record {b[4],
//       w[4]} as two 16-byte loads, 4 x 48 bytes of matrices as twelve 16-byte loads (a pose is a few kilobytes: cache-resident), 15 dword stores.  152 bytes of
//       compulsory traffic per vertex.  No LDS, no atomics, no scratch.
//
// Deforming (glrtx_upload_morph_targets, glrtx_pose_morph, glrtx_pose_dualquat, glrtx_debug_deform; include/glrtx.h "Deforming"): morph targets in front of the
// skinning stage, and dual quaternions as a second way to state a bone.  host/deform.cpp (glrt_deform_vertices) and tests/deform_math.py state it again.
//
//   deform_kernel<DQ>  skin_kernel's shape: one thread per vertex, 256-thread workgroups, no LDS, no atomics, no scratch.  The active morph targets arrive
//       compacted by the host in the kernel's arguments -- a count, and an index and a weight per target --, so the loop's trip count, the weights and each
//       target's base address are scalar (s_load from the argument segment, scalar address arithmetic); only the deltas are per-lane loads.  The deltas keep the
//       layout they are uploaded in, target-major and dense, 24 bytes {dpos, dnormal} a vertex: a lane reads its record as three 8-byte loads (24 i is 8-byte
//       aligned), a wave's 64 records are 1536 contiguous bytes, and a target that is not active is never touched because no byte of it lies between the bytes
//       of one that is.  DQ = false: bones are skin_kernel's 48-byte matrices, 152 + 24 active bytes a vertex.  DQ = true: a bone is 32 bytes {r, d}, two
//       16-byte loads a bone and lane, 136 + 24 active bytes a vertex; sign, blend, normalise, and the 3x4 matrix [L | t] of the blended dual quaternion.  Both
//       end in the same tail (transform_store), which is skin_kernel's arithmetic from B on.
//
// Sparse targets (glrtx_upload_morph_targets_sparse; include/glrtx.h "Deforming", SPARSE TARGETS): a target lists only the vertices it moves, up to 1024 a rig.
// host/deform.cpp (glrt_deform_vertices_sparse) and tests/deform_sparse_math.py state it again.
//
//   deform_sparse_kernel<DQ>  deform_kernel's shape: one thread per vertex, 256-thread workgroups, no atomics, no scratch.  The set arrives as a vertex-major
//       inverted index built on the host: row[n_vert + 1], and the entries in row order, ascending by target inside a row -- each destination sums its own
//       list in a fixed order (a gather), so nothing is shared between lanes and the result is reproducible bit for bit.  An entry is 32 bytes {target, dpos}
//       {dnormal, 0}, two 16-byte loads; a lane reads row[i] and row[i + 1] (a wave: 260 contiguous bytes) and walks its row, a lane-dependent trip count.  The
//       pose's weight table (n_targets floats, exact +0 for an inactive target) is staged once a workgroup in LDS, 4 KB, and looked up per lane by the
//       entry's target; an entry under a zero weight is skipped without touching p or n.  One barrier behind the staging: the body is guarded by i < n_vert and
//       NO thread returns in front of the barrier.  The blend and the dual-quaternion block are deform_kernel's text repeated (the existing kernels are not
//       edited: moving a loop into a shared body has renumbered a kernel here before); the tail is transform_store, shared.  152 + 4 bytes a vertex plus 32 an
//       entry (DQ: 136 + 4).
#pragma once
#include "denoise.hip.h"

namespace glrtx {
namespace skin {

constexpr int kBlock = 256;
constexpr int kVertexWords = 15;  // GLRT_VERTEX_FLOATS: pos, normal, uv, tangent, binormal

struct Args {
    const unsigned *rest;  // n_vert x 15 words: the rest pose, wire format
    const uint4 *rig;      // n_vert x 2: {b0, b1, b2, b3} (int32, each within [0, n_bones): checked on the host before the upload), {w0, w1, w2, w3} (float)
    const float4 *pose;    // n_bones x 3: the rows of the 3x4 matrices
    unsigned *out;         // n_vert x 15 words
    size_t n_vert;
};

// the project's order (pt_kernel.hip.h: dot): (a2 v.z + a1 v.y) + a0 v.x
DEV float dot3(float a0, float a1, float a2, float vx, float vy, float vz) { return (a2 * vz + a1 * vy) + a0 * vx; }
DEV float blend(float w0, float w1, float w2, float w3, float m0, float m1, float m2, float m3) { return ((w0 * m0 + w1 * m1) + w2 * m2) + w3 * m3; }
DEV float4 blend_row(const float4 w, const float4 m0, const float4 m1, const float4 m2, const float4 m3) {
    return make_float4(blend(w.x, w.y, w.z, w.w, m0.x, m1.x, m2.x, m3.x), blend(w.x, w.y, w.z, w.w, m0.y, m1.y, m2.y, m3.y),
                       blend(w.x, w.y, w.z, w.w, m0.z, m1.z, m2.z, m3.z), blend(w.x, w.y, w.z, w.w, m0.w, m1.w, m2.w, m3.w));
}
DEV unsigned word(float x) { return __float_as_uint(denoise::canon(x)); }

__global__ __launch_bounds__(kBlock) void skin_kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_vert) return;
    const unsigned *r = a.rest + kVertexWords * i;
    unsigned in[kVertexWords];
#pragma unroll
    for (int k = 0; k < kVertexWords; k++) in[k] = r[k];
    const uint4 b = a.rig[2 * i];
    const uint4 wu = a.rig[2 * i + 1];
    const float4 w = make_float4(__uint_as_float(wu.x), __uint_as_float(wu.y), __uint_as_float(wu.z), __uint_as_float(wu.w));
    const float4 *m0 = a.pose + 3 * (size_t)b.x, *m1 = a.pose + 3 * (size_t)b.y, *m2 = a.pose + 3 * (size_t)b.z, *m3 = a.pose + 3 * (size_t)b.w;
    // Blend: B = ((w0 M_b0 + w1 M_b1) + w2 M_b2) + w3 M_b3, all twelve entries; B0 .. B2 are B's rows {L[i][0], L[i][1], L[i][2], translation}
    const float4 B0 = blend_row(w, m0[0], m1[0], m2[0], m3[0]);
    const float4 B1 = blend_row(w, m0[1], m1[1], m2[1], m3[1]);
    const float4 B2 = blend_row(w, m0[2], m1[2], m2[2], m3[2]);

    const float px = __uint_as_float(in[0]), py = __uint_as_float(in[1]), pz = __uint_as_float(in[2]);
    const float nx = __uint_as_float(in[3]), ny = __uint_as_float(in[4]), nz = __uint_as_float(in[5]);
    const float tx = __uint_as_float(in[9]), ty = __uint_as_float(in[10]), tz = __uint_as_float(in[11]);
    const float bx = __uint_as_float(in[12]), by = __uint_as_float(in[13]), bz = __uint_as_float(in[14]);

    unsigned o[kVertexWords];
    // Position
    o[0] = word(dot3(B0.x, B0.y, B0.z, px, py, pz) + B0.w);
    o[1] = word(dot3(B1.x, B1.y, B1.z, px, py, pz) + B1.w);
    o[2] = word(dot3(B2.x, B2.y, B2.z, px, py, pz) + B2.w);
    // Cofactor matrix of L (det L^-T): two rounded products and one subtraction an entry
    const float c00 = B1.y * B2.z - B1.z * B2.y, c01 = B1.z * B2.x - B1.x * B2.z, c02 = B1.x * B2.y - B1.y * B2.x;
    const float c10 = B2.y * B0.z - B2.z * B0.y, c11 = B2.z * B0.x - B2.x * B0.z, c12 = B2.x * B0.y - B2.y * B0.x;
    const float c20 = B0.y * B1.z - B0.z * B1.y, c21 = B0.z * B1.x - B0.x * B1.z, c22 = B0.x * B1.y - B0.y * B1.x;
    // Normal
    const float vx = dot3(c00, c01, c02, nx, ny, nz), vy = dot3(c10, c11, c12, nx, ny, nz), vz = dot3(c20, c21, c22, nx, ny, nz);
    const float s = dot3(vx, vy, vz, vx, vy, vz);
    const float l = __builtin_sqrtf(s);
    const bool unit = l > 0.0f;
    o[3] = word(unit ? vx / l : vx);
    o[4] = word(unit ? vy / l : vy);
    o[5] = word(unit ? vz / l : vz);
    // uv: moved as integers
    o[6] = in[6]; o[7] = in[7]; o[8] = in[8];
    // Tangent and binormal: L times the vector, not normalised
    o[9] = word(dot3(B0.x, B0.y, B0.z, tx, ty, tz));
    o[10] = word(dot3(B1.x, B1.y, B1.z, tx, ty, tz));
    o[11] = word(dot3(B2.x, B2.y, B2.z, tx, ty, tz));
    o[12] = word(dot3(B0.x, B0.y, B0.z, bx, by, bz));
    o[13] = word(dot3(B1.x, B1.y, B1.z, bx, by, bz));
    o[14] = word(dot3(B2.x, B2.y, B2.z, bx, by, bz));
    unsigned *d = a.out + kVertexWords * i;
#pragma unroll
    for (int k = 0; k < kVertexWords; k++) d[k] = o[k];
}

// ---- Deforming
constexpr int kMaxTargets = 64;  // GLRTX_MAX_MORPH_TARGETS
constexpr int kDeltaWords = 6;   // {dpos, dnormal}

// The active targets of one pose, compacted by the host (a target is active iff its weight is not a zero after the flush): wave-uniform
struct Morph {
    int n_active;
    unsigned index[kMaxTargets];
    float weight[kMaxTargets];
};

struct DeformArgs {
    const unsigned *rest;  // as Args
    const uint4 *rig;
    const float4 *pose;    // DQ = false: n_bones x 3 matrix rows; DQ = true: n_bones x 2 {r.x, r.y, r.z, r.w} {d.x, d.y, d.z, d.w}
    unsigned *out;
    size_t n_vert;
    const float2 *deltas;  // n_targets x n_vert x 3: {dpos.x, dpos.y} {dpos.z, dnormal.x} {dnormal.y, dnormal.z}; never read when n_active == 0
    Morph morph;
};

DEV float dot4(const float4 a, const float4 b) { return ((a.w * b.w + a.z * b.z) + a.y * b.y) + a.x * b.x; }
DEV float4 quot4(const float4 a, float l, bool unit) { return make_float4(unit ? a.x / l : a.x, unit ? a.y / l : a.y, unit ? a.z / l : a.z, unit ? a.w / l : a.w); }

// Posing from B on: position, the normal through the cofactor matrix, tangent and binormal, uv as words.  p, n: the (morphed) position and normal; `in`: the
// rest record, for uv, tangent and binormal.
DEV void transform_store(const float4 B0, const float4 B1, const float4 B2, const unsigned (&in)[kVertexWords], float px, float py, float pz, float nx, float ny,
                         float nz, unsigned *d) {
    const float tx = __uint_as_float(in[9]), ty = __uint_as_float(in[10]), tz = __uint_as_float(in[11]);
    const float bx = __uint_as_float(in[12]), by = __uint_as_float(in[13]), bz = __uint_as_float(in[14]);
    unsigned o[kVertexWords];
    o[0] = word(dot3(B0.x, B0.y, B0.z, px, py, pz) + B0.w);
    o[1] = word(dot3(B1.x, B1.y, B1.z, px, py, pz) + B1.w);
    o[2] = word(dot3(B2.x, B2.y, B2.z, px, py, pz) + B2.w);
    const float c00 = B1.y * B2.z - B1.z * B2.y, c01 = B1.z * B2.x - B1.x * B2.z, c02 = B1.x * B2.y - B1.y * B2.x;
    const float c10 = B2.y * B0.z - B2.z * B0.y, c11 = B2.z * B0.x - B2.x * B0.z, c12 = B2.x * B0.y - B2.y * B0.x;
    const float c20 = B0.y * B1.z - B0.z * B1.y, c21 = B0.z * B1.x - B0.x * B1.z, c22 = B0.x * B1.y - B0.y * B1.x;
    const float vx = dot3(c00, c01, c02, nx, ny, nz), vy = dot3(c10, c11, c12, nx, ny, nz), vz = dot3(c20, c21, c22, nx, ny, nz);
    const float s = dot3(vx, vy, vz, vx, vy, vz);
    const float l = __builtin_sqrtf(s);
    const bool unit = l > 0.0f;
    o[3] = word(unit ? vx / l : vx);
    o[4] = word(unit ? vy / l : vy);
    o[5] = word(unit ? vz / l : vz);
    o[6] = in[6]; o[7] = in[7]; o[8] = in[8];
    o[9] = word(dot3(B0.x, B0.y, B0.z, tx, ty, tz));
    o[10] = word(dot3(B1.x, B1.y, B1.z, tx, ty, tz));
    o[11] = word(dot3(B2.x, B2.y, B2.z, tx, ty, tz));
    o[12] = word(dot3(B0.x, B0.y, B0.z, bx, by, bz));
    o[13] = word(dot3(B1.x, B1.y, B1.z, bx, by, bz));
    o[14] = word(dot3(B2.x, B2.y, B2.z, bx, by, bz));
#pragma unroll
    for (int k = 0; k < kVertexWords; k++) d[k] = o[k];
}

template <bool DQ>
__global__ __launch_bounds__(kBlock) void deform_kernel(const DeformArgs a) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_vert) return;
    const unsigned *r = a.rest + kVertexWords * i;
    unsigned in[kVertexWords];
#pragma unroll
    for (int k = 0; k < kVertexWords; k++) in[k] = r[k];
    const uint4 b = a.rig[2 * i];
    const uint4 wu = a.rig[2 * i + 1];
    const float4 w = make_float4(__uint_as_float(wu.x), __uint_as_float(wu.y), __uint_as_float(wu.z), __uint_as_float(wu.w));

    // Morph: over the active targets in ascending index, a rounded product and a rounded sum a component
    float px = __uint_as_float(in[0]), py = __uint_as_float(in[1]), pz = __uint_as_float(in[2]);
    float nx = __uint_as_float(in[3]), ny = __uint_as_float(in[4]), nz = __uint_as_float(in[5]);
    for (int k = 0; k < a.morph.n_active; k++) {
        const float wk = a.morph.weight[k];
        const float2 *d = (a.deltas + 3 * (size_t)a.morph.index[k] * a.n_vert) + 3 * i;  // (the target's base is scalar)
        const float2 d0 = d[0], d1 = d[1], d2 = d[2];
        px = px + wk * d0.x; py = py + wk * d0.y; pz = pz + wk * d1.x;
        nx = nx + wk * d1.y; ny = ny + wk * d2.x; nz = nz + wk * d2.y;
    }

    float4 B0, B1, B2;
    if (DQ) {
        const float4 *q0 = a.pose + 2 * (size_t)b.x, *q1 = a.pose + 2 * (size_t)b.y, *q2 = a.pose + 2 * (size_t)b.z, *q3 = a.pose + 2 * (size_t)b.w;
        const float4 r0 = q0[0], r1 = q1[0], r2 = q2[0], r3 = q3[0];
        // Sign: a bone whose rotation lies in the other hemisphere from bone 0's enters with its weight negated (a NaN h keeps the weight)
        const float4 s = make_float4(w.x, dot4(r0, r1) < 0.0f ? -w.y : w.y, dot4(r0, r2) < 0.0f ? -w.z : w.z, dot4(r0, r3) < 0.0f ? -w.w : w.w);
        float4 R = blend_row(s, r0, r1, r2, r3);
        float4 D = blend_row(s, q0[1], q1[1], q2[1], q3[1]);
        // Normalise
        const float l = __builtin_sqrtf(dot4(R, R));
        const bool unit = l > 0.0f;
        R = quot4(R, l, unit);
        D = quot4(D, l, unit);
        // Rotation
        const float xx = R.x * R.x, yy = R.y * R.y, zz = R.z * R.z, xy = R.x * R.y, xz = R.x * R.z, yz = R.y * R.z, wx = R.w * R.x, wy = R.w * R.y, wz = R.w * R.z;
        B0.x = 1.0f - 2.0f * (yy + zz); B0.y = 2.0f * (xy - wz); B0.z = 2.0f * (xz + wy);
        B1.x = 2.0f * (xy + wz); B1.y = 1.0f - 2.0f * (xx + zz); B1.z = 2.0f * (yz - wx);
        B2.x = 2.0f * (xz - wy); B2.y = 2.0f * (yz + wx); B2.z = 1.0f - 2.0f * (xx + yy);
        // Translation
        B0.w = 2.0f * (((R.w * D.x - D.w * R.x) + R.y * D.z) - R.z * D.y);
        B1.w = 2.0f * (((R.w * D.y - D.w * R.y) + R.z * D.x) - R.x * D.z);
        B2.w = 2.0f * (((R.w * D.z - D.w * R.z) + R.x * D.y) - R.y * D.x);
    } else {
        const float4 *m0 = a.pose + 3 * (size_t)b.x, *m1 = a.pose + 3 * (size_t)b.y, *m2 = a.pose + 3 * (size_t)b.z, *m3 = a.pose + 3 * (size_t)b.w;
        B0 = blend_row(w, m0[0], m1[0], m2[0], m3[0]);
        B1 = blend_row(w, m0[1], m1[1], m2[1], m3[1]);
        B2 = blend_row(w, m0[2], m1[2], m2[2], m3[2]);
    }
    transform_store(B0, B1, B2, in, px, py, pz, nx, ny, nz, a.out + kVertexWords * i);
}

// ---- Sparse targets
constexpr int kMaxSparseTargets = 1024;  // GLRTX_MAX_SPARSE_MORPH_TARGETS

struct SparseArgs {
    const unsigned *rest;  // as Args
    const uint4 *rig;
    const float4 *pose;    // as DeformArgs
    unsigned *out;
    size_t n_vert;
    const unsigned *row;   // n_vert + 1: vertex i's entries are [row[i], row[i + 1])
    const float4 *entry;   // nnz x 2: {target (as bits), dpos.x, dpos.y, dpos.z} {dnormal.x, dnormal.y, dnormal.z, 0}, ascending by target inside a row
    const float *weight;   // n_targets: the pose's weights, +0 for an inactive target
    int n_targets;         // <= kMaxSparseTargets; every entry's target is below it (the host built the index)
};

template <bool DQ>
__global__ __launch_bounds__(kBlock) void deform_sparse_kernel(const SparseArgs a) {
    __shared__ float wt[kMaxSparseTargets];
    for (int k = threadIdx.x; k < a.n_targets; k += kBlock) wt[k] = a.weight[k];
    __syncthreads();  // every thread of the workgroup arrives: nothing returns above this line
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < a.n_vert) {
        const unsigned *r = a.rest + kVertexWords * i;
        unsigned in[kVertexWords];
#pragma unroll
        for (int k = 0; k < kVertexWords; k++) in[k] = r[k];
        const uint4 b = a.rig[2 * i];
        const uint4 wu = a.rig[2 * i + 1];
        const float4 w = make_float4(__uint_as_float(wu.x), __uint_as_float(wu.y), __uint_as_float(wu.z), __uint_as_float(wu.w));

        // Morph: the vertex's own entries in ascending target index, a rounded product and a rounded sum a component; an entry of an inactive target is skipped
        float px = __uint_as_float(in[0]), py = __uint_as_float(in[1]), pz = __uint_as_float(in[2]);
        float nx = __uint_as_float(in[3]), ny = __uint_as_float(in[4]), nz = __uint_as_float(in[5]);
        const unsigned e1 = a.row[i + 1];
        for (unsigned e = a.row[i]; e < e1; e++) {
            const float4 d0 = a.entry[2 * (size_t)e], d1 = a.entry[2 * (size_t)e + 1];
            const float wk = wt[__float_as_uint(d0.x)];
            if (wk != 0.0f) {
                px = px + wk * d0.y; py = py + wk * d0.z; pz = pz + wk * d0.w;
                nx = nx + wk * d1.x; ny = ny + wk * d1.y; nz = nz + wk * d1.z;
            }
        }

        float4 B0, B1, B2;
        if (DQ) {
            const float4 *q0 = a.pose + 2 * (size_t)b.x, *q1 = a.pose + 2 * (size_t)b.y, *q2 = a.pose + 2 * (size_t)b.z, *q3 = a.pose + 2 * (size_t)b.w;
            const float4 r0 = q0[0], r1 = q1[0], r2 = q2[0], r3 = q3[0];
            const float4 s = make_float4(w.x, dot4(r0, r1) < 0.0f ? -w.y : w.y, dot4(r0, r2) < 0.0f ? -w.z : w.z, dot4(r0, r3) < 0.0f ? -w.w : w.w);
            float4 R = blend_row(s, r0, r1, r2, r3);
            float4 D = blend_row(s, q0[1], q1[1], q2[1], q3[1]);
            const float l = __builtin_sqrtf(dot4(R, R));
            const bool unit = l > 0.0f;
            R = quot4(R, l, unit);
            D = quot4(D, l, unit);
            const float xx = R.x * R.x, yy = R.y * R.y, zz = R.z * R.z, xy = R.x * R.y, xz = R.x * R.z, yz = R.y * R.z, wx = R.w * R.x, wy = R.w * R.y, wz = R.w * R.z;
            B0.x = 1.0f - 2.0f * (yy + zz); B0.y = 2.0f * (xy - wz); B0.z = 2.0f * (xz + wy);
            B1.x = 2.0f * (xy + wz); B1.y = 1.0f - 2.0f * (xx + zz); B1.z = 2.0f * (yz - wx);
            B2.x = 2.0f * (xz - wy); B2.y = 2.0f * (yz + wx); B2.z = 1.0f - 2.0f * (xx + yy);
            B0.w = 2.0f * (((R.w * D.x - D.w * R.x) + R.y * D.z) - R.z * D.y);
            B1.w = 2.0f * (((R.w * D.y - D.w * R.y) + R.z * D.x) - R.x * D.z);
            B2.w = 2.0f * (((R.w * D.z - D.w * R.z) + R.x * D.y) - R.y * D.x);
        } else {
            const float4 *m0 = a.pose + 3 * (size_t)b.x, *m1 = a.pose + 3 * (size_t)b.y, *m2 = a.pose + 3 * (size_t)b.z, *m3 = a.pose + 3 * (size_t)b.w;
            B0 = blend_row(w, m0[0], m1[0], m2[0], m3[0]);
            B1 = blend_row(w, m0[1], m1[1], m2[1], m3[1]);
            B2 = blend_row(w, m0[2], m1[2], m2[2], m3[2]);
        }
        transform_store(B0, B1, B2, in, px, py, pz, nx, ny, nz, a.out + kVertexWords * i);
    }
}

}  // namespace skin
}  // namespace glrtx
