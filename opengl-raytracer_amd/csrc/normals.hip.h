// normals.hip.h -- rebuilding shading normals from the moved surface (glrtx_upload_normal_topology, glrtx_update_positions, glrtx_set_pose_normals,
// glrtx_debug_rebuild_normals; include/glrtx.h "Rebuilding normals").  The passes run on the context's vertex buffer between whatever wrote the positions -- the
// position-only update below, or a deform kernel of skin.hip.h -- and the refit (refit.hip.h), which reads the buffer exactly as it reads uploaded vertices.
//
// No reference counterpart.  The arithmetic is the header's text: host/normals.cpp (glrt_rebuild_normals) and tests/normals_math.py state it again, and all three
// agree bit for bit under denoise.hip.h's rules (one correctly rounded fp32 operation at a time in the order written, -ffp-contract=off; denormals flushed; a
// stored NaN is 0x7FC00000).  A store pass and a per-destination sum pass through an inverted index, no atomics: every class sums its own face list in a fixed
// order, so the result does not depend on how the lanes are scheduled.  All kernels: 256-thread workgroups, no LDS, no atomics, no scratch.
//
//   positions_kernel  one thread per vertex.  The 60-byte rest record as 15 dword loads (skin_kernel's note on alignment holds: a wave's 64 records are 3840
//       contiguous bytes), the three new position words as dword loads (a wave: 768 contiguous bytes), 15 dword stores.  132 bytes a vertex.  Words are moved as
//       integers: no float instruction touches them.
//   face_kernel       one thread per triangle.  The 16-byte topology record {i0, i1, i2, flip} as one 16-byte load, the three corners' positions as nine dword
//       loads (a gather: the corners of an unindexed mesh are neighbours, 3 x 60 bytes apart), the face vector {f.x, f.y, f.z, 0} as one 16-byte store, the
//       flip applied as an integer XOR of the sign bits.  68 bytes a triangle.
//   class_kernel      one thread per weld class.  row[c] and row[c + 1] (a wave: 260 contiguous bytes), then the class's list: a 4-byte face id and the 16-byte
//       face vector it names an entry, a lane-dependent trip count, summed in chunks of kChunk entries in list order (the chunk rule is the contract's: a later
//       kernel may give a long list's chunks to separate waves without changing a bit; this one walks every class on one lane).  The class's normal {n.x, n.y,
//       n.z, valid} as one 16-byte store; valid is 0 when l == 0 and the members keep their words.  4 + 16 bytes a class plus 20 an entry.
//   vertex_kernel     one thread per vertex.  The 4-byte class id, the class's 16-byte normal (a gather; the members of a class share it), three dword stores
//       into the normal words unless the class is not valid.  32 bytes a vertex.  Position words are only read, by face_kernel; normal words are only written, here.
//
// Compulsory bytes of a rebuild: 68 n_tri + 20 n_classes + 20 entries + 32 n_vert (entries: the sum of the face lists' lengths, at most 3 n_tri).
#pragma once
#include "denoise.hip.h"

namespace glrtx {
namespace normals {

constexpr int kBlock = 256;
constexpr int kVertexWords = 15;  // GLRT_VERTEX_FLOATS
constexpr unsigned kChunk = 256;  // GLRTX_NORMAL_CHUNK

struct Args {
    const uint4 *tri;      // n_tri: {i0, i1, i2, flip ? 0x80000000 : 0}; every index below n_vert (checked on the host before the upload)
    const unsigned *cls;   // n_vert: the class of a vertex, below n_classes
    const unsigned *row;   // n_classes + 1: class c's faces are face[row[c] .. row[c + 1])
    const unsigned *face;  // the face lists: triangle indices below n_tri, ascending inside a list
    unsigned *vert;        // n_vert x 15 words, in place: position words read, normal words written
    float4 *fvec;          // n_tri: the face vectors
    float4 *cnrm;          // n_classes: {n, valid}
    unsigned n_vert, n_tri, n_classes;
};

DEV unsigned word(float x) { return __float_as_uint(denoise::canon(x)); }

__global__ __launch_bounds__(kBlock) void positions_kernel(const unsigned *rest, const unsigned *pos, unsigned *out, unsigned n_vert) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_vert) return;
    const unsigned *r = rest + kVertexWords * i, *p = pos + 3 * i;
    unsigned o[kVertexWords];
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = p[k];
#pragma unroll
    for (int k = 3; k < kVertexWords; k++) o[k] = r[k];
    unsigned *d = out + kVertexWords * i;
#pragma unroll
    for (int k = 0; k < kVertexWords; k++) d[k] = o[k];
}

__global__ __launch_bounds__(kBlock) void face_kernel(const Args a) {
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= a.n_tri) return;
    const uint4 q = a.tri[t];
    const unsigned *v0 = a.vert + kVertexWords * (size_t)q.x, *v1 = a.vert + kVertexWords * (size_t)q.y, *v2 = a.vert + kVertexWords * (size_t)q.z;
    const float p0x = __uint_as_float(v0[0]), p0y = __uint_as_float(v0[1]), p0z = __uint_as_float(v0[2]);
    const float e1x = __uint_as_float(v1[0]) - p0x, e1y = __uint_as_float(v1[1]) - p0y, e1z = __uint_as_float(v1[2]) - p0z;
    const float e2x = __uint_as_float(v2[0]) - p0x, e2y = __uint_as_float(v2[1]) - p0y, e2z = __uint_as_float(v2[2]) - p0z;
    // Face vector: two rounded products and one subtraction a component; a flipped triangle's three sign bits are inverted
    const float fx = e1y * e2z - e1z * e2y, fy = e1z * e2x - e1x * e2z, fz = e1x * e2y - e1y * e2x;
    a.fvec[t] = make_float4(__uint_as_float(__float_as_uint(fx) ^ q.w), __uint_as_float(__float_as_uint(fy) ^ q.w), __uint_as_float(__float_as_uint(fz) ^ q.w), 0.0f);
}

__global__ __launch_bounds__(kBlock) void class_kernel(const Args a) {
    const size_t c = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= a.n_classes) return;
    const unsigned r0 = a.row[c], r1 = a.row[c + 1];
    // Sum: inside a chunk k = f_first, then k = k + f_next; across chunks s = k_0, then s = s + k_j
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (unsigned e0 = r0; e0 < r1; e0 += kChunk) {
        const unsigned e1 = r1 - e0 > kChunk ? e0 + kChunk : r1;
        const float4 f0 = a.fvec[a.face[e0]];
        float kx = f0.x, ky = f0.y, kz = f0.z;
        for (unsigned e = e0 + 1; e < e1; e++) {
            const float4 f = a.fvec[a.face[e]];
            kx = kx + f.x; ky = ky + f.y; kz = kz + f.z;
        }
        if (e0 == r0) { sx = kx; sy = ky; sz = kz; }
        else { sx = sx + kx; sy = sy + ky; sz = sz + kz; }
    }
    // Normal: l == 0 keeps the words in place (an empty list, a degenerate or cancelling neighbourhood); a NaN goes through as the canonical NaN
    const float l = __builtin_sqrtf((sz * sz + sy * sy) + sx * sx);
    a.cnrm[c] = make_float4(__uint_as_float(word(sx / l)), __uint_as_float(word(sy / l)), __uint_as_float(word(sz / l)), l == 0.0f ? 0.0f : 1.0f);
}

__global__ __launch_bounds__(kBlock) void vertex_kernel(const Args a) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n_vert) return;
    const float4 n = a.cnrm[a.cls[i]];
    if (n.w == 0.0f) return;
    unsigned *d = a.vert + kVertexWords * i + 3;
    d[0] = __float_as_uint(n.x); d[1] = __float_as_uint(n.y); d[2] = __float_as_uint(n.z);
}

}  // namespace normals
}  // namespace glrtx
