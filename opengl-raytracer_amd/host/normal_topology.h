// normal_topology.h -- what glrt_normal_topology / glrt_rebuild_normals (host/normals.cpp) and the device library (csrc/glrtx.hip: glrtx_upload_normal_topology,
// glrtx_debug_rebuild_normals) share about rebuilding normals (include/glrtx.h "Rebuilding normals"): the checks that decide what is refused, the weld classes,
// the orientation bits and the classes' face lists.  Plain C++, no dependency on either library; both compile it with -ffp-contract=off.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include <unordered_map>
#include <vector>

#include "statement_math.h"

namespace glrt_detail {

constexpr unsigned kNormalsWeldPositions = 1u;  // GLRT_NORMALS_WELD_POSITIONS, GLRTX_NORMALS_WELD_POSITIONS
constexpr unsigned kNormalChunk = 256u;         // GLRT_NORMAL_CHUNK, GLRTX_NORMAL_CHUNK
constexpr int kVertexFloats = 15;               // GLRT_VERTEX_FLOATS

// Why a mesh is refused: the kind, and the triangle / corner or the vertex where it shows
struct NormalFault {
    enum Kind { kNone, kNull, kTooMany, kFlags, kCorner, kClass } kind = kNone;
    size_t at = 0;
    int corner = 0;
    double value = 0.0;
};

inline void normal_fault_message(const NormalFault &f, size_t n_vert, char *buf, size_t n) {
    switch (f.kind) {
        case NormalFault::kNone: std::snprintf(buf, n, "no fault"); break;
        case NormalFault::kNull: std::snprintf(buf, n, "NULL buffer"); break;
        case NormalFault::kTooMany: std::snprintf(buf, n, "%zu triangles or vertices (at most 2^31 - 1)", f.at); break;
        case NormalFault::kFlags: std::snprintf(buf, n, "unknown flag bits 0x%zx", f.at); break;
        case NormalFault::kCorner: std::snprintf(buf, n, "triangle %zu, corner %d: vertex index %g of %zu", f.at, f.corner, f.value, n_vert); break;
        case NormalFault::kClass: std::snprintf(buf, n, "vertex %zu: class id %.0f of at most %zu", f.at, f.value, n_vert); break;
    }
}

// Every corner of the n_tri wire triangles {i0, i1, i2, material} is an integer within [0, n_vert); n_tri and n_vert below 2^31
inline bool normal_mesh_check(const float *tri, size_t n_tri, size_t n_vert, NormalFault &f) {
    f = NormalFault{};
    if (n_tri >= ((size_t)1 << 31)) { f.kind = NormalFault::kTooMany; f.at = n_tri; return false; }
    if (n_vert >= ((size_t)1 << 31)) { f.kind = NormalFault::kTooMany; f.at = n_vert; return false; }
    if (n_tri > 0 && !tri) { f.kind = NormalFault::kNull; return false; }
    for (size_t t = 0; t < n_tri; t++)
        for (int k = 0; k < 3; k++) {
            const double v = tri[4 * t + k];
            if (!(v >= 0.0 && v < (double)n_vert && v == (double)(uint32_t)v)) { f.kind = NormalFault::kCorner; f.at = t; f.corner = k; f.value = v; return false; }
        }
    return true;
}

inline bool normal_class_check(const uint32_t *class_of_vertex, size_t n_vert, NormalFault &f) {
    for (size_t i = 0; i < n_vert; i++)
        if (class_of_vertex[i] >= n_vert) { f.kind = NormalFault::kClass; f.at = i; f.value = class_of_vertex[i]; return false; }
    return true;
}

// Face vector: e1 = p1 - p0, e2 = p2 - p0, f = e1 x e2 -- two rounded products and one subtraction a component.  The caller runs under FlushDenormals.
inline void face_vector(const float *p0, const float *p1, const float *p2, float f[3]) {
    const float e1x = p1[0] - p0[0], e1y = p1[1] - p0[1], e1z = p1[2] - p0[2];
    const float e2x = p2[0] - p0[0], e2y = p2[1] - p0[1], e2z = p2[2] - p0[2];
    f[0] = e1y * e2z - e1z * e2y;
    f[1] = e1z * e2x - e1x * e2z;
    f[2] = e1x * e2y - e1y * e2x;
}

// Weld classes: vertices whose rest position and rest normal (flags & kNormalsWeldPositions: position alone) are the same 32-bit patterns.  Ids ascend with each
// class's smallest member.  Returns the number of classes.
inline size_t normal_weld(const float *rest_vert, size_t n_vert, unsigned flags, uint32_t *class_of_vertex) {
    struct Key {
        uint32_t w[6];
        bool operator==(const Key &o) const { return std::memcmp(w, o.w, sizeof w) == 0; }
    };
    struct Hash {
        size_t operator()(const Key &k) const {
            uint64_t h = 0xcbf29ce484222325ull;
            for (uint32_t x : k.w) h = (h ^ x) * 0x100000001b3ull;
            return (size_t)(h ^ (h >> 29));
        }
    };
    const int words = (flags & kNormalsWeldPositions) ? 3 : 6;
    std::unordered_map<Key, uint32_t, Hash> seen;
    seen.reserve(n_vert);
    for (size_t i = 0; i < n_vert; i++) {
        Key k{};
        std::memcpy(k.w, rest_vert + kVertexFloats * i, (size_t)words * sizeof(uint32_t));
        class_of_vertex[i] = seen.emplace(k, (uint32_t)seen.size()).first->second;
    }
    return seen.size();
}

// Orientation: triangle t is flipped iff dot(f, m) < 0 in the rest pose, m = (n0 + n1) + n2 over its corners' rest normals.  A NaN or a zero does not flip.
inline void normal_flips(const float *rest_vert, const float *tri, size_t n_tri, uint8_t *flip) {
    FlushDenormals ftz;
    for (size_t t = 0; t < n_tri; t++) {
        const float *v0 = rest_vert + kVertexFloats * (size_t)tri[4 * t], *v1 = rest_vert + kVertexFloats * (size_t)tri[4 * t + 1],
                    *v2 = rest_vert + kVertexFloats * (size_t)tri[4 * t + 2];
        float f[3];
        face_vector(v0, v1, v2, f);
        const float mx = (v0[3] + v1[3]) + v2[3], my = (v0[4] + v1[4]) + v2[4], mz = (v0[5] + v1[5]) + v2[5];
        flip[t] = dot3(f[0], f[1], f[2], mx, my, mz) < 0.0f ? 1 : 0;
    }
}

// The classes' face lists as rows: class c's triangles are face[row[c] .. row[c + 1]), each triangle with a corner in the class once, ascending.  n_rows is
// 1 + the largest class id (0 without vertices); a class id no vertex carries has an empty row.
inline void normal_face_lists(const float *tri, size_t n_tri, const uint32_t *class_of_vertex, size_t n_vert, std::vector<uint64_t> &row, std::vector<uint32_t> &face) {
    size_t n_rows = 0;
    for (size_t i = 0; i < n_vert; i++)
        if ((size_t)class_of_vertex[i] + 1 > n_rows) n_rows = (size_t)class_of_vertex[i] + 1;
    row.assign(n_rows + 1, 0);
    const auto corners = [&](size_t t, uint32_t c[3]) {  // the distinct classes of triangle t's corners
        int n = 0;
        for (int k = 0; k < 3; k++) {
            const uint32_t ck = class_of_vertex[(size_t)tri[4 * t + k]];
            bool dup = false;
            for (int j = 0; j < n; j++) dup = dup || c[j] == ck;
            if (!dup) c[n++] = ck;
        }
        return n;
    };
    uint32_t c[3];
    for (size_t t = 0; t < n_tri; t++)
        for (int k = corners(t, c); k-- > 0;) row[(size_t)c[k] + 1]++;
    for (size_t r = 0; r < n_rows; r++) row[r + 1] += row[r];
    face.resize((size_t)row[n_rows]);
    std::vector<uint64_t> at(row.begin(), row.end() - 1);
    for (size_t t = 0; t < n_tri; t++)
        for (int k = corners(t, c); k-- > 0;) face[(size_t)at[c[k]]++] = (uint32_t)t;
}

}  // namespace glrt_detail
