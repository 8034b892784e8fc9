// normals.cpp -- glrt_normal_topology, glrt_rebuild_normals, glrt_positions_to_vertices (include/glrt_host.h): the CPU statement of the device's normal
// rebuild (glrtx_update_positions, glrtx_set_pose_normals, glrtx_debug_rebuild_normals, include/glrtx.h "Rebuilding normals"; csrc/normals.hip.h).  The contract is
// the text in include/glrtx.h; tests/normals_math.py restates it in numpy.  Every fp32 operation of the statement is one correctly rounded IEEE operation in the
// order written (-ffp-contract=off), under MXCSR FTZ | DAZ.  The topology's pieces are host/normal_topology.h's, which the device library compiles too.
#include <cmath>
#include <cstring>

#include <vector>

#include "glrt_host.h"
#include "normal_topology.h"
#include "statement_math.h"

using namespace glrt_detail;

static_assert(kNormalsWeldPositions == GLRT_NORMALS_WELD_POSITIONS && kNormalChunk == GLRT_NORMAL_CHUNK && kVertexFloats == GLRT_VERTEX_FLOATS,
              "host/normal_topology.h and glrt_host.h disagree");

int glrt_normal_topology(const float *rest_vert, size_t n_vert, const float *tri, size_t n_tri, unsigned flags, uint32_t *class_of_vertex_out,
                         uint8_t *flip_out, size_t *n_classes_out) {
    NormalFault f;
    if ((n_vert > 0 && (!rest_vert || !class_of_vertex_out)) || (n_tri > 0 && !flip_out)) return GLRT_HOST_EINVAL;
    if (flags & ~kNormalsWeldPositions) return GLRT_HOST_EINVAL;
    if (!normal_mesh_check(tri, n_tri, n_vert, f)) return GLRT_HOST_EINVAL;
    const size_t n_classes = normal_weld(rest_vert, n_vert, flags, class_of_vertex_out);
    normal_flips(rest_vert, tri, n_tri, flip_out);
    if (n_classes_out) *n_classes_out = n_classes;
    return GLRT_HOST_OK;
}

int glrt_rebuild_normals(float *vert_inout, size_t n_vert, const float *tri, size_t n_tri, const uint32_t *class_of_vertex, const uint8_t *flip) {
    NormalFault fault;
    if ((n_vert > 0 && (!vert_inout || !class_of_vertex)) || (n_tri > 0 && !flip)) return GLRT_HOST_EINVAL;
    if (!normal_mesh_check(tri, n_tri, n_vert, fault) || !normal_class_check(class_of_vertex, n_vert, fault)) return GLRT_HOST_EINVAL;
    std::vector<uint64_t> row;
    std::vector<uint32_t> face;
    normal_face_lists(tri, n_tri, class_of_vertex, n_vert, row, face);
    FlushDenormals ftz;
    // Face vectors, the flip applied: the three sign bits inverted
    std::vector<float> fv(3 * n_tri);
    for (size_t t = 0; t < n_tri; t++) {
        float *f = &fv[3 * t];
        face_vector(vert_inout + kVertexFloats * (size_t)tri[4 * t], vert_inout + kVertexFloats * (size_t)tri[4 * t + 1],
                    vert_inout + kVertexFloats * (size_t)tri[4 * t + 2], f);
        if (flip[t])
            for (int r = 0; r < 3; r++) f[r] = bits_f(bits(f[r]) ^ 0x80000000u);
    }
    // Sum of a class in chunks of kNormalChunk entries, then its normal; `keep`: l == 0, the members keep their words
    const size_t n_rows = row.size() - 1;
    std::vector<float> cn(3 * n_rows);
    std::vector<uint8_t> keep(n_rows);
    for (size_t c = 0; c < n_rows; c++) {
        float s[3] = {0.0f, 0.0f, 0.0f};
        for (uint64_t e0 = row[c]; e0 < row[c + 1]; e0 += kNormalChunk) {
            const uint64_t e1 = e0 + kNormalChunk < row[c + 1] ? e0 + kNormalChunk : row[c + 1];
            float k[3];
            std::memcpy(k, &fv[3 * (size_t)face[e0]], sizeof k);
            for (uint64_t e = e0 + 1; e < e1; e++)
                for (int r = 0; r < 3; r++) k[r] = k[r] + fv[3 * (size_t)face[e] + r];
            for (int r = 0; r < 3; r++) s[r] = e0 == row[c] ? k[r] : s[r] + k[r];
        }
        const float l = std::sqrt(dot3(s[0], s[1], s[2], s[0], s[1], s[2]));
        keep[c] = l == 0.0f;
        for (int r = 0; r < 3; r++) cn[3 * c + r] = canon(s[r] / l);
    }
    for (size_t i = 0; i < n_vert; i++) {
        const size_t c = class_of_vertex[i];
        if (!keep[c]) std::memcpy(vert_inout + kVertexFloats * i + 3, &cn[3 * c], 3 * sizeof(float));
    }
    return GLRT_HOST_OK;
}

int glrt_positions_to_vertices(const float *rest_vert, const float *pos, size_t n_vert, float *vert_out) {
    if (n_vert > 0 && (!rest_vert || !pos || !vert_out)) return GLRT_HOST_EINVAL;
    for (size_t i = 0; i < n_vert; i++) {
        std::memcpy(vert_out + kVertexFloats * i, rest_vert + kVertexFloats * i, kVertexFloats * sizeof(float));  // (words: nothing is converted)
        std::memcpy(vert_out + kVertexFloats * i, pos + 3 * i, 3 * sizeof(float));
    }
    return GLRT_HOST_OK;
}
