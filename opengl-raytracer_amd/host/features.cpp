// features.cpp -- glrt_render_features / glrt_render_features_geom (include/glrt_host.h): the CPU statement of the device's feature pass (glrtx_render_features, include/glrtx.h;
// csrc/features.hip.h), on the wire-format scene.
//
// Per owned pixel: the primary ray of the pixel's centre (the renderer's camera_ray with r0 = r1 = 0.5 and no thin lens, the same expressions in the same
// order, unfused), searched by glrt_trace_rays' walker (host/query.cpp) with tmin = 1e-4 and tmax = 1e8 -- what a primary ray of the renderer is given --,
// then the renderer's shading normal (surf_tri: barycentric mix of the vertex normals, IEEE sqrt, IEEE reciprocal) and the hit material's albedo.
// Compiled with -ffp-contract=off and run under MXCSR FTZ | DAZ, like host/query.cpp: the device's arithmetic, bit for bit.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "centre_ray.h"
#include "cutout_statement.h"
#include "glrt_host.h"
#include "statement_math.h"
#include "texture_statement.h"

namespace {

using glrt_detail::centre_ray;
using glrt_detail::rsq;

using glrt_detail::canon;
using glrt_detail::dot3;
using glrt_detail::FlushDenormals;

// the pass; out_g (may be NULL): the geometry plane {wire triangle as int32 bits, u, v, 0} of glrt_render_features_geom.  hook (may be NULL): the cutout rule
// inside the search, and material_texture (with it): plane A's looked-up albedo of a bound diffuse material (glrt_render_features_geom_cutout)
int render_planes(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                  const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, float *out_n, float *out_a, float *out_g,
                  const glrt_detail::CutoutHook *hook = nullptr, const int32_t *material_texture = nullptr) {
    if (!c2w || !s2c || !out_n || !out_a) return GLRT_HOST_EINVAL;
    if (width < 1 || height < 1 || width > 65536 || height > 65536 || world < 1 || rank < 0 || rank >= world || stripe < 1) return GLRT_HOST_EINVAL;
    if (n_nodes > 0 && (!vert || !tri || !nodes || !mat)) return GLRT_HOST_EINVAL;
    for (size_t t = 0; t < n_tri; t++) {
        const float m = tri[4 * t + 3];
        if (!(m >= 0.0f) || (size_t)m >= n_mat) return GLRT_HOST_EINDEX;
    }
    // the owned rows, in the device's order: stripe s of the image belongs to rank s % world (glrtx_local_row_to_y)
    std::vector<int> rows;
    for (int y = 0; y < height; y++)
        if ((y / stripe) % world == rank) rows.push_back(y);
    if (rows.empty()) return GLRT_HOST_OK;
    FlushDenormals ftz;
    const size_t n = rows.size() * (size_t)width;
    std::vector<float> rays(8 * n), hits(4 * n);
    for (size_t r = 0; r < rows.size(); r++)
        for (int x = 0; x < width; x++) centre_ray(c2w, s2c, (float)width, (float)height, x, rows[r], &rays[8 * (r * width + x)]);
    if (const int rc = glrt_detail::trace_rays_cutout(vert, n_vert, tri, n_tri, nodes, n_nodes, rays.data(), n, hits.data(), GLRT_TRACE_CLOSEST, hook)) return rc;
    for (size_t i = 0; i < n; i++) {
        const float *h = &hits[4 * i];
        float *N = out_n + 4 * i, *A = out_a + 4 * i;
        int32_t t;
        std::memcpy(&t, &h[1], 4);
        int32_t id = -1;
        N[0] = N[1] = N[2] = N[3] = 0.0f;
        A[0] = A[1] = A[2] = 1.0f;
        if (t >= 0) {
            const float *tr = tri + 4 * (size_t)t;
            const float *n0 = vert + GLRT_VERTEX_FLOATS * (size_t)tr[0] + 3, *n1 = vert + GLRT_VERTEX_FLOATS * (size_t)tr[1] + 3,
                        *n2 = vert + GLRT_VERTEX_FLOATS * (size_t)tr[2] + 3;
            const float u = h[2], v = h[3];
            const float w0 = (1.0f - u) - v;
            const float tx = (w0 * n0[0] + u * n1[0]) + v * n2[0];
            const float ty = (w0 * n0[1] + u * n1[1]) + v * n2[1];
            const float tz = (w0 * n0[2] + u * n1[2]) + v * n2[2];
            const float r = rsq(dot3(tx, ty, tz, tx, ty, tz));
            N[0] = canon(tx * r); N[1] = canon(ty * r); N[2] = canon(tz * r); N[3] = h[0];
            id = (int32_t)tr[3];
            const float *m = mat + GLRT_MATERIAL_FLOATS * (size_t)id;
            if ((int)m[0] == 2) { A[0] = m[6]; A[1] = m[7]; A[2] = m[8]; }  // a diffuse material: param0
            if (hook && material_texture && (int)m[0] == 2 && material_texture[id] >= 0) {  // ... or the bound texture's lookup at the hit ("Textures": AT A HIT)
                const float *a = vert + GLRT_VERTEX_FLOATS * (size_t)tr[0] + 6, *b = vert + GLRT_VERTEX_FLOATS * (size_t)tr[1] + 6,
                            *c = vert + GLRT_VERTEX_FLOATS * (size_t)tr[2] + 6;
                glrt_detail::texture_lookup_one(hook->tex[material_texture[id]], hook->texels, (w0 * a[0] + u * b[0]) + v * c[0], (w0 * a[1] + u * b[1]) + v * c[1], A);
            }
        }
        std::memcpy(&A[3], &id, 4);
        if (out_g) {  // the walker's own {tri, u, v}; a miss {-1, 0, 0, 0}
            float *G = out_g + 4 * i;
            const int32_t miss = -1;
            std::memcpy(&G[0], t >= 0 ? &t : &miss, 4);
            G[1] = t >= 0 ? h[2] : 0.0f; G[2] = t >= 0 ? h[3] : 0.0f; G[3] = 0.0f;
        }
    }
    return GLRT_HOST_OK;
}

}  // namespace

int glrt_render_features(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                         const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, float *out_n, float *out_a) {
    return render_planes(vert, n_vert, tri, n_tri, nodes, n_nodes, mat, n_mat, c2w, s2c, width, height, rank, world, stripe, out_n, out_a, nullptr);
}

int glrt_render_features_geom(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                              const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, float *out_n, float *out_a, float *out_g) {
    if (!out_g) return GLRT_HOST_EINVAL;
    return render_planes(vert, n_vert, tri, n_tri, nodes, n_nodes, mat, n_mat, c2w, s2c, width, height, rank, world, stripe, out_n, out_a, out_g);
}

int glrt_render_features_geom_cutout(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                                     const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, const glrt_texture *tex, size_t n_tex,
                                     const void *texels, size_t texel_bytes, const int32_t *material_texture, const glrt_cutout *cut, float *out_n, float *out_a,
                                     float *out_g) {
    if (!out_g || (n_mat && (!cut || !material_texture || !mat))) return GLRT_HOST_EINVAL;
    const glrt_detail::TexRecord *rec = reinterpret_cast<const glrt_detail::TexRecord *>(tex);
    if (!glrt_detail::texture_set_error(rec, n_tex, texels, texel_bytes).empty()) return GLRT_HOST_EINVAL;
    for (size_t m = 0; m < n_mat; m++) {  // what glrtx_upload_textures and glrtx_bind_cutouts refuse
        const int type = (int)mat[GLRT_MATERIAL_FLOATS * m];
        if (material_texture[m] < -1 || (material_texture[m] >= 0 && ((size_t)material_texture[m] >= n_tex || type != 2))) return GLRT_HOST_EINDEX;
        const glrt_cutout &r = cut[m];
        if (r.texture < -1 || (r.texture >= 0 && (size_t)r.texture >= n_tex) || r.channel < 0 || r.channel > 3) return GLRT_HOST_EINDEX;
        if (!std::isfinite(r.cutoff) || r.reserved != 0 || (r.texture >= 0 && type != 2 && type != 3)) return GLRT_HOST_EINVAL;
    }
    const glrt_detail::CutoutHook hook{rec, (const unsigned char *)texels, cut};
    return render_planes(vert, n_vert, tri, n_tri, nodes, n_nodes, mat, n_mat, c2w, s2c, width, height, rank, world, stripe, out_n, out_a, out_g, &hook, material_texture);
}
