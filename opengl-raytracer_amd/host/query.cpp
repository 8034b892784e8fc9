// query.cpp -- glrt_trace_rays (include/glrt_host.h): the CPU statement of the device's ray queries (glrtx_trace_rays, include/glrtx.h;
// csrc/query.hip.h), on the wire-format tree.
//
// The traversal and the triangle test are those of the renderer's CPU statement (the checker's pt_traverse / pt_tri, after raytrace.frag :276-335 and
// :226-257): depth first from node 0, a fork's own box tested when the fork is taken from the stack, children.x pushed before children.y (so children.y
// is visited first), leaves never box-tested.  The query's changes: the search limit starts at tmax (so tmax also culls boxes), a hit needs t > tmin
// instead of t > EPS, and in any-hit mode the first accepted hit ends the search.  The device visits the same triangles in the same order and applies
// the same IEEE operations, so the two agree bit for bit:
//   - compiled with -ffp-contract=off (Makefile): no fused multiply-adds;
//   - IEEE quotients: the device's 1 / x forms equal them wherever they matter (pt_kernel.hip.h: frcp, rcp_newton), except that rcp_newton gives NaN for
//     an infinite det where 1 / det is 0; that one case is written out below;
//   - denormals flushed: the call runs with MXCSR FTZ | DAZ, as the device's arithmetic does (restored on return), and the ray's components are read as
//     the device reads them (denormals as zeros of their sign).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "cutout_statement.h"
#include "glrt_host.h"
#include "statement_math.h"
#include "texture_statement.h"

namespace {

constexpr float kEps = 1.0e-4f;  // the renderer's |det| rejection (PT_EPS)

// GLSL min / max as the renderer lowers them: the other operand when one is NaN
inline float fmin_g(float a, float b) { return (b != b) ? a : (a < b ? a : b); }
inline float fmax_g(float a, float b) { return (b != b) ? a : (a > b ? a : b); }
using glrt_detail::bits;
using glrt_detail::bits_f;
using glrt_detail::dot3;
using glrt_detail::FlushDenormals;

inline float flush(float x) { const uint32_t b = bits(x); return (b & 0x7F800000u) == 0u ? bits_f(b & 0x80000000u) : x; }
inline bool finite(float x) { return (bits(x) & 0x7F800000u) != 0x7F800000u; }

struct Tree {
    const float *vert, *tri, *nodes;
    const glrt_detail::CutoutHook *cut;  // glrt_render_features_geom_cutout's search alone (include/glrtx.h "Cutouts"); null: the geometric query
};

// The cutout rule at a candidate (u, v) of wire triangle tr with corners v0, v1, v2: accepted iff the channel's value >= cutoff (a NaN rejects)
bool cut_accepts(const glrt_detail::CutoutHook &h, const float *tr, const float *v0, const float *v1, const float *v2, float u, float v) {
    const glrt_cutout &r = h.cut[(size_t)tr[3]];
    if (r.texture < 0) return true;
    const float w0 = (1.0f - u) - v;
    const float s = (w0 * v0[6] + u * v1[6]) + v * v2[6];
    const float t = (w0 * v0[7] + u * v1[7]) + v * v2[7];
    return glrt_detail::texture_channel_one(h.tex[r.texture], h.texels, r.channel, s, t) >= r.cutoff;
}

// One ray.  hit: {t, tri (int32 bits), u, v}.
void trace_one(const Tree &s, const float *r, float *hit, bool any, std::vector<int> &stack) {
    float o[3], d[3], tmin, tmax;
    for (int k = 0; k < 3; k++) { o[k] = flush(r[k]); d[k] = flush(r[4 + k]); }
    tmin = flush(r[3]);
    tmax = flush(r[7]);
    float tHit = tmax, hu = 0.0f, hv = 0.0f;
    int htri = -1;
    bool fin = finite(tmin) && finite(tmax);
    for (int k = 0; k < 3; k++) fin = fin && finite(o[k]) && finite(d[k]);
    const bool dir = ((bits(d[0]) | bits(d[1]) | bits(d[2])) & 0x7FFFFFFFu) != 0u;
    if (fin && dir && tmin < tmax && s.nodes) {
        const float ix = 1.0f / d[0], iy = 1.0f / d[1], iz = 1.0f / d[2];
        stack.clear();
        stack.push_back(0);
        while (!stack.empty()) {
            const int node = stack.back();
            stack.pop_back();
            const float *nd = s.nodes + 9 * (size_t)node;
            if (nd[8] < 0.0f) {  // fork: its own box, then the children
                const float fx = (nd[3] - o[0]) * ix, fy = (nd[4] - o[1]) * iy, fz = (nd[5] - o[2]) * iz;
                const float nx = (nd[0] - o[0]) * ix, ny = (nd[1] - o[1]) * iy, nz = (nd[2] - o[2]) * iz;
                const float t1 = fmin_g(fmax_g(fx, nx), fmin_g(fmax_g(fy, ny), fmax_g(fz, nz)));
                const float t0 = fmax_g(fmin_g(fx, nx), fmax_g(fmin_g(fy, ny), fmin_g(fz, nz)));
                if (fmin_g(t1, tHit) >= t0) {  // (t1 >= t0 && t0 <= tHit) evaluated as min(t1, tHit) >= t0
                    if (nd[6] >= 0.0f) stack.push_back((int)nd[6]);
                    if (nd[7] >= 0.0f) stack.push_back((int)nd[7]);
                }
                continue;
            }
            const int t = (int)nd[8];
            const float *tr = s.tri + 4 * (size_t)t;
            const float *v0 = s.vert + GLRT_VERTEX_FLOATS * (size_t)tr[0], *v1 = s.vert + GLRT_VERTEX_FLOATS * (size_t)tr[1],
                        *v2 = s.vert + GLRT_VERTEX_FLOATS * (size_t)tr[2];
            const float e1x = v1[0] - v0[0], e1y = v1[1] - v0[1], e1z = v1[2] - v0[2];
            const float e2x = v2[0] - v0[0], e2y = v2[1] - v0[1], e2z = v2[2] - v0[2];
            const float px = d[1] * e2z - d[2] * e2y;
            const float py = d[2] * e2x - d[0] * e2z;
            const float pz = d[0] * e2y - d[1] * e2x;
            const float det = dot3(e1x, e1y, e1z, px, py, pz);
            if (-kEps < det && det < kEps) continue;
            const float inv = std::isinf(det) ? std::numeric_limits<float>::quiet_NaN() : 1.0f / det;
            const float tx = o[0] - v0[0], ty = o[1] - v0[1], tz = o[2] - v0[2];
            const float U = dot3(tx, ty, tz, px, py, pz);
            const float u = U * inv;
            if (u < 0.0f || 1.0f < u) continue;
            const float qx = ty * e1z - tz * e1y;
            const float qy = tz * e1x - tx * e1z;
            const float qz = tx * e1y - ty * e1x;
            const float V = dot3(d[0], d[1], d[2], qx, qy, qz);
            const float v = V * inv;
            if (v < 0.0f || 1.0f < inv * (U + V)) continue;  // u + v > 1 evaluated as inv * (U + V) > 1
            const float tt = dot3(e2x, e2y, e2z, qx, qy, qz) * inv;
            if (tmin >= tt || !(tt < tHit)) continue;  // strict: among equal distances the first one visited wins; a NaN t is never a hit
            if (s.cut && !cut_accepts(*s.cut, tr, v0, v1, v2, u, v)) continue;  // a rejected candidate changes nothing
            tHit = tt; htri = t; hu = u; hv = v;
            if (any) break;
        }
    }
    hit[0] = tHit;
    std::memcpy(&hit[1], &htri, 4);
    hit[2] = hu;
    hit[3] = hv;
}

}  // namespace

int glrt_trace_rays(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *rays, size_t n,
                    float *hits_out, int flags) {
    return glrt_detail::trace_rays_cutout(vert, n_vert, tri, n_tri, nodes, n_nodes, rays, n, hits_out, flags, nullptr);
}

int glrt_detail::trace_rays_cutout(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *rays, size_t n,
                                   float *hits_out, int flags, const CutoutHook *hook) {
    if (flags != GLRT_TRACE_CLOSEST && flags != GLRT_TRACE_ANY) return GLRT_HOST_EINVAL;
    if (n == 0) return GLRT_HOST_OK;
    if (!rays || !hits_out) return GLRT_HOST_EINVAL;
    if (n_nodes > 0 && (!vert || !tri || !nodes)) return GLRT_HOST_EINVAL;
    // The tree reachable from node 0 must be a tree over valid triangles (the checks of glrt_bvh_refit): every node reached once, children and leaf
    // triangles in range, vertex indices in range.
    if (n_nodes > 0) {
        std::vector<char> seen(n_nodes, 0);
        std::vector<size_t> st{0};
        while (!st.empty()) {
            const size_t nd = st.back();
            st.pop_back();
            if (seen[nd]) return GLRT_HOST_EINVAL;
            seen[nd] = 1;
            const float *c = nodes + 9 * nd + 6;
            if (c[2] < 0.0f) {
                for (int k = 0; k < 2; k++) {
                    if (!(c[k] >= 0.0f)) continue;
                    if ((size_t)c[k] >= n_nodes) return GLRT_HOST_EINVAL;
                    st.push_back((size_t)c[k]);
                }
            } else {
                if (!(c[2] >= 0.0f) || (size_t)c[2] >= n_tri) return GLRT_HOST_EINVAL;
                const float *tr = tri + 4 * (size_t)c[2];
                for (int k = 0; k < 3; k++)
                    if (!(tr[k] >= 0.0f) || (size_t)tr[k] >= n_vert) return GLRT_HOST_EINDEX;
            }
        }
    }
    FlushDenormals ftz;
    const Tree s{vert, tri, n_nodes > 0 ? nodes : nullptr, hook};
    std::vector<int> stack;
    stack.reserve(64);
    for (size_t i = 0; i < n; i++) trace_one(s, rays + 8 * i, hits_out + 4 * i, flags == GLRT_TRACE_ANY, stack);
    return GLRT_HOST_OK;
}
