// reproject_motion.hip.h -- reprojection across a geometry move (glrtx_reproject_motion / glrtx_debug_reproject_motion, include/glrtx.h "Reprojection across a
// geometry move"): reproject.hip.h's pass with SVGF's motion vector.  The surface point of a pixel of the new view is named by the geometry plane G1
// {wire triangle, u, v} (features.hip.h); topology is fixed across glrtx_update_vertices, so the same (triangle, u, v) on the PREVIOUS vertices is where that
// material point was when the old view was rendered: P = (p0 + u e1) + v e2, looked up in the old view exactly as reproject_kernel looks its P up.  The normal
// test uses the previous normal at that point (surf_tri on the previous vertex normals): what the old view should have seen there.
//
// No reference counterpart.  The arithmetic is the header's text: host/reproject_motion.cpp (glrt_reproject_motion) and tests/reproject_motion_math.py state it
// again, and all three agree bit for bit.
//
// reproject_kernel's shape: a wave is one 8x8 tile, a workgroup four consecutive tiles; A1 and G1 are read once with non-temporal 16-byte loads (N1 is not
// read); the previous triangle's six float4 are plain 16-byte loads -- the lanes of a tile lie on the same or neighbouring triangles, so most of them are L1
// hits --; the four taps, the store and the 64 counter slots are reproject_kernel's: reproject.hip.h's history_lookup, store_pixel and count_wave, called with the
// previous point and the previous normal.  No LDS, no scratch.
//
// The previous geometry: two arrays indexed by WIRE triangle, three float4 each -- {p0} {p1 - p0} {p2 - p0} (the leaf record's own words: pack_scene's
// edges, denormals kept) and {n0} {n1} {n2}.  snapshot_kernel copies them out of the scene's leaf records before the first refit after a feature pass.
#pragma once
#include "reproject.hip.h"

namespace glrtx {
namespace motion {

using reproject::pos_finite;  // (no longer called here: history_lookup applies it; tests/test_reproject_motion_abi.py's source check still names the line)

struct Args {
    reproject::Common c;      // (x1: G1)
    const float4 *prev_pos;   // 3 per wire triangle: {p0} {e1} {e2}
    const float4 *prev_nrm;   // 3 per wire triangle: the vertex normals
    int n_tri;                // triangles the two arrays hold
};

__global__ __launch_bounds__(256) void reproject_motion_kernel(const Args a) {
    const reproject::Pixel px = reproject::pixel_of(a.c);
    bool hit = false, carried = false;
    float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f), m4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (px.in) {
        const size_t p = (size_t)px.y * a.c.width + px.x;
        const float4 G1 = ld_stream(a.c.x1 + p), A1 = ld_stream(a.c.a1 + p);
        const int id = __float_as_int(A1.w);
        hit = id >= 0;  // (the reserved id INT32_MIN is negative)
        const unsigned tri = __float_as_uint(G1.x);
        if (hit && tri < (unsigned)a.n_tri) {  // (a negative index is a large unsigned one)
            const float4 p0 = a.prev_pos[3 * (size_t)tri], e1 = a.prev_pos[3 * (size_t)tri + 1], e2 = a.prev_pos[3 * (size_t)tri + 2];
            const float u = G1.y, v = G1.z;
            const float Px = (p0.x + u * e1.x) + v * e2.x, Py = (p0.y + u * e1.y) + v * e2.y, Pz = (p0.z + u * e1.z) + v * e2.z;
            DevScene prev{};  // surf_tri reads the normals alone
            prev.nrms = a.prev_nrm;
            Hit h;
            h.t = 0.f; h.tri = (int)tri; h.u = u; h.v = v;
            const Surf M = surf_tri(prev, h);
            reproject::history_lookup(a.c, Px, Py, Pz, M.nx, M.ny, M.nz, id, o4, m4, carried);
        }
        reproject::store_pixel(a.c, px, o4, m4);
    }
    reproject::count_wave(a.c, carried, hit);
}

// The previous geometry out of the scene's leaf records: one thread per leaf record k (id k + 1, at node record n_ids - 1 - id; its normals at 3 id), to the
// wire triangle the ray queries' table names for it.  Words are moved as integers: nothing is flushed.
struct SnapArgs {
    const uint4 *nodes, *nrms;
    const int *wire;        // id -> wire triangle (id 0: -1)
    int n_ids, n_leaf, n_tri;
    uint4 *prev_pos, *prev_nrm;
};

__global__ __launch_bounds__(256) void snapshot_kernel(const SnapArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n_leaf) return;
    const int id = i + 1;
    const unsigned w = (unsigned)a.wire[id];
    if (w >= (unsigned)a.n_tri) return;
    const uint4 *r = a.nodes + 4 * (size_t)(a.n_ids - 1 - id), *m = a.nrms + 3 * (size_t)id;
    for (int j = 0; j < 3; j++) {
        a.prev_pos[3 * (size_t)w + j] = r[j];
        a.prev_nrm[3 * (size_t)w + j] = m[j];
    }
}

}  // namespace motion
}  // namespace glrtx
