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
// hits --; the four taps, the store and the 64 counter slots are reproject_kernel's.  No LDS, no scratch.
//
// The previous geometry: two arrays indexed by WIRE triangle, three float4 each -- {p0} {p1 - p0} {p2 - p0} (the leaf record's own words: pack_scene's
// edges, denormals kept) and {n0} {n1} {n2}.  snapshot_kernel copies them out of the scene's leaf records before the first refit after a feature pass.
#pragma once
#include "reproject.hip.h"

namespace glrtx {
namespace motion {

struct Args {
    float W[16], S[16];       // inverse(c2w_prev), inverse(s2c_prev)
    float opx, opy, opz;      // the previous camera's origin
    const float4 *acc;        // the old view: accumulator (pitch_f4 per row) and planes (packed rows of width)
    const float4 *n0, *a0;
    const float4 *g1, *a1;    // the new view's planes
    const float4 *prev_pos;   // 3 per wire triangle: {p0} {e1} {e2}
    const float4 *prev_nrm;   // 3 per wire triangle: the vertex normals
    int n_tri;                // triangles the two arrays hold
    float4 *out;              // pitch_f4 per row
    int pitch_f4, width, rows, tiles_x, n_tiles;
    float max_history, depth_tol, normal_tol;
    unsigned long long *counts;  // reproject::kCountSlots words
    const float4 *mom;        // the old view's moments plane M (pitch_f4 per row), or null; mom_out: the new view's (reproject::Args')
    float4 *mom_out;
};

__global__ __launch_bounds__(256) void reproject_motion_kernel(const Args a) {
    using reproject::canon;
    using reproject::pos_finite;
    using reproject::tiny;
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), k = threadIdx.x & 63;
    const int x = (tile % a.tiles_x) * 8 + (k & 7), y = (tile / a.tiles_x) * 8 + (k >> 3);
    const bool in = tile < a.n_tiles && x < a.width && y < a.rows;
    bool hit = false, carried = false;
    float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f), m4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (in) {
        const size_t p = (size_t)y * a.width + x;
        const float4 G1 = ld_stream(a.g1 + p), A1 = ld_stream(a.a1 + p);
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
            const float *W = a.W, *S = a.S;
            const float qx = ((W[0] * Px + W[4] * Py) + W[8] * Pz) + W[12];
            const float qy = ((W[1] * Px + W[5] * Py) + W[9] * Pz) + W[13];
            const float qz = ((W[2] * Px + W[6] * Py) + W[10] * Pz) + W[14];
            const float qw = ((W[3] * Px + W[7] * Py) + W[11] * Pz) + W[15];
            const float sx = ((S[0] * qx + S[4] * qy) + S[8] * qz) + S[12] * qw;
            const float sy = ((S[1] * qx + S[5] * qy) + S[9] * qz) + S[13] * qw;
            const float sw4 = ((S[3] * qx + S[7] * qy) + S[11] * qz) + S[15] * qw;
            const float Wf = (float)a.width, Hf = (float)a.rows;
            const float ui = ((sx / sw4 + 1.0f) * 0.5f) * Wf + -1.0f;
            const float vi = ((sy / sw4 + 1.0f) * 0.5f) * Hf + -1.0f;
            // (outside [-1, size) no tap lies inside the image; a NaN fails the comparisons)
            if (pos_finite(sw4) && ui >= -1.0f && ui < Wf && vi >= -1.0f && vi < Hf) {
                const float ex = Px - a.opx, ey = Py - a.opy, ez = Pz - a.opz;
                const float e = __builtin_sqrtf((ez * ez + ey * ey) + ex * ex);
                const float lim = a.depth_tol * e;
                const float fx0 = __builtin_floorf(ui), fy0 = __builtin_floorf(vi);
                const int x0 = (int)fx0, y0 = (int)fy0;
                const float fx = ui - fx0, fy = vi - fy0;
                const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
                float sw = 0.f, sc = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
                reproject::MomSum ms = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 2; j++) {
#pragma unroll
                    for (int i = 0; i < 2; i++) {
                        const int tx = x0 + i, ty = y0 + j;
                        if (tx < 0 || tx >= a.width || ty < 0 || ty >= a.rows) continue;
                        const size_t q = (size_t)ty * a.width + tx;
                        const float4 A0 = a.a0[q];
                        if (__float_as_int(A0.w) != id) continue;
                        const float4 C = a.acc[(size_t)ty * a.pitch_f4 + tx];
                        const float4 N0 = a.n0[q];
                        if (tiny(C.w)) continue;
                        if (!(dot3(M.nx, M.ny, M.nz, N0.x, N0.y, N0.z) >= a.normal_tol)) continue;
                        if (!(__builtin_fabsf(N0.w - e) <= lim)) continue;
                        const float w = wx[i] * wy[j];
                        sw = sw + w;
                        sc = sc + w * C.w;
                        sr = sr + w * (C.x / C.w); sg = sg + w * (C.y / C.w); sb = sb + w * (C.z / C.w);
                        if (a.mom) reproject::moments_tap(ms, w, a.mom[(size_t)ty * a.pitch_f4 + tx]);
                    }
                }
                if (sw > reproject::kMinWeight) {
                    const float r = __builtin_rintf(sc / sw);
                    const float n = r > a.max_history ? a.max_history : r;
                    if (n >= 1.0f) {
                        o4 = make_float4(canon((sr / sw) * n), canon((sg / sw) * n), canon((sb / sw) * n), n);
                        carried = true;
                        if (a.mom) m4 = reproject::moments_out(ms, a.max_history);
                    }
                }
            }
        }
        a.out[(size_t)y * a.pitch_f4 + x] = o4;
        if (a.mom_out) a.mom_out[(size_t)y * a.pitch_f4 + x] = m4;
    }
    const unsigned long long nc = __popcll(__ballot(carried)), nh = __popcll(__ballot(hit));
    if (k == 0 && (nc | nh) != 0ull)
        atomicAdd(a.counts + (size_t)(blockIdx.x % reproject::kCountSlots) * reproject::kCountStride, nc | (nh << 32));
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
