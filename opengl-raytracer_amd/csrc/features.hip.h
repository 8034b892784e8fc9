// features.hip.h -- the denoiser's feature planes (glrtx_render_features, include/glrtx.h "Denoising"): per owned pixel the shading normal and distance of the
// primary ray's closest hit, and the hit material's albedo and id.
//
// No reference counterpart.  Nothing here is a second traversal or a second camera: the ray is camera_ray's (pt_kernel.hip.h) with r0 = r1 = 0.5 and the thin
// lens skipped -- the same expressions in the same order --, trees are walked by trav_step<true, COMPACT> and vines scanned by trav_scan<true, 1> with the
// renderer's own constants (tmin = PT_EPS, limit PT_INFTY: a primary ray), and the normal and material id are surf_tri's.  The launch is query.hip.h's: a
// persistent grid, waves claiming 64 ids at a time from one counter, on trees per-lane refill once kRefillMin lanes are idle.  An id is a tile-order pixel id
// (wf_pixel's numbering: 8x8 tiles of the owned rows, row-major, lane k at (k & 7, k >> 3)), so a chunk is one tile and a wave's rays start out coherent; the
// rays are generated here, not staged through memory.  host/features.cpp states the same pass on the CPU, bit for bit.
//
// Planes (packed rows of `width` float4 over the owned rows):  N {nx, ny, nz, t}, a miss {0, 0, 0, 0};  A {albedo rgb, material id as int32 bits}: param0 of a
// diffuse material, {1, 1, 1} otherwise and on a miss (id -1).  A NaN normal component is stored as 0x7FC00000.
// The tree kernel is a template on its argument type, features_tree<COMPACT, A>, and the vine kernels are features_vine_* by name; A's store() says what is written:
// Under glrtx_track_motion GeomArgs adds a third plane  G {wire triangle as int32 bits, u, v, 0}, a miss {-1, 0, 0, 0}: the traversal's own hit, the
// triangle mapped through the ray queries' table (query::store_hit's).
// With a texture set bound (glrtx_upload_textures) TexArgs / TexGeomArgs add the set, and their store() puts the albedo tex_lookup finds at the hit's
// coordinates into A for a diffuse material bound to a texture -- what the extension kernel shades with.  The material id is unchanged.
// With material maps bound as well (glrtx_bind_material_maps) MapArgs / MapGeomArgs are the textured arguments, and their store() puts the mapped normal n'
// (maps.hip.h) into N for a hit whose material is bound to a normal map.
// With cutouts bound (glrtx_bind_cutouts; include/glrtx.h "Cutouts") CutArgs<Base> is any of the four textured argument types with the cutout tables behind
// it: the walk is then trav_step<true, COMPACT, false, true> -- the renderer's CUT step --, so the planes describe the surface the image shows, holes included.
// store() is Base's.  (A vine never gets here: glrtx_bind_cutouts refuses one.)
// With emission maps bound (glrtx_bind_emission_maps; include/glrtx.h "Emission maps") EmitArgs<Base> is any of the four textured argument types with the
// emission table behind it: store() is Base's, then A's rgb again -- the looked-up texel c, without the emission -- for a hit whose material is bound and
// not diffuse (host/texture.cpp: glrt_emission_albedo states it on plane G).  The walk is Base's; a vine is walked by features_vine_emit<Base>.
// Each form is launched only while what it adds is bound; the instantiations on Args are what is launched otherwise.
#pragma once
#include "query.hip.h"

namespace glrtx {
namespace features {

struct Args {
    DevScene sc;
    float cam[32];      // c2w[16], s2c[16]
    int width, height;  // full image
    int owned_rows, rank, world, stripe;
    int tiles8_x;
    unsigned n;         // ids: 64 x tiles
    float4 *out_n, *out_a;
    unsigned *counter;
};

DEV bool pixel_of(const Args &q, unsigned id, int &lx, int &lrow) {
    const int t = (int)(id >> 6), k = (int)(id & 63u);
    lx = (t % q.tiles8_x) * 8 + (k & 7);
    lrow = (t / q.tiles8_x) * 8 + (k >> 3);
    return lx < q.width && lrow < q.owned_rows;
}

// camera_ray (pt_kernel.hip.h:1436) at the pixel's centre; then query::load_ray's rule for what is searched at all
DEV bool centre_ray(const Args &q, int lx, int lrow, float4 &o, float4 &d) {
    const int gy = ((lrow / q.stripe) * q.world + q.rank) * q.stripe + lrow % q.stripe;  // local_row_to_y
    const float fcx = (float)lx + 0.5f, fcy = (float)gy + 0.5f;
    const float W = (float)q.width, H = (float)q.height;
    const float *S = q.cam + 16, *C = q.cam;
    const float nx = ((fcx + 0.5f) / W) * 2.0f + -1.0f;
    const float ny = ((fcy + 0.5f) / H) * 2.0f + -1.0f;
    const float tx = (S[0] * nx + S[12]) + S[4] * ny;
    const float ty = (S[1] * nx + S[13]) + S[5] * ny;
    const float tz = (S[2] * nx + S[14]) + S[6] * ny;
    const float tw = (S[3] * nx + S[15]) + S[7] * ny;
    const float cx = tx / tw, cy = ty / tw, cz = tz / tw;
    const float rn = rsq((cz * cz + cy * cy) + cx * cx);
    const float dx = cx * rn, dy = cy * rn, dz = cz * rn;
    const float lox = 0.0f, loy = 0.0f;
    const float wx = (C[0] * lox + C[12]) + C[4] * loy;
    const float wy = (C[1] * lox + C[13]) + C[5] * loy;
    const float wz = (C[2] * lox + C[14]) + C[6] * loy;
    const float ww = (C[3] * lox + C[15]) + C[7] * loy;
    const float ex = (C[0] * dx + C[4] * dy) + C[8] * dz;
    const float ey = (C[1] * dx + C[5] * dy) + C[9] * dz;
    const float ez = (C[2] * dx + C[6] * dy) + C[10] * dz;
    const float re = rsq((ez * ez + ey * ey) + ex * ex);
    o = make_float4(query::flush(wx / ww), query::flush(wy / ww), query::flush(wz / ww), PT_EPS);
    d = make_float4(query::flush(ex * re), query::flush(ey * re), query::flush(ez * re), PT_INFTY);
    const bool fin = query::finite(o.x) && query::finite(o.y) && query::finite(o.z) && query::finite(d.x) && query::finite(d.y) && query::finite(d.z);
    const bool dir = ((__float_as_uint(d.x) | __float_as_uint(d.y) | __float_as_uint(d.z)) & 0x7FFFFFFFu) != 0u;
    return fin && dir;
}

DEV float canon(float x) { return x != x ? __uint_as_float(0x7FC00000u) : x; }

DEV void store(const Args &q, unsigned id, const Hit &h) {
    int lx, lrow;
    if (!pixel_of(q, id, lx, lrow)) return;
    float4 N = make_float4(0.f, 0.f, 0.f, 0.f), A = make_float4(1.f, 1.f, 1.f, __int_as_float(-1));
    if (h.tri >= 0) {
        const Surf S = surf_tri(q.sc, h);
        N = make_float4(canon(S.nx), canon(S.ny), canon(S.nz), h.t);
        const float4 m0 = q.sc.mats[3 * S.mtrl], m1 = q.sc.mats[3 * S.mtrl + 1];
        if (__float_as_int(m0.w) == 2) { A.x = m1.x; A.y = m1.y; A.z = m1.z; }
        A.w = __int_as_float(S.mtrl);
    }
    const size_t p = (size_t)lrow * q.width + lx;
    q.out_n[p] = N;
    q.out_a[p] = A;
}

// The third plane (glrtx_track_motion): the feature pass's arguments, where G goes and the leaf id -> wire triangle table (id 0: -1)
struct GeomArgs : Args {
    float4 *out_g;
    const int *wire;
};

// (store(const Args &) stays as it is for the kernels without G; the second pixel_of below costs nothing: inlined into one function, the compiler merges the
// two -- the kernels on GeomArgs hold as many division chains as the kernels they extend)
DEV void store(const GeomArgs &q, unsigned id, const Hit &h) {
    store(static_cast<const Args &>(q), id, h);
    int lx, lrow;
    if (!pixel_of(q, id, lx, lrow)) return;
    float4 G = make_float4(__int_as_float(-1), 0.f, 0.f, 0.f);
    if (h.tri >= 0) G = make_float4(__int_as_float(q.wire[h.tri]), h.u, h.v, 0.f);
    q.out_g[(size_t)lrow * q.width + lx] = G;
}

// With textures: the planes as above, then A's rgb again for a hit whose material is bound (host/texture.cpp: glrt_texture_albedo states it on plane G)
DEV void store_albedo(const Args &q, const TexSet &ts, unsigned id, const Hit &h) {
    int lx, lrow;
    if (h.tri < 0 || !pixel_of(q, id, lx, lrow)) return;
    const int mtrl = __float_as_int(q.sc.nrms[3 * h.tri].w);
    const int k = ts.mat_tex[mtrl];
    if (k < 0) return;
    const float2 st = tex_hit_st(ts, h.tri, h.u, h.v);
    const float3 c = tex_lookup(ts, k, st.x, st.y);
    q.out_a[(size_t)lrow * q.width + lx] = make_float4(c.x, c.y, c.z, __int_as_float(mtrl));
}
struct TexArgs : Args {
    TexSet tex;
};
struct TexGeomArgs : GeomArgs {
    TexSet tex;
};
DEV void store(const TexArgs &q, unsigned id, const Hit &h) {
    store(static_cast<const Args &>(q), id, h);
    store_albedo(q, q.tex, id, h);
}
DEV void store(const TexGeomArgs &q, unsigned id, const Hit &h) {
    store(static_cast<const GeomArgs &>(q), id, h);
    store_albedo(q, q.tex, id, h);
}

// With material maps bound on top of the set (glrtx_bind_material_maps): the planes as above, then N's normal again for a hit whose material is bound to a
// normal map -- n' of maps.hip.h, what the extension kernel shades the primary hit with.  t, A, the material id and G are unchanged.
DEV void store_mapped_normal(const Args &q, const TexSet &ts, unsigned id, const Hit &h) {
    int lx, lrow;
    if (h.tri < 0 || !pixel_of(q, id, lx, lrow)) return;
    const MapRec mr = ts.maps[__float_as_int(q.sc.nrms[3 * h.tri].w)];
    if (mr.normal < 0) return;
    const Surf S = surf_tri(q.sc, h);
    const float3 n = map_hit_normal(ts, q.sc.forks, mr.normal, mr.scale, h.tri, tex_hit_st(ts, h.tri, h.u, h.v), make_float3(S.nx, S.ny, S.nz));
    q.out_n[(size_t)lrow * q.width + lx] = make_float4(canon(n.x), canon(n.y), canon(n.z), h.t);
}
struct MapArgs : TexArgs {};
struct MapGeomArgs : TexGeomArgs {};
DEV void store(const MapArgs &q, unsigned id, const Hit &h) {
    store(static_cast<const TexArgs &>(q), id, h);
    store_mapped_normal(q, q.tex, id, h);
}
DEV void store(const MapGeomArgs &q, unsigned id, const Hit &h) {
    store(static_cast<const TexGeomArgs &>(q), id, h);
    store_mapped_normal(q, q.tex, id, h);
}

// With cutouts bound: Base's arguments and store(), and the tables the CUT step reads (texture.hip.h)
template <class Base>
struct CutArgs : Base {
    CutSet cut;
};
template <class A>
struct is_cut : std::false_type {};
template <class Base>
struct is_cut<CutArgs<Base>> : std::true_type {};

// With emission maps bound: Base's arguments and store(), then the emitter's picture into A (a bound diffuse material keeps its albedo rule)
template <class Base>
struct EmitArgs : Base {
    EmitSet emit;
};
template <class Base>
DEV void store(const EmitArgs<Base> &q, unsigned id, const Hit &h) {
    store(static_cast<const Base &>(q), id, h);
    int lx, lrow;
    if (h.tri < 0 || !pixel_of(q, id, lx, lrow)) return;
    const int mtrl = __float_as_int(q.sc.nrms[3 * h.tri].w);
    const int k = q.emit.mat_emit[mtrl];
    if (k < 0 || __float_as_int(q.sc.mats[3 * mtrl].w) == 2) return;
    const float2 st = tex_hit_st(q.tex, h.tri, h.u, h.v);
    const float3 c = tex_lookup(q.tex, k, st.x, st.y);
    q.out_a[(size_t)lrow * q.width + lx] = make_float4(c.x, c.y, c.z, __int_as_float(mtrl));
}

template <class A>
struct is_emit : std::false_type {};
template <class Base>
struct is_emit<EmitArgs<Base>> : std::true_type {};

// Trees: query::trace_tree's loop with the ray made here.  A: the argument type, which chooses store().  The loop is stated in the kernel template and nowhere
// else: moved into a body shared by __global__ wrappers, the compiler allocated features_tree<*, Args>' registers differently (the same operations, other
// register numbers and a slightly different schedule), and that kernel is to keep its instructions (tools/isa_diff.py against a build of the parent shows it).
template <bool COMPACT, class A = Args>
__global__ __launch_bounds__(kBlockThreads) void features_tree(const A q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    int *stack = reinterpret_cast<int *>(lds_raw) + 2 * threadIdx.x;
    uint2 *ranks = reinterpret_cast<uint2 *>(lds_raw + (size_t)2 * q.sc.stack_entries * kBlockThreads * sizeof(int));
    if (COMPACT) {
        for (int i = threadIdx.x; i < q.sc.n_crank; i += kBlockThreads) ranks[i] = q.sc.cranks[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    float4 co = make_float4(0.f, 0.f, 0.f, 0.f), cd = co;  // this lane's ray of the wave's current chunk, 1 / direction, and whether it is searched
    float cix = 0.f, ciy = 0.f, ciz = 0.f;
    int cgo = 0;
    unsigned cur_base = 0;  // wave-uniform
    int cur_pos = 0, cur_cnt = 0;
    auto fetch = [&]() -> int {  // the next chunk (one 8x8 tile); returns its number of ids (0: none left)
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(q.counter, (unsigned)query::kChunk);
        base = __builtin_amdgcn_readfirstlane(base);
        const int cnt = base >= q.n ? 0 : query::kChunk;  // (n is a multiple of 64)
        cur_base = base;
        if (cnt) {
            int lx, lrow;
            bool go = pixel_of(q, base + lane, lx, lrow) && centre_ray(q, lx, lrow, co, cd);
            cix = frcp(cd.x); ciy = frcp(cd.y); ciz = frcp(cd.z);
            float t0;
            if (go && q.sc.root_boxed && !box_pass(q.sc.root_lo, q.sc.root_hi, co.x, co.y, co.z, cix, ciy, ciz, cd.w, t0)) go = false;
            cgo = go ? 1 : 0;
        }
        return cnt;
    };
    cur_cnt = fetch();
    bool exhausted = cur_cnt == 0;
    bool active = false, unsaved = false;  // a finished ray's planes are written when the lane is refilled
    unsigned rid = 0;
    Trav T;
    T.cur = REF_FIN; T.sp = 0; T.stop_d = -__builtin_inff();
    T.h.t = 0.f; T.h.tri = -1; T.h.u = 0.f; T.h.v = 0.f;
    for (;;) {
        unsigned long long idle = __ballot(!active);
        if ((int)__popcll(idle) >= query::kRefillMin || idle == ~0ull) {
            while (idle != 0ull && !exhausted) {
                if (cur_pos >= cur_cnt) {
                    cur_cnt = fetch();
                    cur_pos = 0;
                    if (cur_cnt == 0) { exhausted = true; break; }
                }
                const int n = __popcll(idle);
                const int avail = cur_cnt - cur_pos;
                const int take = n < avail ? n : avail;
                const int rank = __popcll(idle & lt_mask);
                const int src = (cur_pos + rank) & 63;
                const float ox = __shfl(co.x, src), oy = __shfl(co.y, src), oz = __shfl(co.z, src);
                const float dx = __shfl(cd.x, src), dy = __shfl(cd.y, src), dz = __shfl(cd.z, src);
                const float ix = __shfl(cix, src), iy = __shfl(ciy, src), iz = __shfl(ciz, src);
                const int go = __shfl(cgo, src);
                if (!active && rank < take) {
                    if (unsaved) store(q, rid, T.h);
                    rid = cur_base + (unsigned)src;
                    T.ox = ox; T.oy = oy; T.oz = oz; T.dx = dx; T.dy = dy; T.dz = dz; T.ix = ix; T.iy = iy; T.iz = iz;
                    T.h.t = PT_INFTY; T.h.tri = -1; T.h.u = 0.f; T.h.v = 0.f;  // trav_init's start
                    T.sp = 0;
                    T.cur = COMPACT ? 0 : q.sc.root_ref;
                    active = go != 0;
                    unsaved = !active;  // not searched, the root box missed, or outside the image (store() drops those)
                }
                cur_pos += take;
                idle = __ballot(!active);
            }
        }
        if (!__any(active)) {
            if (exhausted) break;
            continue;
        }
        if (active) {
            if constexpr (is_cut<A>::value) {  // cutouts bound: the same trip with the CUT step, which reads the launch's set and tables
                const CutRef cr{&q.tex, &q.cut};
                bool fin_cut = trav_step<true, COMPACT, false, true>(q.sc, stack, T, ranks, PT_EPS, &cr);
#pragma unroll
                for (int k = 1; k < query::kStepsPerTrip; k++)
                    if (!fin_cut) fin_cut = trav_step<true, COMPACT, false, true>(q.sc, stack, T, ranks, PT_EPS, &cr);
                if (fin_cut) {
                    active = false;
                    unsaved = true;
                }
            } else {
                bool fin = trav_step<true, COMPACT>(q.sc, stack, T, ranks);
#pragma unroll
                for (int k = 1; k < query::kStepsPerTrip; k++)
                    if (!fin) fin = trav_step<true, COMPACT>(q.sc, stack, T, ranks);
                if (fin) {
                    active = false;
                    unsaved = true;
                }
            }
        }
    }
    if (unsaved) store(q, rid, T.h);
}

// Vines: the list scan, a wave 64 ids (one tile) at a time.
template <class A>
DEV void vine_body(const A &q) {
    const int lane = threadIdx.x & 63;
    for (;;) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(q.counter, (unsigned)query::kChunk);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= q.n) break;
        int lx, lrow;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f), d = o;
        const bool go = pixel_of(q, base + lane, lx, lrow) && centre_ray(q, lx, lrow, o, d);
        const Hit h = trav_scan<true, 1>(q.sc, o.x, o.y, o.z, d.x, d.y, d.z, go, PT_INFTY, -__builtin_inff(), PT_EPS);  // (not searched: {PT_INFTY, -1, 0, 0})
        store(q, base + lane, h);
    }
}
__global__ __launch_bounds__(kBlockThreads) void features_vine(const Args q) { vine_body(q); }
__global__ __launch_bounds__(kBlockThreads) void features_vine_geom(const GeomArgs q) { vine_body(q); }
__global__ __launch_bounds__(kBlockThreads) void features_vine_tex(const TexArgs q) { vine_body(q); }
__global__ __launch_bounds__(kBlockThreads) void features_vine_geom_tex(const TexGeomArgs q) { vine_body(q); }
__global__ __launch_bounds__(kBlockThreads) void features_vine_maps(const MapArgs q) { vine_body(q); }
__global__ __launch_bounds__(kBlockThreads) void features_vine_geom_maps(const MapGeomArgs q) { vine_body(q); }
template <class Base>
__global__ __launch_bounds__(kBlockThreads) void features_vine_emit(const EmitArgs<Base> q) { vine_body(q); }

}  // namespace features
}  // namespace glrtx
