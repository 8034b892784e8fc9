// query.hip.h -- batched ray queries against the uploaded scene (glrtx_trace_rays / glrtx_trace_rays_device, include/glrtx.h).
//
// No reference counterpart: the renderer's own traversal opened to rays a host hands in.  Nothing here is a second traversal: trees are walked by
// trav_init / trav_step<true, COMPACT, ANY> and vines scanned by trav_scan<true, 1 | 2> (pt_kernel.hip.h), the renderer's code with the query's two
// template arguments -- a per-ray tmin in place of EPS, and the any-hit stop -- so a query's hit is the renderer's by construction.
//
// Ray record: 2 x float4 {ox, oy, oz, tmin} {dx, dy, dz, tmax}, read with two non-temporal 16-byte loads.  Hit record: one float4 {t, tri (int32 bits),
// u, v} written with one 16-byte store; tri is the WIRE triangle index (Args::wire maps the leaf id a hit carries), -1 on a miss, where t = tmax, u = v = 0.
//
// Launch: a persistent grid of 256-thread workgroups sized to the device (glrtx.hip: trace_launch).  No workgroup waits for another.  Waves claim rays
// from one global counter in chunks of 64; on trees a lane whose ray is finished takes the next ray of the chunk, by a cross-lane read, once at least
// kRefillMin lanes of its wave are idle (the wavefront kernel's traverse phase, wg_traverse_phase, does the same), so that the long rays of an incoherent
// batch do not hold a whole wave.  The per-lane stacks are in LDS (DevScene::stack_entries entries), then the compact layout's rank table when it is walked.
#pragma once
#include "pt_kernel.hip.h"

namespace glrtx {
namespace query {

constexpr int kChunk = 64;      // rays a wave claims at a time
constexpr int kRefillMin = 16;  // idle lanes from which a wave refills
constexpr int kStepsPerTrip = 2;  // trav_step calls between two looks at the refill

struct Args {
    DevScene sc;
    const float4 *rays;  // 2 per ray
    float4 *hits;        // 1 per ray
    const int *wire;     // leaf id -> wire triangle; id 0 (the never-hit record) -> -1
    unsigned *counter;   // rays claimed so far (zeroed before the launch)
    unsigned n;          // rays (< 2^31)
};

// Denormals are read as the zero of their sign, as the device's arithmetic reads them (and the CPU statement, host/query.cpp, under FTZ | DAZ): the
// comparisons against tmin / tmax then see the same values on both sides.
DEV float flush(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x7F800000u) == 0u ? __uint_as_float(b & 0x80000000u) : x;
}
DEV bool finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// The ray after flush(), and whether it needs a search at all: every component finite, a direction other than zero, tmin < tmax.  A ray that does not
// is answered with the miss record, which is also what a search of it would give.
DEV bool load_ray(const Args &q, unsigned i, float4 &o, float4 &d) {
    o = ld_stream(&q.rays[2 * (size_t)i]);
    d = ld_stream(&q.rays[2 * (size_t)i + 1]);
    o.x = flush(o.x); o.y = flush(o.y); o.z = flush(o.z); o.w = flush(o.w);
    d.x = flush(d.x); d.y = flush(d.y); d.z = flush(d.z); d.w = flush(d.w);
    const bool fin = finite(o.x) && finite(o.y) && finite(o.z) && finite(o.w) && finite(d.x) && finite(d.y) && finite(d.z) && finite(d.w);
    const bool dir = ((__float_as_uint(d.x) | __float_as_uint(d.y) | __float_as_uint(d.z)) & 0x7FFFFFFFu) != 0u;
    return fin && dir && o.w < d.w;
}

DEV void store_hit(const Args &q, unsigned i, const Hit &h) {
    const int w = h.tri >= 0 ? q.wire[h.tri] : -1;
    q.hits[i] = make_float4(h.t, __int_as_float(w), h.u, h.v);
}

// Trees: per-lane traversal with refill.  COMPACT: the 48-byte records (DevScene::cnodes) with the rank table staged in LDS.
template <bool ANY, bool COMPACT>
__global__ __launch_bounds__(kBlockThreads) void trace_tree(const Args q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    int *stack = reinterpret_cast<int *>(lds_raw) + 2 * threadIdx.x;
    uint2 *ranks = reinterpret_cast<uint2 *>(lds_raw + (size_t)2 * q.sc.stack_entries * kBlockThreads * sizeof(int));
    if (COMPACT) {
        for (int i = threadIdx.x; i < q.sc.n_crank; i += kBlockThreads) ranks[i] = q.sc.cranks[i];
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
    // this lane's record of the wave's current chunk, 1 / direction (:260) and whether the ray is searched: worked out when the chunk arrives, with all
    // lanes busy, not in the few lanes a refill serves
    float4 co = make_float4(0.f, 0.f, 0.f, 0.f), cd = co;
    float cix = 0.f, ciy = 0.f, ciz = 0.f;
    int cgo = 0;
    unsigned cur_base = 0;  // wave-uniform
    int cur_pos = 0, cur_cnt = 0;
    auto fetch = [&]() -> int {  // the next chunk; returns its number of rays (0: none left)
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(q.counter, (unsigned)kChunk);
        base = __builtin_amdgcn_readfirstlane(base);
        const int cnt = base >= q.n ? 0 : (q.n - base < (unsigned)kChunk ? (int)(q.n - base) : kChunk);
        cur_base = base;
        if (lane < cnt) {
            bool go = load_ray(q, base + lane, co, cd);
            cix = frcp(cd.x); ciy = frcp(cd.y); ciz = frcp(cd.z);
            float t0;
            if (go && q.sc.root_boxed && !box_pass(q.sc.root_lo, q.sc.root_hi, co.x, co.y, co.z, cix, ciy, ciz, cd.w, t0)) go = false;
            cgo = go ? 1 : 0;
        }
        return cnt;
    };
    cur_cnt = fetch();
    bool exhausted = cur_cnt == 0;
    bool active = false, unsaved = false;  // the finished ray's hit is written when the lane is refilled (a store inside the loop holds up every fetch behind it)
    unsigned rid = 0;
    float tmin = 0.f;
    Trav T;
    T.cur = REF_FIN; T.sp = 0; T.stop_d = -__builtin_inff();
    T.h.t = 0.f; T.h.tri = -1; T.h.u = 0.f; T.h.v = 0.f;
    for (;;) {
        unsigned long long idle = __ballot(!active);
        if ((int)__popcll(idle) >= kRefillMin || idle == ~0ull) {
            while (idle != 0ull && !exhausted) {
                if (cur_pos >= cur_cnt) {  // chunk used up: the next one
                    cur_cnt = cur_cnt == kChunk ? fetch() : 0;
                    cur_pos = 0;
                    if (cur_cnt == 0) { exhausted = true; break; }
                }
                const int n = __popcll(idle);
                const int avail = cur_cnt - cur_pos;
                const int take = n < avail ? n : avail;
                const int rank = __popcll(idle & lt_mask);
                const int src = (cur_pos + rank) & 63;
                const float ox = __shfl(co.x, src), oy = __shfl(co.y, src), oz = __shfl(co.z, src), t_min = __shfl(co.w, src);
                const float dx = __shfl(cd.x, src), dy = __shfl(cd.y, src), dz = __shfl(cd.z, src), t_max = __shfl(cd.w, src);
                const float ix = __shfl(cix, src), iy = __shfl(ciy, src), iz = __shfl(ciz, src);
                const int go = __shfl(cgo, src);
                if (!active && rank < take) {
                    if (unsaved) store_hit(q, rid, T.h);
                    rid = cur_base + (unsigned)src;
                    T.ox = ox; T.oy = oy; T.oz = oz; T.dx = dx; T.dy = dy; T.dz = dz; T.ix = ix; T.iy = iy; T.iz = iz;
                    T.h.t = t_max; T.h.tri = -1; T.h.u = 0.f; T.h.v = 0.f;  // trav_init's start: the search is limited to t < tmax
                    T.sp = 0;
                    T.cur = COMPACT ? 0 : q.sc.root_ref;  // (the compact array's root is position 0)
                    tmin = t_min;
                    active = go != 0;
                    unsaved = !active;  // no search (or the root box missed): the miss record is final
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
            bool fin = trav_step<true, COMPACT, ANY>(q.sc, stack, T, ranks, tmin);
#pragma unroll
            for (int k = 1; k < kStepsPerTrip; k++)
                if (!fin) fin = trav_step<true, COMPACT, ANY>(q.sc, stack, T, ranks, tmin);
            if (fin) {
                active = false;
                unsaved = true;
            }
        }
    }
    if (unsaved) store_hit(q, rid, T.h);
}

// Vines (DevScene::n_vine > 0): the list scan.  Every ray of a wave walks the same list positions, so a wave simply takes 64 rays at a time.
template <bool ANY>
__global__ __launch_bounds__(kBlockThreads) void trace_vine(const Args q) {
    const int lane = threadIdx.x & 63;
    for (;;) {
        unsigned base = 0;
        if (lane == 0) base = atomicAdd(q.counter, (unsigned)kChunk);
        base = __builtin_amdgcn_readfirstlane(base);
        if (base >= q.n) break;
        const bool valid = base + (unsigned)lane < q.n;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f), d = o;
        const bool go = valid && load_ray(q, base + lane, o, d);
        const Hit h = trav_scan<true, ANY ? 2 : 1>(q.sc, o.x, o.y, o.z, d.x, d.y, d.z, go, d.w, -__builtin_inff(), o.w);  // (not searched: {tmax, -1, 0, 0})
        if (valid) store_hit(q, base + lane, h);
    }
}

}  // namespace query
}  // namespace glrtx
