// refit.hip.h -- the device refit behind glrtx_update_vertices (include/glrtx.h): every geometry-derived scene buffer rewritten from a new vertex array and
// the plan glrtx_upload_scene kept (glrtx.hip: RefitPlan), byte-identical to what glrtx_upload_scene(new vertices, glrt_bvh_refit(old tree)) uploads.
//
// Three launches on the context's stream:
//   k_refit_leaves  one thread per leaf record: its 64-byte record {v0, mat} {v1 - v0, next} {v2 - v0, 0}, its normals, its wire box; then the climb -- an
//                   arrival counter per two-child fork lets the LAST child to arrive fold the fork and go on up, so a tree of any depth is one pass.  Also the
//                   terminals without a triangle (forks with no children: they keep their box and only climb) and the light records.
//   k_refit_vine    vines only (every fork's children.y a leaf; the chain tree): the forks' boxes as a parallel suffix fold over the leaf list, in one
//                   workgroup, instead of a climb through n - 1 serial levels.  Exact: the fold is on ordered-integer keys (below), so association is free.
//   k_refit_scatter the wire boxes into the 64-byte fork records, the compact records (cnodes), the vine list; the root box and vine_uniform for the read-back.
//
// Boxes are kept as ordered-integer keys (glrt_host.h, glrt_bvh_refit): key(u) = u ^ 0xffffffff for a set sign bit, u | 0x80000000 otherwise.  Min / max on
// keys is a total order on bit patterns (-0 < +0, NaNs beyond +-inf), needs no float instruction -- so nothing is flushed under the library's
// -fgpu-flush-denormals-to-zero -- and gives the host's bits whatever order the children arrive in.  Every other word is moved as an integer.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace glrtx {
namespace refit {

constexpr int kBlock = 256;
constexpr int kVineBlock = 1024;

struct Args {
    const unsigned *vert;   // the new vertices, GLRT_VERTEX_FLOATS (15) words each: position at 0..2, normal at 3..5
    const int4 *leaf;       // leaf record k (id k + 1): {three vertex indices, wire node}
    int n_leaf;
    const int *extra;       // reachable forks with no children (terminals without a triangle)
    int n_extra;
    const int4 *light;      // light record l: {three vertex indices, -}
    int n_light;
    const int *parent;      // wire node -> parent (-1: the root, or unreachable)
    const int2 *kids;       // wire node -> {children.x, children.y} (-1: absent)
    unsigned *cnt;          // wire node -> arrivals so far (0 between refits: the last arrival resets it)
    unsigned *box;          // wire node -> its box as 6 keys {lo xyz, hi xyz}
    int climb;              // 1: k_refit_leaves climbs; 0: a vine, k_refit_vine folds the forks
    uint4 *nodes;           // the 64-byte node array: leaf id k at record n_ids - 1 - k, fork record r at n_ids + r (4 uint4 per record)
    int n_ids;
    uint4 *nrms;            // 3 per id
    uint4 *lights;          // 6 per light
    const int2 *slot;       // fork record r -> the wire fork whose box lies in its left / right slot (-1: a leaf child or none: the +-inf box, never rewritten)
    int n_fork;
    const int *cpos;        // compact position -> fork record, or -1 (a leaf record: its id is in the position's first word .w)
    int n_cpos;
    uint4 *cnodes;          // 3 per position
    const int *vine_fork;   // vine record i < n_vine - 1 -> its wire fork
    const int *vine_leaf;   // the vine's leaves in list order (children.y of fork i, then the last fork's children.x)
    int n_vine, vine_main;
    uint4 *vine;            // 4 per record
    int root_boxed;
    unsigned *out;          // {root lo xyz, root hi xyz, vine_uniform, -}: read back by the host (kernel arguments)
};

__device__ __forceinline__ unsigned key_of(unsigned u) { return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ unsigned bits_of(unsigned k) { return (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k; }

// The float subtraction pack_scene performs on the host (an IEEE binary32 subtraction, round to nearest even, denormals kept; x86 SSE for NaN / inf), as
// integer and double arithmetic that no flush can touch.  Both operands are widened to double EXACTLY from their bits (a denormal from its integer
// significand); their double difference rounded once more to binary32, by integer code, is the correctly rounded binary32 difference: double rounding is
// innocuous for + and - when the wide format has at least 2p + 1 = 49 bits (53 here; Figueroa 1995).  A result below 2^-126 in magnitude is a multiple of
// 2^-149 smaller than 2^-126, hence exact in both formats: it is written as the denormal it is.  No fpext / fptrunc appears, so the compiler cannot narrow
// the subtraction back to a float one (which the flush mode would change).
__device__ __forceinline__ double widen(unsigned u) {
    const unsigned long long s = (unsigned long long)(u >> 31) << 63;
    const unsigned e = (u >> 23) & 0xffu, m = u & 0x7fffffu;
    if (e == 0u) {
        if (m == 0u) return __longlong_as_double((long long)s);
        const int p = 31 - __clz((int)m);  // leading bit: the value is 1.f x 2^(p - 149)
        const unsigned long long mant = ((unsigned long long)m << (52 - p)) & ((1ull << 52) - 1ull);
        return __longlong_as_double((long long)(s | ((unsigned long long)(p - 149 + 1023) << 52) | mant));
    }
    return __longlong_as_double((long long)(s | ((unsigned long long)(e - 127u + 1023u) << 52) | ((unsigned long long)m << 29)));
}

__device__ __forceinline__ unsigned narrow(double d) {  // d: finite, the double difference of two binary32 values
    const unsigned long long b = (unsigned long long)__double_as_longlong(d);
    const unsigned s = (unsigned)(b >> 63) << 31;
    const int E = (int)((b >> 52) & 0x7ffu) - 1023;
    const unsigned long long mant = b & ((1ull << 52) - 1ull);
    if (((b >> 52) & 0x7ffu) == 0u) return s;  // zero (no double here is denormal)
    if (E < -126) return s | (unsigned)((mant | (1ull << 52)) >> (-97 - E));  // exact denormal: E >= -149, so the shift is 30 ... 52
    unsigned e32 = (unsigned)(E + 127), m = (unsigned)(mant >> 29);
    const unsigned long long rem = mant & ((1ull << 29) - 1ull), half = 1ull << 28;
    if (rem > half || (rem == half && (m & 1u))) {
        if (++m == (1u << 23)) { m = 0u; e32++; }
    }
    if (e32 >= 255u) return s | 0x7f800000u;
    return s | (e32 << 23) | m;
}

__device__ __forceinline__ unsigned host_sub(unsigned a, unsigned b) {  // a - b
    const bool fa = ((a >> 23) & 0xffu) == 0xffu, fb = ((b >> 23) & 0xffu) == 0xffu;
    if (fa || fb) {  // SSE: a NaN operand comes back quieted (the first one if both are); inf - inf of one sign is the default NaN
        if (fa && (a & 0x7fffffu)) return a | 0x400000u;
        if (fb && (b & 0x7fffffu)) return b | 0x400000u;
        if (fa && fb) return ((a ^ b) & 0x80000000u) ? a : 0xffc00000u;
        return fa ? a : (b ^ 0x80000000u);
    }
    return narrow(widen(a) - widen(b));
}

__device__ __forceinline__ void st_relaxed(unsigned *p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned ld_relaxed(const unsigned *p) { return __hip_atomic_load(const_cast<unsigned *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// Bottom-up from wire node n, whose box is stored: at a two-child fork the first arrival stops, the second folds.  Hand-off: the box words are stored and
// loaded as agent-scope atomics (write-through, L1 bypassed), drained, and the counter add is acq_rel at agent scope -- release of this lane's box stores,
// acquire of the sibling's.
__device__ void climb(const Args &a, int n) {
    while (true) {
        const int p = a.parent[n];
        if (p < 0) return;
        const int2 k = a.kids[p];
        if (k.x >= 0 && k.y >= 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned prev = __hip_atomic_fetch_add(&a.cnt[p], 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
            if (prev == 0u) return;  // the sibling's subtree is not done: its last thread folds p
            st_relaxed(&a.cnt[p], 0u);  // (nothing else touches p's counter in this launch)
        }
        unsigned b[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
        for (int c = 0; c < 2; c++) {
            const int ch = c ? k.y : k.x;
            if (ch < 0) continue;
            for (int j = 0; j < 3; j++) {
                b[j] = min(b[j], ld_relaxed(&a.box[6 * (size_t)ch + j]));
                b[3 + j] = max(b[3 + j], ld_relaxed(&a.box[6 * (size_t)ch + 3 + j]));
            }
        }
        for (int j = 0; j < 6; j++) st_relaxed(&a.box[6 * (size_t)p + j], b[j]);
        n = p;
    }
}

__global__ __launch_bounds__(kBlock) void k_refit_leaves(Args a) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) a.out[6] = 1u;  // vine_uniform until k_refit_scatter finds a fork box that differs from the root's
    if (i < a.n_leaf) {
        const int4 L = a.leaf[i];
        const unsigned *v[3] = {a.vert + 15 * (size_t)L.x, a.vert + 15 * (size_t)L.y, a.vert + 15 * (size_t)L.z};
        unsigned p[3][3], nr[3][3];
        for (int k = 0; k < 3; k++)
            for (int j = 0; j < 3; j++) { p[k][j] = v[k][j]; nr[k][j] = v[k][3 + j]; }
        uint4 *r = a.nodes + 4 * (size_t)(a.n_ids - 2 - i);  // id i + 1
        uint4 q = r[0]; q.x = p[0][0]; q.y = p[0][1]; q.z = p[0][2]; r[0] = q;
        q = r[1]; q.x = host_sub(p[1][0], p[0][0]); q.y = host_sub(p[1][1], p[0][1]); q.z = host_sub(p[1][2], p[0][2]); r[1] = q;
        q = r[2]; q.x = host_sub(p[2][0], p[0][0]); q.y = host_sub(p[2][1], p[0][1]); q.z = host_sub(p[2][2], p[0][2]); r[2] = q;
        uint4 *m = a.nrms + 3 * (size_t)(i + 1);
        for (int k = 0; k < 3; k++) { q = m[k]; q.x = nr[k][0]; q.y = nr[k][1]; q.z = nr[k][2]; m[k] = q; }
        unsigned *b = a.box + 6 * (size_t)L.w;
        for (int j = 0; j < 3; j++) {
            const unsigned k0 = key_of(p[0][j]), k1 = key_of(p[1][j]), k2 = key_of(p[2][j]);
            st_relaxed(&b[j], min(k0, min(k1, k2)));
            st_relaxed(&b[3 + j], max(k0, max(k1, k2)));
        }
        if (a.climb) climb(a, L.w);
        return;
    }
    const int e = i - a.n_leaf;
    if (e < a.n_extra) {  // its box is the uploaded one (a fork with no children keeps its box)
        if (a.climb) climb(a, a.extra[e]);
        return;
    }
    const int l = e - a.n_extra;
    if (l < a.n_light) {
        const int4 L = a.light[l];
        const int vi[3] = {L.x, L.y, L.z};
        uint4 *r = a.lights + 6 * (size_t)l;
        for (int k = 0; k < 3; k++) {
            const unsigned *v = a.vert + 15 * (size_t)vi[k];
            uint4 q = r[k]; q.x = v[0]; q.y = v[1]; q.z = v[2]; r[k] = q;
            q = r[3 + k]; q.x = v[3]; q.y = v[4]; q.z = v[5]; r[3 + k] = q;
        }
    }
}

__device__ __forceinline__ void fold6(unsigned *d, const unsigned *s) {
    for (int j = 0; j < 3; j++) { d[j] = min(d[j], s[j]); d[3 + j] = max(d[3 + j], s[3 + j]); }
}

// One workgroup: thread t folds a contiguous run of the leaf list, the runs' folds are suffix-scanned in LDS, and every thread walks its run back to front
// from the fold of everything behind it, writing fork i's box = fold(leaves i .. n - 1).
__global__ __launch_bounds__(kVineBlock) void k_refit_vine(Args a) {
    __shared__ unsigned part[6][kVineBlock];
    const int t = threadIdx.x, n = a.n_vine;
    const int chunk = (n + kVineBlock - 1) / kVineBlock;
    const int lo = min(n, t * chunk), hi = min(n, lo + chunk);
    unsigned acc[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    for (int i = lo; i < hi; i++) fold6(acc, a.box + 6 * (size_t)a.vine_leaf[i]);
    for (int j = 0; j < 6; j++) part[j][t] = acc[j];
    __syncthreads();
    for (int d = 1; d < kVineBlock; d <<= 1) {  // inclusive suffix fold of the runs
        unsigned o[6];
        const bool has = t + d < kVineBlock;
        if (has) for (int j = 0; j < 6; j++) o[j] = part[j][t + d];
        __syncthreads();
        if (has) {
            for (int j = 0; j < 3; j++) { part[j][t] = min(part[j][t], o[j]); part[3 + j][t] = max(part[3 + j][t], o[3 + j]); }
        }
        __syncthreads();
    }
    unsigned s[6] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0u, 0u, 0u};
    if (t + 1 < kVineBlock)
        for (int j = 0; j < 6; j++) s[j] = part[j][t + 1];
    for (int i = hi - 1; i >= lo; i--) {
        fold6(s, a.box + 6 * (size_t)a.vine_leaf[i]);
        if (i < n - 1)
            for (int j = 0; j < 6; j++) a.box[6 * (size_t)a.vine_fork[i] + j] = s[j];
    }
}

__device__ __forceinline__ void wire_box(const Args &a, int w, unsigned lo[3], unsigned hi[3]) {  // w < 0: the +-inf box of a leaf child / absent child
    for (int j = 0; j < 3; j++) {
        lo[j] = w < 0 ? 0xff800000u : bits_of(a.box[6 * (size_t)w + j]);
        hi[j] = w < 0 ? 0x7f800000u : bits_of(a.box[6 * (size_t)w + 3 + j]);
    }
}

__global__ __launch_bounds__(kBlock) void k_refit_scatter(Args a) {
    int i = blockIdx.x * kBlock + threadIdx.x;
    unsigned lo[3], hi[3];
    if (i < 2 * a.n_fork) {  // a fork record's slot
        const int2 s = a.slot[i >> 1];
        const int w = (i & 1) ? s.y : s.x;
        if (w < 0) return;
        wire_box(a, w, lo, hi);
        uint4 *r = a.nodes + 4 * ((size_t)a.n_ids + (size_t)(i >> 1)) + 2 * (i & 1);
        uint4 q = r[0]; q.x = lo[0]; q.y = lo[1]; q.z = lo[2]; r[0] = q;
        q = r[1]; q.x = hi[0]; q.y = hi[1]; q.z = hi[2]; r[1] = q;
        return;
    }
    i -= 2 * a.n_fork;
    if (i < a.n_cpos) {  // a compact position
        uint4 *o = a.cnodes + 3 * (size_t)i;
        const int f = a.cpos[i];
        if (f >= 0) {  // {minL, maxR.x} {maxL, maxR.y} {minR, maxR.z}
            const int2 s = a.slot[f];
            unsigned lo2[3], hi2[3];
            wire_box(a, s.x, lo, hi);
            wire_box(a, s.y, lo2, hi2);
            o[0] = make_uint4(lo[0], lo[1], lo[2], hi2[0]);
            o[1] = make_uint4(hi[0], hi[1], hi[2], hi2[1]);
            o[2] = make_uint4(lo2[0], lo2[1], lo2[2], hi2[2]);
        } else {  // {v0, id} {v1 - v0, next} {v2 - v0, 0}: the leaf record k_refit_leaves wrote
            const int id = (int)o[0].w;
            const uint4 *r = a.nodes + 4 * (size_t)(a.n_ids - 1 - id);
            for (int k = 0; k < 3; k++) { uint4 q = o[k]; q.x = r[k].x; q.y = r[k].y; q.z = r[k].z; o[k] = q; }
        }
        return;
    }
    i -= a.n_cpos;
    if (i < a.n_vine) {  // {box min, v0.x} {box max, v0.y} {v0.z, v1 - v0} {v2 - v0, id}
        const int rec = i < a.n_vine - 1 ? i : a.vine_main;
        uint4 *o = a.vine + 4 * (size_t)rec;
        const int w = i < a.n_vine - 1 ? a.vine_fork[i] : -1;
        wire_box(a, w, lo, hi);
        const unsigned id = o[3].w;
        const uint4 *r = a.nodes + 4 * (size_t)(a.n_ids - 1 - (int)id);
        const uint4 t0 = r[0], t1 = r[1], t2 = r[2];
        o[0] = make_uint4(lo[0], lo[1], lo[2], t0.x);
        o[1] = make_uint4(hi[0], hi[1], hi[2], t0.y);
        o[2] = make_uint4(t0.z, t1.x, t1.y, t1.z);
        o[3] = make_uint4(t2.x, t2.y, t2.z, id);
        if (w >= 0) {  // pack_scene: a memcmp of every fork box against the root's (node 0)
            unsigned rl[3], rh[3];
            wire_box(a, 0, rl, rh);
            bool same = true;
            for (int j = 0; j < 3; j++) same = same && lo[j] == rl[j] && hi[j] == rh[j];
            if (!same) atomicAnd(&a.out[6], 0u);
        }
        return;
    }
    i -= a.n_vine;
    if (i == 0) {
        if (a.root_boxed) wire_box(a, 0, lo, hi);
        for (int j = 0; j < 3; j++) { a.out[j] = a.root_boxed ? lo[j] : 0u; a.out[3 + j] = a.root_boxed ? hi[j] : 0u; }
    }
}

}  // namespace refit
}  // namespace glrtx
