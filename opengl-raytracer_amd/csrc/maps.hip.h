// maps.hip.h -- material maps (include/glrtx.h "Material maps"): map_normal, the one device statement of the tangent-space normal rule, and map_alpha, the
// conductor's roughness from a texel.  Used by the extension megakernel's MAPS instantiations (pt_kernel.hip.h: bounce_ext<.., MAPS>), by the feature pass's
// *_maps kernels (features.hip.h) and by the kernel behind glrtx_debug_map_normal.
//
// Every operation is one rounded fp32 operation in the order written (the file is compiled with -ffp-contract=off, denormals flushed); host/maps.cpp
// (glrt_map_normal, glrt_map_alpha) and tests/maps_math.py state the same rule, bit for bit.  Dots are (x x' + y y') + z z' -- NOT dot3's order.
//
// TANGENTS ARE PER TRIANGLE AND ARE NOT INTERPOLATED.  The frame is formed at the hit from the leaf record's two edges e1 = v1 - v0, e2 = v2 - v0 (the words
// the refit rewrites after every move, in the wire's corner order: glrtx.hip, pack_scene) and the triangle's three frozen {s, t}: the tangent is the direction
// of increasing s in the triangle's plane, made orthogonal to the INTERPOLATED shading normal.  A mesh whose neighbouring triangles disagree about ds shows a
// crease in the mapped detail where an interpolated per-vertex tangent would not; the wire's tangent / binormal words are not read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "texture.hip.h"

namespace glrtx {

// == glrtx_material_map (include/glrtx.h), 16 bytes: texture indices of the bound set (-1: none) and the normal map's scale
struct MapRec {
    int normal, roughness;
    float scale;
    int reserved;
};
constexpr float MAP_ALPHA_MIN = 1e-3f;  // GLRTX_MAP_ALPHA_MIN
constexpr int kMapRecordFloats = 18;    // glrtx_debug_map_normal: {n, e1, e2, st0, st1, st2, m}

TEX_DEV float map_dot(float ax, float ay, float az, float bx, float by, float bz) { return (ax * bx + ay * by) + az * bz; }
TEX_DEV float map_rsq(float x) {  // == rsq (pt_kernel.hip.h): IEEE sqrt, then frcp's IEEE reciprocal
    const float s = __builtin_sqrtf(x);
    const float r = __builtin_amdgcn_rcpf(s);
    const float n = __builtin_fmaf(__builtin_fmaf(-s, r, 1.0f), r, r);
    return __builtin_amdgcn_class(s, 0x2F4) ? r : n;
}
TEX_DEV float map_neg(float x) { return __uint_as_float(__float_as_uint(x) ^ 0x80000000u); }                     // the sign bit inverted, whatever the value
TEX_DEV bool map_tiny(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0u; }                                // a zero or a denormal
TEX_DEV bool map_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
TEX_DEV bool map_pos_finite(float x) { return (__float_as_uint(x) - 0x00800000u) < 0x7F000000u; }                   // sign clear, exponent neither 0 nor 255

// texel -> tangent-space vector, every format: m = c * 2 + -1
TEX_DEV float3 map_decode(float3 c) { return make_float3(c.x * 2.0f + -1.0f, c.y * 2.0f + -1.0f, c.z * 2.0f + -1.0f); }

// The rule.  n: surf_tri's shading normal; e1, e2: the leaf record's edges; (s0, t0) .. (s2, t2): the corners' coordinates; m: the decoded texel.  Returns n',
// or n word for word where the contract keeps it: det zero or not finite, l2 or q not a finite positive number, a and b both zero.
TEX_DEV float3 map_normal(float3 n, float3 e1, float3 e2, float2 st0, float2 st1, float2 st2, float3 m, float scale) {
    const float a = m.x * scale, b = m.y * scale;
    if (map_tiny(a) && map_tiny(b)) return n;  // a flat texel: the unmapped image, bit for bit
    const float ds1 = st1.x - st0.x, ds2 = st2.x - st0.x, dt1 = st1.y - st0.y, dt2 = st2.y - st0.y;
    const float det = ds1 * dt2 - ds2 * dt1;
    if (map_tiny(det) || !map_finite(det)) return n;
    float Trx = e1.x * dt2 - e2.x * dt1, Try = e1.y * dt2 - e2.y * dt1, Trz = e1.z * dt2 - e2.z * dt1;
    float Brx = e2.x * ds1 - e1.x * ds2, Bry = e2.y * ds1 - e1.y * ds2, Brz = e2.z * ds1 - e1.z * ds2;
    if (det < 0.0f) {
        Trx = map_neg(Trx); Try = map_neg(Try); Trz = map_neg(Trz);
        Brx = map_neg(Brx); Bry = map_neg(Bry); Brz = map_neg(Brz);
    }
    const float k = map_dot(n.x, n.y, n.z, Trx, Try, Trz);
    const float Tpx = Trx - k * n.x, Tpy = Try - k * n.y, Tpz = Trz - k * n.z;
    const float l2 = map_dot(Tpx, Tpy, Tpz, Tpx, Tpy, Tpz);
    if (!map_pos_finite(l2)) return n;
    const float rl = map_rsq(l2);
    const float Tx = Tpx * rl, Ty = Tpy * rl, Tz = Tpz * rl;
    float Bx = n.y * Tz - n.z * Ty, By = n.z * Tx - n.x * Tz, Bz = n.x * Ty - n.y * Tx;  // C = cross(n, T)
    if (map_dot(Bx, By, Bz, Brx, Bry, Brz) < 0.0f) { Bx = map_neg(Bx); By = map_neg(By); Bz = map_neg(Bz); }
    const float px = (a * Tx + b * Bx) + m.z * n.x;
    const float py = (a * Ty + b * By) + m.z * n.y;
    const float pz = (a * Tz + b * Bz) + m.z * n.z;
    const float q = map_dot(px, py, pz, px, py, pz);
    if (!map_pos_finite(q)) return n;
    const float rq = map_rsq(q);
    return make_float3(px * rq, py * rq, pz * rq);
}

// The conductor's (alpha.x, alpha.y) from a roughness texel: channels r and g, floored; b and alpha are not read
TEX_DEV float2 map_alpha(float3 c) { return make_float2(c.x > MAP_ALPHA_MIN ? c.x : MAP_ALPHA_MIN, c.y > MAP_ALPHA_MIN ? c.y : MAP_ALPHA_MIN); }

// n' at a hit (u, v) of device triangle `tri` whose material is bound to normal map `k`: the lookup, the leaf record's edges, the rule
TEX_DEV float3 map_hit_normal(const TexSet &ts, const float4 *forks, int k, float scale, int tri, float2 st, float3 n) {
    const float3 m = map_decode(tex_lookup(ts, k, st.x, st.y));
    const float4 *rec = forks + 4 * (ptrdiff_t)~tri;  // {v0, mat} {v1 - v0, next} {v2 - v0, 0} (DevScene::forks)
    const float4 E1 = rec[1], E2 = rec[2];
    return map_normal(n, make_float3(E1.x, E1.y, E1.z), make_float3(E2.x, E2.y, E2.z), ts.tri_st[3 * tri], ts.tri_st[3 * tri + 1], ts.tri_st[3 * tri + 2], m, scale);
}

// glrtx_debug_map_normal: out[3i..] = map_normal(record i, scale)
__global__ __launch_bounds__(256) void map_normal_kernel(const float *rec, unsigned n, float scale, float *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float *r = rec + (size_t)kMapRecordFloats * i;
    const float3 o = map_normal(make_float3(r[0], r[1], r[2]), make_float3(r[3], r[4], r[5]), make_float3(r[6], r[7], r[8]), make_float2(r[9], r[10]),
                                make_float2(r[11], r[12]), make_float2(r[13], r[14]), make_float3(r[15], r[16], r[17]), scale);
    out[3 * i] = o.x; out[3 * i + 1] = o.y; out[3 * i + 2] = o.z;
}

}  // namespace glrtx
