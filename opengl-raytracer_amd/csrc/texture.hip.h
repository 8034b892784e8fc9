// texture.hip.h -- filtered texture lookups (include/glrtx.h "Textures"): tex_lookup, the one device statement of the rule, used by the extension megakernel's
// shading (pt_kernel.hip.h: bounce_ext<VOL, true>), by the feature pass's textured kernels (features.hip.h) and by the kernel behind glrtx_debug_texture_lookup.
//
// gfx950 has no image-sampling path: a lookup is address arithmetic and one (nearest) or four (bilinear) gathers -- a 16-byte load a texel for RGBA32F, a
// 4-byte load for the two 8-bit formats.  Texels are row-major; there are no mip levels.  Every operation is one rounded fp32 operation in the order written
// (the file is compiled with -ffp-contract=off); host/texture.cpp and tests/texture_math.py state the same rule, bit for bit.
//
// The sRGB decode table is 1 KiB of constants in global memory, read with one per-lane load a channel: a texture's bytes differ from lane to lane, so the
// table is gathered whatever it lies in, and 1 KiB stays in a CU's cache while a textured launch runs.  Staging it into LDS would cost every workgroup of the
// extension kernel 1 KiB and a barrier, also in launches whose textures are not sRGB; that form has not been measured against this one.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace glrtx {

#define TEX_DEV __device__ __forceinline__

// == glrtx_texture (include/glrtx.h), 32 bytes
struct TexDesc {
    unsigned long long offset;
    int width, height, format, wrap_s, wrap_t, filter;
};
constexpr int TEX_RGBA32F = 0, TEX_RGBA8_UNORM = 1, TEX_RGBA8_SRGB = 2;
constexpr int TEX_REPEAT = 0, TEX_CLAMP = 1;
constexpr int TEX_NEAREST = 0, TEX_BILINEAR = 1;

// A bound set.  tri_st: three {s, t} a device triangle (the index surf_tri reads nrms with; triangle 0 is the never-hit record), frozen when the set was
// uploaded.  mat_tex: texture index a material, -1 untextured.  maps: the material maps bound on top of the set (glrtx_bind_material_maps; maps.hip.h), one record
// a material, or null; only the MAPS instantiations read it, and they are launched only while maps are bound.
struct MapRec;
struct TexSet {
    const TexDesc *desc;
    const unsigned char *texels;
    const float2 *tri_st;
    const int *mat_tex;
    int n_tex;
    const MapRec *maps;
};

// sRGB byte -> linear: the piecewise formula in float64, rounded once to fp32 (bit patterns; tests/test_texture_host.py recomputes them)
__device__ const unsigned kSrgbBits[256] = {
    0x00000000u, 0x399f22b4u, 0x3a1f22b4u, 0x3a6eb40eu, 0x3a9f22b4u, 0x3ac6eb61u, 0x3aeeb40eu, 0x3b0b3e5du,
    0x3b1f22b4u, 0x3b33070au, 0x3b46eb61u, 0x3b5b518eu, 0x3b70f18fu, 0x3b83e1c6u, 0x3b8fe616u, 0x3b9c87fdu,
    0x3ba9c9b6u, 0x3bb7ad6fu, 0x3bc6354au, 0x3bd56360u, 0x3be539c1u, 0x3bf5ba71u, 0x3c0373b6u, 0x3c0c6153u,
    0x3c15a705u, 0x3c1f45beu, 0x3c293e6bu, 0x3c3391f7u, 0x3c3e4149u, 0x3c494d44u, 0x3c54b6c9u, 0x3c607eb4u,
    0x3c6ca5dfu, 0x3c792d22u, 0x3c830aa9u, 0x3c89af9fu, 0x3c9085dcu, 0x3c978dc6u, 0x3c9ec7c2u, 0x3ca63433u,
    0x3cadd37du, 0x3cb5a602u, 0x3cbdac21u, 0x3cc5e63au, 0x3cce54acu, 0x3cd6f7d5u, 0x3cdfd010u, 0x3ce8ddbau,
    0x3cf2212du, 0x3cfb9ac3u, 0x3d02a56au, 0x3d0798ddu, 0x3d0ca7e6u, 0x3d11d2afu, 0x3d171964u, 0x3d1c7c30u,
    0x3d21fb3cu, 0x3d2796b2u, 0x3d2d4ebbu, 0x3d332381u, 0x3d39152bu, 0x3d3f23e4u, 0x3d454fd2u, 0x3d4b991du,
    0x3d51ffecu, 0x3d588468u, 0x3d5f26b6u, 0x3d65e6fdu, 0x3d6cc563u, 0x3d73c20eu, 0x3d7add24u, 0x3d810b65u,
    0x3d84b793u, 0x3d88732eu, 0x3d8c3e48u, 0x3d9018f4u, 0x3d940344u, 0x3d97fd49u, 0x3d9c0715u, 0x3da020bau,
    0x3da44a4au, 0x3da883d6u, 0x3daccd6fu, 0x3db12727u, 0x3db5910fu, 0x3dba0b38u, 0x3dbe95b3u, 0x3dc33090u,
    0x3dc7dbe0u, 0x3dcc97b4u, 0x3dd1641du, 0x3dd6412bu, 0x3ddb2eeeu, 0x3de02d76u, 0x3de53cd4u, 0x3dea5d18u,
    0x3def8e51u, 0x3df4d090u, 0x3dfa23e5u, 0x3dff885eu, 0x3e027f06u, 0x3e05427fu, 0x3e080ea2u, 0x3e0ae377u,
    0x3e0dc104u, 0x3e10a753u, 0x3e13966au, 0x3e168e51u, 0x3e198f0fu, 0x3e1c98acu, 0x3e1fab30u, 0x3e22c6a1u,
    0x3e25eb07u, 0x3e29186au, 0x3e2c4ed0u, 0x3e2f8e42u, 0x3e32d6c5u, 0x3e362862u, 0x3e39831fu, 0x3e3ce703u,
    0x3e405417u, 0x3e43ca60u, 0x3e4749e6u, 0x3e4ad2afu, 0x3e4e64c3u, 0x3e520029u, 0x3e55a4e7u, 0x3e595305u,
    0x3e5d0a89u, 0x3e60cb7au, 0x3e6495dfu, 0x3e6869beu, 0x3e6c471fu, 0x3e702e07u, 0x3e741e7eu, 0x3e78188bu,
    0x3e7c1c33u, 0x3e8014bfu, 0x3e822039u, 0x3e84308bu, 0x3e8645b8u, 0x3e885fc3u, 0x3e8a7eb0u, 0x3e8ca281u,
    0x3e8ecb3bu, 0x3e90f8dfu, 0x3e932b72u, 0x3e9562f6u, 0x3e979f6fu, 0x3e99e0e0u, 0x3e9c274cu, 0x3e9e72b6u,
    0x3ea0c321u, 0x3ea31890u, 0x3ea57307u, 0x3ea7d288u, 0x3eaa3716u, 0x3eaca0b6u, 0x3eaf0f68u, 0x3eb18332u,
    0x3eb3fc15u, 0x3eb67a14u, 0x3eb8fd34u, 0x3ebb8576u, 0x3ebe12deu, 0x3ec0a56eu, 0x3ec33d2au, 0x3ec5da14u,
    0x3ec87c30u, 0x3ecb2380u, 0x3ecdd008u, 0x3ed081cau, 0x3ed338c9u, 0x3ed5f508u, 0x3ed8b68au, 0x3edb7d52u,
    0x3ede4963u, 0x3ee11abfu, 0x3ee3f169u, 0x3ee6cd65u, 0x3ee9aeb5u, 0x3eec955bu, 0x3eef815cu, 0x3ef272b8u,
    0x3ef56974u, 0x3ef86593u, 0x3efb6716u, 0x3efe6e00u, 0x3f00bd2bu, 0x3f02460cu, 0x3f03d1a5u, 0x3f055ff7u,
    0x3f06f104u, 0x3f0884cdu, 0x3f0a1b54u, 0x3f0bb499u, 0x3f0d509fu, 0x3f0eef65u, 0x3f1090efu, 0x3f12353du,
    0x3f13dc50u, 0x3f15862au, 0x3f1732ccu, 0x3f18e237u, 0x3f1a946eu, 0x3f1c4970u, 0x3f1e0140u, 0x3f1fbbdeu,
    0x3f21794du, 0x3f23398cu, 0x3f24fc9fu, 0x3f26c285u, 0x3f288b41u, 0x3f2a56d2u, 0x3f2c253cu, 0x3f2df67fu,
    0x3f2fca9cu, 0x3f31a194u, 0x3f337b6au, 0x3f35581du, 0x3f3737b0u, 0x3f391a24u, 0x3f3aff7au, 0x3f3ce7b2u,
    0x3f3ed2cfu, 0x3f40c0d2u, 0x3f42b1bcu, 0x3f44a58eu, 0x3f469c49u, 0x3f4895efu, 0x3f4a9280u, 0x3f4c91ffu,
    0x3f4e946cu, 0x3f5099c9u, 0x3f52a216u, 0x3f54ad56u, 0x3f56bb88u, 0x3f58ccafu, 0x3f5ae0ccu, 0x3f5cf7dfu,
    0x3f5f11eau, 0x3f612eefu, 0x3f634eeeu, 0x3f6571e9u, 0x3f6797e0u, 0x3f69c0d5u, 0x3f6beccau, 0x3f6e1bbfu,
    0x3f704db5u, 0x3f7282aeu, 0x3f74baabu, 0x3f76f5aeu, 0x3f7933b6u, 0x3f7b74c6u, 0x3f7db8deu, 0x3f800000u,
};

TEX_DEV float tex_coord(float s, int wrap) {
    if (!(__builtin_fabsf(s) < __builtin_inff())) s = 0.0f;  // +-inf, NaN
    if (wrap == TEX_CLAMP) {
        const float x = s > 0.0f ? s : 0.0f;
        return x < 1.0f ? x : 1.0f;
    }
    return s - __builtin_floorf(s);
}
TEX_DEV int tex_index(int i, int n, int wrap) {
    if (wrap == TEX_CLAMP) {
        i = i < 0 ? 0 : i;
        i = i > n - 1 ? n - 1 : i;
    } else {
        i = i < 0 ? i + n : i;
        i = i >= n ? i - n : i;
    }
    return (unsigned)i < (unsigned)n ? i : n - 1;  // (the rule keeps every index inside already; this only guards the fetch)
}
// One axis: the two texel indices and the weight of the second (nearest: i1 = i0, f = 0)
TEX_DEV void tex_axis(float s, int n, int wrap, int filter, int &i0, int &i1, float &f) {
    const float a = tex_coord(s, wrap) * (float)n;
    if (filter == TEX_BILINEAR) {
        const float b = a - 0.5f;
        const float fl = __builtin_floorf(b);
        f = b - fl;
        const int i = (int)fl;
        i0 = tex_index(i, n, wrap);
        i1 = tex_index(i + 1, n, wrap);
    } else {
        i0 = i1 = tex_index((int)__builtin_floorf(a), n, wrap);
        f = 0.0f;
    }
}
TEX_DEV float3 tex_texel(const TexSet &ts, const TexDesc &d, int ix, int iy) {
    const size_t k = (size_t)iy * (size_t)d.width + (size_t)ix;
    const unsigned char *base = ts.texels + d.offset;
    if (d.format == TEX_RGBA32F) {
        const float4 v = *reinterpret_cast<const float4 *>(base + 16 * k);
        return make_float3(v.x, v.y, v.z);
    }
    const unsigned w = *reinterpret_cast<const unsigned *>(base + 4 * k);  // bytes r, g, b, a in memory order
    const unsigned r = w & 255u, g = (w >> 8) & 255u, b = (w >> 16) & 255u;
    if (d.format == TEX_RGBA8_SRGB) return make_float3(__uint_as_float(kSrgbBits[r]), __uint_as_float(kSrgbBits[g]), __uint_as_float(kSrgbBits[b]));
    return make_float3((float)r / 255.0f, (float)g / 255.0f, (float)b / 255.0f);
}
TEX_DEV float tex_mix(float fx, float fy, float t00, float t10, float t01, float t11) {
    const float c0 = t00 + fx * (t10 - t00);
    const float c1 = t01 + fx * (t11 - t01);
    return c0 + fy * (c1 - c0);
}

// The lookup.  index must lie in [0, set.n_tex): the callers' bindings are checked when a set is uploaded.
TEX_DEV float3 tex_lookup(const TexSet &ts, int index, float s, float t) {
    const TexDesc d = ts.desc[index];
    int x0, x1, y0, y1;
    float fx, fy;
    tex_axis(s, d.width, d.wrap_s, d.filter, x0, x1, fx);
    tex_axis(t, d.height, d.wrap_t, d.filter, y0, y1, fy);
    const float3 t00 = tex_texel(ts, d, x0, y0);
    if (d.filter != TEX_BILINEAR) return t00;
    const float3 t10 = tex_texel(ts, d, x1, y0), t01 = tex_texel(ts, d, x0, y1), t11 = tex_texel(ts, d, x1, y1);
    return make_float3(tex_mix(fx, fy, t00.x, t10.x, t01.x, t11.x), tex_mix(fx, fy, t00.y, t10.y, t01.y, t11.y), tex_mix(fx, fy, t00.z, t10.z, t01.z, t11.z));
}

// Texture coordinates at a hit (u, v) of device triangle `tri`: the order surf_tri mixes the normals in
TEX_DEV float2 tex_hit_st(const TexSet &ts, int tri, float u, float v) {
    const float2 a = ts.tri_st[3 * tri], b = ts.tri_st[3 * tri + 1], c = ts.tri_st[3 * tri + 2];
    const float w0 = (1.0f - u) - v;
    return make_float2((w0 * a.x + u * b.x) + v * c.x, (w0 * a.y + u * b.y) + v * c.y);
}

// One channel of the lookup (include/glrtx.h "Cutouts"): channels 0 to 2 are tex_lookup's x, y, z word for word; channel 3 is the texel's .w (RGBA32F) or
// byte / 255.0f (both 8-bit formats: alpha is never sRGB-decoded), filtered by the same tex_mix.  Fetches what the channel needs and no more: one 4-byte load a
// texel in every format (one dword of the RGBA32F texel, or the packed 8-bit texel).
TEX_DEV float tex_texel_channel(const TexSet &ts, const TexDesc &d, int channel, int ix, int iy) {
    const size_t k = (size_t)iy * (size_t)d.width + (size_t)ix;
    const unsigned char *base = ts.texels + d.offset;
    if (d.format == TEX_RGBA32F) return *reinterpret_cast<const float *>(base + 16 * k + 4 * (size_t)(unsigned)channel);
    const unsigned w = *reinterpret_cast<const unsigned *>(base + 4 * k);  // bytes r, g, b, a in memory order
    const unsigned b = (w >> (8u * (unsigned)channel)) & 255u;
    if (d.format == TEX_RGBA8_SRGB && channel < 3) return __uint_as_float(kSrgbBits[b]);
    return (float)b / 255.0f;
}
// index must lie in [0, set.n_tex), channel in 0 .. 3: the callers' records are checked when they are bound (glrtx_bind_cutouts).
TEX_DEV float tex_lookup_channel(const TexSet &ts, int index, int channel, float s, float t) {
    const TexDesc d = ts.desc[index];
    int x0, x1, y0, y1;
    float fx, fy;
    tex_axis(s, d.width, d.wrap_s, d.filter, x0, x1, fx);
    tex_axis(t, d.height, d.wrap_t, d.filter, y0, y1, fy);
    const float t00 = tex_texel_channel(ts, d, channel, x0, y0);
    if (d.filter != TEX_BILINEAR) return t00;
    const float t10 = tex_texel_channel(ts, d, channel, x1, y0), t01 = tex_texel_channel(ts, d, channel, x0, y1), t11 = tex_texel_channel(ts, d, channel, x1, y1);
    return tex_mix(fx, fy, t00, t10, t01, t11);
}

// Cutouts (include/glrtx.h "Cutouts"; glrtx_bind_cutouts).  == glrtx_cutout, 16 bytes: one record a material, texture -1: none.
struct CutRec {
    int texture, channel;
    float cutoff;
    int reserved;
};
// The bound records and tri_cut: the record index of every device triangle (tex_hit_st's index), -1 for a triangle whose material is not cut -- built when the
// records are bound, from the triangles' materials.  Passed to the CUT kernels behind their last argument; nothing else reads it.
struct CutSet {
    const int *tri_cut;
    const CutRec *rec;
};
// What the CUT traversal step takes: the launch's texture set and its cutout tables, both in the kernel's argument segment
struct CutRef {
    const TexSet *tex;
    const CutSet *cut;
};
// The rule, at a candidate hit (u, v) of device triangle `tri` that would become the ray's closest: accepted iff value >= cutoff (a NaN rejects).  One 4-byte
// gather for every candidate; only a cut triangle goes on to its record, tri_st and the texels.
TEX_DEV bool cut_accepts(const CutRef &cr, int tri, float u, float v) {
    const int k = cr.cut->tri_cut[tri];
    if (k < 0) return true;
    const CutRec r = cr.cut->rec[k];
    const float2 st = tex_hit_st(*cr.tex, tri, u, v);
    return tex_lookup_channel(*cr.tex, r.texture, r.channel, st.x, st.y) >= r.cutoff;
}

// Emission maps (include/glrtx.h "Emission maps"; glrtx_bind_emission_maps).  mat_emit: texture index a material, -1 unbound.  light_st: three {s, t} a light
// (the uv words of the light's three vertices in wire order), frozen when the maps are bound.  Passed to the EMIT kernels behind their last argument, and
// to the textured feature kernels while emission maps are bound; nothing else reads it.
struct EmitSet {
    const int *mat_emit;
    const float2 *light_st;
};
// The sample (ua, ub) -- after the flip -- of light `lid`: the order sampleDirect mixes the light's vertices in
TEX_DEV float2 emit_light_st(const EmitSet &es, int lid, float ua, float ub) {
    const float2 a = es.light_st[3 * lid], b = es.light_st[3 * lid + 1], c = es.light_st[3 * lid + 2];
    const float w0 = (1.0f - ua) - ub;
    return make_float2((w0 * a.x + ua * b.x) + ub * c.x, (w0 * a.y + ua * b.y) + ub * c.y);
}
// Le = emission * c, per channel: one rounded product
TEX_DEV float3 emit_radiance(const TexSet &ts, int index, float s, float t, float ex, float ey, float ez) {
    const float3 c = tex_lookup(ts, index, s, t);
    return make_float3(ex * c.x, ey * c.y, ez * c.z);
}

// glrtx_debug_light_emission: out[5i..] = {s, t, Le.rgb} of light lid[i] at the raw uniforms u[2i..] (the flip is taken here, as sampleDirect takes it).
// lights: six float4 a light, {v0, material} first; mats: three float4 a material, {emission, type} first.
__global__ __launch_bounds__(256) void emit_light_kernel(const TexSet ts, const EmitSet es, const float4 *lights, const float4 *mats, const int *lid, const float *u,
                                                         unsigned n, float *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float ua0 = u[2 * i], ub0 = u[2 * i + 1];
    const bool flip = 1.0f < ua0 + ub0;
    const float ua = flip ? 1.0f - ua0 : ua0;
    const float ub = flip ? 1.0f - ub0 : ub0;
    const int l = lid[i];
    const int m = __float_as_int(lights[6 * l].w);
    const float4 m0 = mats[3 * m];
    const float2 st = emit_light_st(es, l, ua, ub);
    const int k = es.mat_emit[m];
    float3 le = make_float3(m0.x, m0.y, m0.z);
    if (k >= 0) le = emit_radiance(ts, k, st.x, st.y, m0.x, m0.y, m0.z);
    out[5 * i] = st.x; out[5 * i + 1] = st.y; out[5 * i + 2] = le.x; out[5 * i + 3] = le.y; out[5 * i + 4] = le.z;
}

// glrtx_debug_texture_channel: out[i] = tex_lookup_channel(which[i], channel[i], st[2i], st[2i + 1])
__global__ __launch_bounds__(256) void tex_channel_kernel(const TexSet ts, const int *which, const int *channel, const float *st, unsigned n, float *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    out[i] = tex_lookup_channel(ts, which[i], channel[i], st[2 * i], st[2 * i + 1]);
}

// glrtx_debug_texture_lookup: out[3i..] = tex_lookup(which[i], st[2i], st[2i + 1])
__global__ __launch_bounds__(256) void tex_lookup_kernel(const TexSet ts, const int *which, const float *st, unsigned n, float *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float3 c = tex_lookup(ts, which[i], st[2 * i], st[2 * i + 1]);
    out[3 * i] = c.x; out[3 * i + 1] = c.y; out[3 * i + 2] = c.z;
}

}  // namespace glrtx
