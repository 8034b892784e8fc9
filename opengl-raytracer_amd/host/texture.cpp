// texture.cpp -- glrt_texture_lookup / glrt_srgb_table / glrt_texture_albedo (include/glrt_host.h): the CPU statement of the device's texture lookup
// (include/glrtx.h "Textures"; csrc/texture.hip.h), bit for bit.  Compiled with -ffp-contract=off and run under MXCSR FTZ | DAZ like the other statements:
// every operation is one rounded fp32 operation in the order the header writes it.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "emission_statement.h"
#include "glrt_host.h"
#include "statement_math.h"
#include "texture_set.h"
#include "texture_statement.h"

namespace {

using glrt_detail::bits_f;
using glrt_detail::FlushDenormals;
using glrt_detail::TexRecord;

static_assert(sizeof(glrt_texture) == sizeof(TexRecord), "glrt_texture is the wire descriptor");

// sRGB byte -> linear: the piecewise formula in float64, rounded once to fp32 (bit patterns; tests/test_texture_host.py recomputes them)
const uint32_t kSrgbBits[256] = {
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

float coord(float s, int wrap) {
    if (!(std::fabs(s) < INFINITY)) s = 0.0f;  // +-inf, NaN
    if (glrt_detail::tiny(s)) s = std::copysign(0.0f, s);  // (a denormal coordinate is a zero for the device's floor; libm's floorf does not look at MXCSR)
    if (wrap == GLRT_TEX_CLAMP) {
        const float x = s > 0.0f ? s : 0.0f;
        return x < 1.0f ? x : 1.0f;
    }
    return s - std::floor(s);
}
int index_of(int i, int n, int wrap) {
    if (wrap == GLRT_TEX_CLAMP) {
        i = i < 0 ? 0 : i;
        i = i > n - 1 ? n - 1 : i;
    } else {
        i = i < 0 ? i + n : i;
        i = i >= n ? i - n : i;
    }
    return (unsigned)i < (unsigned)n ? i : n - 1;
}
void axis(float s, int n, int wrap, int filter, int &i0, int &i1, float &f) {
    const float a = coord(s, wrap) * (float)n;
    if (filter == GLRT_TEX_BILINEAR) {
        const float b = a - 0.5f;
        const float fl = std::floor(b);
        f = b - fl;
        const int i = (int)fl;
        i0 = index_of(i, n, wrap);
        i1 = index_of(i + 1, n, wrap);
    } else {
        i0 = i1 = index_of((int)std::floor(a), n, wrap);
        f = 0.0f;
    }
}
void texel(const TexRecord &d, const unsigned char *texels, int ix, int iy, float rgb[3]) {
    const size_t k = (size_t)iy * (size_t)d.width + (size_t)ix;
    const unsigned char *p = texels + d.offset;
    if (d.format == GLRT_TEX_RGBA32F) { std::memcpy(rgb, p + 16 * k, 12); return; }
    for (int c = 0; c < 3; c++) {
        const unsigned b = p[4 * k + c];
        rgb[c] = d.format == GLRT_TEX_RGBA8_SRGB ? bits_f(kSrgbBits[b]) : (float)b / 255.0f;
    }
}
float mix(float fx, float fy, float t00, float t10, float t01, float t11) {
    const float c0 = t00 + fx * (t10 - t00);
    const float c1 = t01 + fx * (t11 - t01);
    return c0 + fy * (c1 - c0);
}
void lookup(const TexRecord &d, const unsigned char *texels, float s, float t, float rgb[3]) {
    int x0, x1, y0, y1;
    float fx, fy;
    axis(s, d.width, d.wrap_s, d.filter, x0, x1, fx);
    axis(t, d.height, d.wrap_t, d.filter, y0, y1, fy);
    float t00[3], t10[3], t01[3], t11[3];
    texel(d, texels, x0, y0, t00);
    if (d.filter != GLRT_TEX_BILINEAR) { std::memcpy(rgb, t00, 12); return; }
    texel(d, texels, x1, y0, t10); texel(d, texels, x0, y1, t01); texel(d, texels, x1, y1, t11);
    for (int c = 0; c < 3; c++) rgb[c] = mix(fx, fy, t00[c], t10[c], t01[c], t11[c]);
}

// One channel (include/glrtx.h "Cutouts"): 0 .. 2 are lookup()'s words; 3 is the texel's fourth float, or byte / 255.0f for both 8-bit formats
float texel_channel(const TexRecord &d, const unsigned char *texels, int channel, int ix, int iy) {
    const size_t k = (size_t)iy * (size_t)d.width + (size_t)ix;
    const unsigned char *p = texels + d.offset;
    if (d.format == GLRT_TEX_RGBA32F) {
        float f;
        std::memcpy(&f, p + 16 * k + 4 * (size_t)channel, 4);
        return f;
    }
    const unsigned b = p[4 * k + (size_t)channel];
    return d.format == GLRT_TEX_RGBA8_SRGB && channel < 3 ? bits_f(kSrgbBits[b]) : (float)b / 255.0f;
}
float lookup_channel(const TexRecord &d, const unsigned char *texels, int channel, float s, float t) {
    int x0, x1, y0, y1;
    float fx, fy;
    axis(s, d.width, d.wrap_s, d.filter, x0, x1, fx);
    axis(t, d.height, d.wrap_t, d.filter, y0, y1, fy);
    const float t00 = texel_channel(d, texels, channel, x0, y0);
    if (d.filter != GLRT_TEX_BILINEAR) return t00;
    return mix(fx, fy, t00, texel_channel(d, texels, channel, x1, y0), texel_channel(d, texels, channel, x0, y1), texel_channel(d, texels, channel, x1, y1));
}

}  // namespace

float glrt_detail::texture_channel_one(const TexRecord &d, const unsigned char *texels, int channel, float s, float t) { return lookup_channel(d, texels, channel, s, t); }

int glrt_texture_channel(const glrt_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const int32_t *channel, const float *st,
                         size_t n, float *value_out) {
    if (n && (!which || !channel || !st || !value_out)) return GLRT_HOST_EINVAL;
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(tex);
    if (!glrt_detail::texture_set_error(rec, n_tex, texels, texel_bytes).empty()) return GLRT_HOST_EINVAL;
    for (size_t i = 0; i < n; i++)
        if (which[i] < 0 || (size_t)which[i] >= n_tex || channel[i] < 0 || channel[i] > 3) return GLRT_HOST_EINDEX;
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++) value_out[i] = lookup_channel(rec[which[i]], (const unsigned char *)texels, channel[i], st[2 * i], st[2 * i + 1]);
    return GLRT_HOST_OK;
}

// (texture_statement.h: the same statement for host/environment.cpp)
void glrt_detail::texture_lookup_one(const TexRecord &d, const unsigned char *texels, float s, float t, float rgb[3]) { lookup(d, texels, s, t, rgb); }
void glrt_detail::texture_texel_one(const TexRecord &d, const unsigned char *texels, int ix, int iy, float rgb[3]) { texel(d, texels, ix, iy, rgb); }

const float *glrt_srgb_table(void) {
    static float table[256];
    static const bool once = [] { std::memcpy(table, kSrgbBits, sizeof table); return true; }();
    (void)once;
    return table;
}

int glrt_texture_lookup(const glrt_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const float *st, size_t n,
                        float *rgb_out) {
    if (n && (!which || !st || !rgb_out)) return GLRT_HOST_EINVAL;
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(tex);
    if (!glrt_detail::texture_set_error(rec, n_tex, texels, texel_bytes).empty()) return GLRT_HOST_EINVAL;
    for (size_t i = 0; i < n; i++)
        if (which[i] < 0 || (size_t)which[i] >= n_tex) return GLRT_HOST_EINDEX;
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++) lookup(rec[which[i]], (const unsigned char *)texels, st[2 * i], st[2 * i + 1], rgb_out + 3 * i);
    return GLRT_HOST_OK;
}

int glrt_texture_albedo(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat, const glrt_texture *tex, size_t n_tex,
                        const void *texels, size_t texel_bytes, const int32_t *material_texture, const float *hits, size_t n, float *rgb_out) {
    if (n && (!hits || !rgb_out)) return GLRT_HOST_EINVAL;
    if ((n_tri && (!vert || !tri || !mat)) || (n_mat && !material_texture)) return GLRT_HOST_EINVAL;
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(tex);
    if (!glrt_detail::texture_set_error(rec, n_tex, texels, texel_bytes).empty()) return GLRT_HOST_EINVAL;
    for (size_t m = 0; m < n_mat; m++)
        if (material_texture[m] >= 0 && ((size_t)material_texture[m] >= n_tex || (int)mat[GLRT_MATERIAL_FLOATS * m] != 2)) return GLRT_HOST_EINDEX;
    for (size_t t = 0; t < n_tri; t++) {
        for (int k = 0; k < 3; k++)
            if (!(tri[4 * t + k] >= 0.0f) || (size_t)tri[4 * t + k] >= n_vert) return GLRT_HOST_EINDEX;
        if (!(tri[4 * t + 3] >= 0.0f) || (size_t)tri[4 * t + 3] >= n_mat) return GLRT_HOST_EINDEX;
    }
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++) {
        const float *h = hits + 4 * i;
        float *A = rgb_out + 3 * i;
        int32_t t;
        std::memcpy(&t, &h[0], 4);
        A[0] = A[1] = A[2] = 1.0f;
        if (t < 0) continue;
        if ((size_t)t >= n_tri) return GLRT_HOST_EINDEX;
        const float *tr = tri + 4 * (size_t)t;
        const size_t id = (size_t)tr[3];
        const float *m = mat + GLRT_MATERIAL_FLOATS * id;
        if ((int)m[0] != 2) continue;
        if (material_texture[id] < 0) { A[0] = m[6]; A[1] = m[7]; A[2] = m[8]; continue; }
        const float *a = vert + GLRT_VERTEX_FLOATS * (size_t)tr[0] + 6, *b = vert + GLRT_VERTEX_FLOATS * (size_t)tr[1] + 6,
                    *c = vert + GLRT_VERTEX_FLOATS * (size_t)tr[2] + 6;
        const float u = h[1], v = h[2];
        const float w0 = (1.0f - u) - v;
        const float s = (w0 * a[0] + u * b[0]) + v * c[0];
        const float q = (w0 * a[1] + u * b[1]) + v * c[1];
        lookup(rec[material_texture[id]], (const unsigned char *)texels, s, q, A);
    }
    return GLRT_HOST_OK;
}

// ---- emission maps (include/glrtx.h "Emission maps"): the CPU statements of the sampled-side rule and of the feature pass's plane A

int glrt_light_st(const float *vert, size_t n_vert, const float *light, size_t n_light, float *st_out) {
    if (n_light && (!vert || !light || !st_out)) return GLRT_HOST_EINVAL;
    for (size_t l = 0; l < n_light; l++)
        for (int j = 0; j < 3; j++) {
            const float i = light[4 * l + j];
            if (!(i >= 0.0f) || (size_t)i >= n_vert) return GLRT_HOST_EINDEX;
            const float *v = vert + GLRT_VERTEX_FLOATS * (size_t)i;
            st_out[6 * l + 2 * j] = v[6];
            st_out[6 * l + 2 * j + 1] = v[7];
        }
    return GLRT_HOST_OK;
}

int glrt_emission_bind_check(const float *mat, size_t n_scene_mat, size_t n_tex, int cutouts_bound, const int32_t *material_emission, size_t n_mat, char *msg, size_t cap) {
    if ((n_scene_mat && !mat) || (n_mat && !material_emission)) return GLRT_HOST_EINVAL;
    const std::string bad = glrt_detail::emission_bind_error(true, n_scene_mat, n_tex, cutouts_bound != 0, material_emission, n_mat,
                                                             [&](size_t m) { return (int)mat[GLRT_MATERIAL_FLOATS * m]; });
    if (msg && cap) std::snprintf(msg, cap, "%s", bad.c_str());
    return bad.empty() ? GLRT_HOST_OK : GLRT_HOST_EINVAL;
}

int glrt_light_emission(const float *vert, size_t n_vert, const float *light, size_t n_light, const float *mat, size_t n_mat, const glrt_texture *tex, size_t n_tex,
                        const void *texels, size_t texel_bytes, const int32_t *material_emission, const int32_t *lid, const float *u, size_t n, float *out) {
    if (n && (!lid || !u || !out)) return GLRT_HOST_EINVAL;
    if ((n_light && (!vert || !light || !mat)) || (n_mat && !material_emission)) return GLRT_HOST_EINVAL;
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(tex);
    if (!glrt_detail::texture_set_error(rec, n_tex, texels, texel_bytes).empty()) return GLRT_HOST_EINVAL;
    for (size_t m = 0; m < n_mat; m++)
        if (material_emission[m] < -1 || (material_emission[m] >= 0 && ((size_t)material_emission[m] >= n_tex || (int)mat[GLRT_MATERIAL_FLOATS * m] == 5))) return GLRT_HOST_EINDEX;
    std::vector<float> st(6 * n_light);
    if (const int rc = glrt_light_st(vert, n_vert, light, n_light, st.data())) return rc;
    for (size_t l = 0; l < n_light; l++)
        if (!(light[4 * l + 3] >= 0.0f) || (size_t)light[4 * l + 3] >= n_mat) return GLRT_HOST_EINDEX;
    for (size_t i = 0; i < n; i++)
        if (lid[i] < 0 || (size_t)lid[i] >= n_light) return GLRT_HOST_EINDEX;
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++) {
        const float ua0 = u[2 * i], ub0 = u[2 * i + 1];
        const bool flip = 1.0f < ua0 + ub0;  // sampleDirect's flip
        const float ua = flip ? 1.0f - ua0 : ua0;
        const float ub = flip ? 1.0f - ub0 : ub0;
        const float w0 = (1.0f - ua) - ub;
        const float *q = &st[6 * (size_t)lid[i]];
        const float s = (w0 * q[0] + ua * q[2]) + ub * q[4];
        const float t = (w0 * q[1] + ua * q[3]) + ub * q[5];
        const size_t id = (size_t)light[4 * (size_t)lid[i] + 3];
        const float *m = mat + GLRT_MATERIAL_FLOATS * id;
        float *o = out + 5 * i;
        o[0] = s; o[1] = t;
        o[2] = m[3]; o[3] = m[4]; o[4] = m[5];  // an unbound light: its plain emission
        if (material_emission[id] >= 0) {
            float c[3];
            lookup(rec[material_emission[id]], (const unsigned char *)texels, s, t, c);
            o[2] = m[3] * c[0]; o[3] = m[4] * c[1]; o[4] = m[5] * c[2];  // Le = emission * c: one rounded product a channel
        }
    }
    return GLRT_HOST_OK;
}

int glrt_emission_albedo(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat, const glrt_texture *tex, size_t n_tex,
                         const void *texels, size_t texel_bytes, const int32_t *material_texture, const int32_t *material_emission, const float *hits, size_t n,
                         float *rgb_out) {
    if (n_mat && !material_emission) return GLRT_HOST_EINVAL;
    if (const int rc = glrt_texture_albedo(vert, n_vert, tri, n_tri, mat, n_mat, tex, n_tex, texels, texel_bytes, material_texture, hits, n, rgb_out)) return rc;
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(tex);
    for (size_t m = 0; m < n_mat; m++)
        if (material_emission[m] < -1 || (material_emission[m] >= 0 && ((size_t)material_emission[m] >= n_tex || (int)mat[GLRT_MATERIAL_FLOATS * m] == 5))) return GLRT_HOST_EINDEX;
    FlushDenormals ftz;
    for (size_t i = 0; i < n; i++) {
        const float *h = hits + 4 * i;
        int32_t t;
        std::memcpy(&t, &h[0], 4);
        if (t < 0) continue;
        const float *tr = tri + 4 * (size_t)t;
        const size_t id = (size_t)tr[3];
        if ((int)mat[GLRT_MATERIAL_FLOATS * id] == 2 || material_emission[id] < 0) continue;  // a diffuse material keeps its albedo rule
        const float *a = vert + GLRT_VERTEX_FLOATS * (size_t)tr[0] + 6, *b = vert + GLRT_VERTEX_FLOATS * (size_t)tr[1] + 6,
                    *c = vert + GLRT_VERTEX_FLOATS * (size_t)tr[2] + 6;
        const float u = h[1], v = h[2];
        const float w0 = (1.0f - u) - v;
        lookup(rec[material_emission[id]], (const unsigned char *)texels, (w0 * a[0] + u * b[0]) + v * c[0], (w0 * a[1] + u * b[1]) + v * c[1], rgb_out + 3 * i);
    }
    return GLRT_HOST_OK;
}

// ---- surface context (include/glrt_host.h "Surface context"): the three lookups above as per-hit calls, for a path tracer that takes them as callbacks.
// The context owns copies of everything it reads: the {s, t} of every wire triangle's and every light's corners as they were when it was made, the triangles'
// and lights' materials, the checked set and the three kinds of per-material bindings.  The calls only read it, so any number of threads may share one.
struct glrt_surface {
    std::vector<TexRecord> tex;
    std::vector<unsigned char> texels;
    std::vector<float> tri_st, light_st;      // six floats a triangle / a light: {s0, t0, s1, t1, s2, t2}
    std::vector<int32_t> tri_mat, light_mat;  // the material of every triangle / light
    std::vector<int32_t> albedo, emission;    // one texture index a material, -1 none
    std::vector<glrt_cutout> cut;             // one record a material, texture -1: none
};

namespace {
// (s, t) at (u, v) of corner coordinates q: the order glrt_texture_albedo and glrt_light_emission mix them in
inline void mix_st(const float *q, float u, float v, float &s, float &t) {
    const float w0 = (1.0f - u) - v;
    s = (w0 * q[0] + u * q[2]) + v * q[4];
    t = (w0 * q[1] + u * q[3]) + v * q[5];
}
}  // namespace

int glrt_surface_create(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *light, size_t n_light, const float *mat, size_t n_mat,
                        const glrt_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *material_texture, const glrt_cutout *cut,
                        const int32_t *material_emission, glrt_surface **surface_out) {
    if (!surface_out) return GLRT_HOST_EINVAL;
    *surface_out = nullptr;
    if ((n_tri && (!vert || !tri)) || (n_light && (!vert || !light)) || (n_mat && !mat)) return GLRT_HOST_EINVAL;
    if (n_tri >= (size_t)INT32_MAX || n_light >= (size_t)INT32_MAX || n_mat >= (size_t)INT32_MAX) return GLRT_HOST_EINVAL;
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(tex);
    if (!glrt_detail::texture_set_error(rec, n_tex, texels, texel_bytes).empty()) return GLRT_HOST_EINVAL;
    for (size_t m = 0; m < n_mat; m++) {  // what glrtx_upload_textures, glrtx_bind_cutouts and glrtx_bind_emission_maps refuse of a material
        const int type = (int)mat[GLRT_MATERIAL_FLOATS * m];
        if (material_texture && (material_texture[m] < -1 || (material_texture[m] >= 0 && ((size_t)material_texture[m] >= n_tex || type != 2)))) return GLRT_HOST_EINDEX;
        if (material_emission && (material_emission[m] < -1 || (material_emission[m] >= 0 && ((size_t)material_emission[m] >= n_tex || type == 5)))) return GLRT_HOST_EINDEX;
        if (cut) {
            const glrt_cutout &r = cut[m];
            if (r.texture < -1 || (r.texture >= 0 && (size_t)r.texture >= n_tex) || r.channel < 0 || r.channel > 3) return GLRT_HOST_EINDEX;
            if (!std::isfinite(r.cutoff) || r.reserved != 0 || (r.texture >= 0 && type != 2 && type != 3)) return GLRT_HOST_EINVAL;
        }
    }
    glrt_surface *s = new glrt_surface;
    const auto corners = [&](const float *records, size_t n, std::vector<float> &st, std::vector<int32_t> &material) {
        st.assign(6 * n, 0.0f);
        material.assign(n, 0);
        for (size_t t = 0; t < n; t++) {
            const float *r = records + 4 * t;
            for (int k = 0; k < 3; k++) {
                if (!(r[k] >= 0.0f) || (size_t)r[k] >= n_vert) return false;
                const float *v = vert + GLRT_VERTEX_FLOATS * (size_t)r[k];
                st[6 * t + 2 * k] = v[6];
                st[6 * t + 2 * k + 1] = v[7];
            }
            if (!(r[3] >= 0.0f) || (size_t)r[3] >= n_mat) return false;
            material[t] = (int32_t)r[3];
        }
        return true;
    };
    if (!corners(tri, n_tri, s->tri_st, s->tri_mat) || !corners(light, n_light, s->light_st, s->light_mat)) { delete s; return GLRT_HOST_EINDEX; }
    s->tex.assign(rec, rec + n_tex);
    s->texels.assign((const unsigned char *)texels, (const unsigned char *)texels + (n_tex ? texel_bytes : 0));
    s->albedo.assign(n_mat, -1);
    s->emission.assign(n_mat, -1);
    s->cut.assign(n_mat, glrt_cutout{-1, 3, 0.5f, 0});
    if (material_texture) s->albedo.assign(material_texture, material_texture + n_mat);
    if (material_emission) s->emission.assign(material_emission, material_emission + n_mat);
    if (cut) s->cut.assign(cut, cut + n_mat);
    *surface_out = s;
    return GLRT_HOST_OK;
}

void glrt_surface_free(glrt_surface *surface) { delete surface; }

int glrt_surface_albedo(void *surface, int tri, float u, float v, float rgb[3]) {
    const glrt_surface &c = *static_cast<const glrt_surface *>(surface);
    if (tri < 0 || (size_t)tri >= c.tri_mat.size()) return 0;
    const int32_t k = c.albedo[(size_t)c.tri_mat[(size_t)tri]];
    if (k < 0) return 0;
    FlushDenormals ftz;
    float s, t;
    mix_st(&c.tri_st[6 * (size_t)tri], u, v, s, t);
    lookup(c.tex[(size_t)k], c.texels.data(), s, t, rgb);
    return 1;
}

int glrt_surface_accept(void *surface, int tri, float u, float v) {
    const glrt_surface &c = *static_cast<const glrt_surface *>(surface);
    if (tri < 0 || (size_t)tri >= c.tri_mat.size()) return 1;
    const glrt_cutout &r = c.cut[(size_t)c.tri_mat[(size_t)tri]];
    if (r.texture < 0) return 1;
    FlushDenormals ftz;
    float s, t;
    mix_st(&c.tri_st[6 * (size_t)tri], u, v, s, t);
    return lookup_channel(c.tex[(size_t)r.texture], c.texels.data(), r.channel, s, t) >= r.cutoff ? 1 : 0;  // (a NaN rejects)
}

int glrt_surface_emission(void *surface, int index, int light, float u, float v, float texel[3]) {
    const glrt_surface &c = *static_cast<const glrt_surface *>(surface);
    const std::vector<int32_t> &material = light ? c.light_mat : c.tri_mat;
    if (index < 0 || (size_t)index >= material.size()) return 0;
    const int32_t k = c.emission[(size_t)material[(size_t)index]];
    if (k < 0) return 0;
    FlushDenormals ftz;
    float s, t;
    mix_st(&(light ? c.light_st : c.tri_st)[6 * (size_t)index], u, v, s, t);
    lookup(c.tex[(size_t)k], c.texels.data(), s, t, texel);
    return 1;
}
