// emission_sanitize.cpp -- a stand-alone program that runs the host statements of the emission maps (glrt_light_st, glrt_light_emission,
// glrt_emission_albedo, glrt_emission_bind_check; host/texture.cpp) over hostile textures, coordinates, uniforms and bindings.  tests/test_emission_host.py
// compiles it together with that file under -fsanitize=address,undefined and runs it: every buffer is exactly as large as the header says.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glrt_host.h"

namespace {

int failures = 0;
void check(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

const float inf = std::numeric_limits<float>::infinity(), qnan = std::numeric_limits<float>::quiet_NaN(), den = 1e-40f;

}  // namespace

int main() {
    // two light triangles on two emitter materials, one diffuse triangle; hostile coordinates on the second light
    const float hostile[] = {qnan, inf, -inf, den, -den, 0.0f, -0.0f, 0.5f, 1.0f};
    std::vector<float> vert(9 * GLRT_VERTEX_FLOATS, 0.0f);
    for (int v = 0; v < 9; v++) {
        float *p = &vert[(size_t)v * GLRT_VERTEX_FLOATS];
        p[0] = (float)(v % 3); p[1] = (float)(v / 3); p[2] = (float)(v % 2);
        p[4] = 1.0f;
        p[6] = v < 3 ? 0.25f * (float)v : hostile[v];
        p[7] = v < 3 ? 1.0f - 0.5f * (float)v : hostile[8 - v];
    }
    const std::vector<float> tri = {0, 1, 2, 0, 3, 4, 5, 1, 6, 7, 8, 2};
    const std::vector<float> light = {0, 1, 2, 0, 3, 4, 5, 1};
    std::vector<float> mat(3 * GLRT_MATERIAL_FLOATS, 0.0f);
    for (int m = 0; m < 3; m++) {
        float *p = &mat[(size_t)m * GLRT_MATERIAL_FLOATS];
        p[0] = p[1] = p[2] = m < 2 ? 1.0f : 2.0f;
        p[3] = 3.0f + (float)m; p[4] = m == 1 ? inf : 2.0f; p[5] = 0.5f;
        p[6] = p[7] = p[8] = 0.5f;
    }
    // the set: a 1 x 1 RGBA32F texel, a 3 x 2 sRGB bilinear texture, a 2 x 2 RGBA32F texture of hostile floats
    std::vector<unsigned char> blob;
    std::vector<glrt_texture> tex;
    const auto add = [&](int w, int h, int format, int wrap, int filter, int kind) {
        blob.resize((blob.size() + 15) / 16 * 16, 0);
        tex.push_back(glrt_texture{(uint64_t)blob.size(), w, h, format, wrap, 1 - wrap, filter});
        const size_t texel = format == GLRT_TEX_RGBA32F ? 16 : 4, at = blob.size();
        blob.resize(at + (size_t)w * h * texel, 0);
        for (size_t k = 0; k < (size_t)w * h * 4; k++) {
            if (format == GLRT_TEX_RGBA32F) {
                const float v = kind ? hostile[k % 9] : 0.75f;
                std::memcpy(&blob[at + 4 * k], &v, 4);
            } else {
                blob[at + k] = (unsigned char)(37 * k + 11);
            }
        }
    };
    add(1, 1, GLRT_TEX_RGBA32F, GLRT_TEX_CLAMP, GLRT_TEX_BILINEAR, 0);
    add(3, 2, GLRT_TEX_RGBA8_SRGB, GLRT_TEX_REPEAT, GLRT_TEX_BILINEAR, 0);
    add(2, 2, GLRT_TEX_RGBA32F, GLRT_TEX_REPEAT, GLRT_TEX_NEAREST, 1);

    std::vector<float> st(12);
    check(glrt_light_st(vert.data(), 9, light.data(), 2, st.data()) == GLRT_HOST_OK, "glrt_light_st");
    check(st[0] == 0.0f && st[2] == 0.25f && st[4] == 0.5f && st[1] == 1.0f, "glrt_light_st: the first light's words");
    const std::vector<float> bad_light = {0, 1, 9, 0};
    check(glrt_light_st(vert.data(), 9, bad_light.data(), 1, st.data()) == GLRT_HOST_EINDEX, "glrt_light_st: a vertex out of range");

    const float us[] = {0.0f, 0.25f, 0.5f, 0.75f, 0.99999994f, 1.0f, qnan, inf, -1.0f, den};
    std::vector<int32_t> lid;
    std::vector<float> u;
    for (int l = 0; l < 2; l++)
        for (float a : us)
            for (float b : us) { lid.push_back(l); u.push_back(a); u.push_back(b); }
    std::vector<float> out(5 * lid.size());
    for (int k0 = -1; k0 < 3; k0++)
        for (int k1 = -1; k1 < 3; k1++) {
            const int32_t bind[3] = {k0, k1, -1};
            check(glrt_light_emission(vert.data(), 9, light.data(), 2, mat.data(), 3, tex.data(), tex.size(), blob.data(), blob.size(), bind, lid.data(), u.data(),
                                      lid.size(), out.data()) == GLRT_HOST_OK, "glrt_light_emission");
            if (k0 == 0) check(out[2] == 3.0f * 0.75f && out[3] == 2.0f * 0.75f && out[4] == 0.5f * 0.75f, "Le on the 1 x 1 texture");
            if (k0 == -1) check(out[2] == 3.0f && out[3] == 2.0f && out[4] == 0.5f, "an unbound light: the plain emission");
        }
    {
        const int32_t bind[3] = {3, -1, -1};
        check(glrt_light_emission(vert.data(), 9, light.data(), 2, mat.data(), 3, tex.data(), tex.size(), blob.data(), blob.size(), bind, lid.data(), u.data(), lid.size(),
                                  out.data()) == GLRT_HOST_EINDEX, "a texture index out of range");
        const int32_t ok[3] = {0, 1, 2}, two = 2;
        check(glrt_light_emission(vert.data(), 9, light.data(), 2, mat.data(), 3, tex.data(), tex.size(), blob.data(), blob.size(), ok, &two, u.data(), 1, out.data()) ==
                  GLRT_HOST_EINDEX, "a light out of range");
        check(glrt_light_emission(vert.data(), 9, light.data(), 2, mat.data(), 3, tex.data(), tex.size(), blob.data(), blob.size(), ok, nullptr, nullptr, 0, nullptr) ==
                  GLRT_HOST_OK, "no samples");
    }

    // plane A: hits on every triangle at hostile (u, v), a miss, and a triangle out of range
    std::vector<float> hits;
    for (int t = -1; t < 3; t++)
        for (float a : us) {
            const int32_t id = t;
            float w;
            std::memcpy(&w, &id, 4);
            hits.insert(hits.end(), {w, a, 0.25f, 0.0f});
        }
    std::vector<float> rgb(3 * hits.size() / 4);
    const int32_t alb[3] = {-1, -1, 1}, emi[3] = {2, 0, 1};
    check(glrt_emission_albedo(vert.data(), 9, tri.data(), 3, mat.data(), 3, tex.data(), tex.size(), blob.data(), blob.size(), alb, emi, hits.data(), hits.size() / 4,
                               rgb.data()) == GLRT_HOST_OK, "glrt_emission_albedo");
    check(rgb[0] == 1.0f && rgb[1] == 1.0f && rgb[2] == 1.0f, "a miss keeps plane A's (1, 1, 1)");
    check(rgb[3 * (2 * 10) + 0] == 0.75f, "a bound emitter's hit carries the texel");
    {
        const int32_t id = 3;
        float w;
        std::memcpy(&w, &id, 4);
        const float far_hit[4] = {w, 0.1f, 0.1f, 0.0f};
        check(glrt_emission_albedo(vert.data(), 9, tri.data(), 3, mat.data(), 3, tex.data(), tex.size(), blob.data(), blob.size(), alb, emi, far_hit, 1, rgb.data()) ==
                  GLRT_HOST_EINDEX, "a hit on a triangle out of range");
    }

    // the validator: every refusal, into a message buffer that is exactly as large as it says -- and one that is too small
    char msg[256], tiny[8];
    const int32_t good[3] = {0, -1, 2};
    check(glrt_emission_bind_check(mat.data(), 3, 3, 0, good, 3, msg, sizeof msg) == GLRT_HOST_OK && msg[0] == 0, "the validator accepts");
    check(glrt_emission_bind_check(mat.data(), 3, 0, 0, good, 3, msg, sizeof msg) == GLRT_HOST_EINVAL && std::strstr(msg, "no texture set"), "no set");
    check(glrt_emission_bind_check(mat.data(), 3, 3, 0, good, 2, msg, sizeof msg) == GLRT_HOST_EINVAL && std::strstr(msg, "2 bindings, the scene has 3"), "the count");
    check(glrt_emission_bind_check(mat.data(), 3, 2, 0, good, 3, msg, sizeof msg) == GLRT_HOST_EINVAL && std::strstr(msg, "material 2: emission map 2 of 2"), "the range");
    check(glrt_emission_bind_check(mat.data(), 3, 3, 1, good, 3, tiny, sizeof tiny) == GLRT_HOST_EINVAL && std::strlen(tiny) == 7, "a small message buffer");
    mat[2 * GLRT_MATERIAL_FLOATS] = 5.0f;
    check(glrt_emission_bind_check(mat.data(), 3, 3, 0, good, 3, msg, sizeof msg) == GLRT_HOST_EINVAL && std::strstr(msg, "is a medium"), "a bound medium");
    check(glrt_emission_bind_check(mat.data(), 3, 3, 0, good, 3, nullptr, 0) == GLRT_HOST_EINVAL, "no message buffer");

    if (failures) return 1;
    std::printf("emission_sanitize ok: %zu samples\n", lid.size());
    return 0;
}
