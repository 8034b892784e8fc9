// surface_sanitize.cpp -- a stand-alone program that drives the per-hit calls of the surface context (glrt_surface_albedo, glrt_surface_accept,
// glrt_surface_emission; host/texture.cpp, include/glrt_host.h "Surface context") over hostile barycentrics, corner coordinates, texels and ids.
// tests/test_oracle_surface.py compiles it together with host/texture.cpp under -fsanitize=address,undefined and runs it: every buffer is exactly as large
// as the header says, and the context's copies are the only thing the calls may read.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glrt_host.h"

namespace {

int failures = 0;
long bound_calls = 0, rejected = 0, accepted = 0;
void check(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), den = 1e-40f;

std::vector<unsigned char> make_texels(int w, int h, int format, int kind) {
    const size_t texel = format == GLRT_TEX_RGBA32F ? 16 : 4;
    std::vector<unsigned char> t((size_t)w * h * texel, 0);
    unsigned state = 4242u + (unsigned)(w * 31 + h);
    const float hostile[] = {nan, inf, -inf, den, -den, 0.0f, -0.0f, 0.5f};
    for (size_t k = 0; k < (size_t)w * h; k++)
        for (int c = 0; c < 4; c++) {
            state = state * 1664525u + 1013904223u;
            if (format == GLRT_TEX_RGBA32F) {
                const float v = kind == 1 ? hostile[(state >> 9) & 7u] : (float)((state >> 8) & 255u) / 255.0f;
                std::memcpy(t.data() + 16 * k + 4 * c, &v, 4);
            } else {
                t[4 * k + c] = kind == 1 ? (unsigned char)(((state >> 9) & 1u) * 255u) : (unsigned char)((state >> 8) & 255u);
            }
        }
    return t;
}

// Four triangles on two materials (0 diffuse, 1 emitter), the last two of them lights; hostile coordinates at some corners
void drive(int w, int h, int format, int wrap, int filter, int kind, int channel) {
    const glrt_texture desc{0, w, h, format, wrap, 1 - wrap, filter};
    std::vector<unsigned char> texels = make_texels(w, h, format, kind);
    const float uv[12][2] = {{0.0f, 0.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}, {nan, 1.0f}, {1.0f, inf}, {-3.5f, 0.25f},
                             {den, -den}, {7.25f, -inf}, {0.5f, 0.5f}, {-1.0f, 2.0f}, {2.0f, -1.0f}, {1e30f, -1e30f}};
    std::vector<float> vert(12 * GLRT_VERTEX_FLOATS, 0.0f);
    for (int k = 0; k < 12; k++) { vert[GLRT_VERTEX_FLOATS * k + 6] = uv[k][0]; vert[GLRT_VERTEX_FLOATS * k + 7] = uv[k][1]; }
    const float tri[16] = {0, 1, 2, 0, 3, 4, 5, 0, 6, 7, 8, 1, 9, 10, 11, 1};
    const float light[8] = {6, 7, 8, 1, 9, 10, 11, 1};
    std::vector<float> mat(2 * GLRT_MATERIAL_FLOATS, 0.0f);
    mat[0] = mat[1] = mat[2] = 2.0f;
    mat[GLRT_MATERIAL_FLOATS] = mat[GLRT_MATERIAL_FLOATS + 1] = mat[GLRT_MATERIAL_FLOATS + 2] = 1.0f;
    const int32_t albedo[2] = {0, -1}, emission[2] = {-1, 0};
    const glrt_cutout cut[2] = {{0, channel, 0.5f, 0}, {-1, 3, 0.5f, 0}};
    glrt_surface *s = nullptr;
    check(glrt_surface_create(vert.data(), 12, tri, 4, light, 2, mat.data(), 2, &desc, 1, texels.data(), texels.size(), albedo, cut, emission, &s) == GLRT_HOST_OK && s,
          "glrt_surface_create");
    if (!s) return;
    // the context holds copies: the caller's buffers may go
    std::fill(vert.begin(), vert.end(), nan);
    std::fill(texels.begin(), texels.end(), (unsigned char)0xA5);
    std::vector<unsigned char>().swap(texels);
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, den, -den, inf, -inf, nan, 1e30f, -1e30f, 0.5f, 0.25f, 0.999999f, 2.5f};
    const int ids[] = {INT32_MIN, -2, -1, 0, 1, 2, 3, 4, 5, INT32_MAX};
    for (int id : ids)
        for (float u : special)
            for (float v : special) {
                float rgb[3] = {-7.0f, -7.0f, -7.0f}, c[3] = {-7.0f, -7.0f, -7.0f};
                const int a = glrt_surface_albedo(s, id, u, v, rgb);
                check(a == (id == 0 || id == 1 ? 1 : 0), "albedo: bound exactly on the diffuse material's triangles");
                if (!a) check(rgb[0] == -7.0f && rgb[1] == -7.0f && rgb[2] == -7.0f, "albedo: an unbound call leaves rgb alone");
                const int k = glrt_surface_accept(s, id, u, v);
                check(k == 0 || k == 1, "accept returns 0 or 1");
                if (!(id == 0 || id == 1)) check(k == 1, "accept: a triangle without a record, or outside the scene, is accepted");
                else { rejected += k == 0; accepted += k == 1; }
                for (int light_side = 0; light_side < 2; light_side++) {
                    const int e = glrt_surface_emission(s, id, light_side, u, v, c);
                    const bool want = light_side ? (id == 0 || id == 1) : (id == 2 || id == 3);
                    check(e == (want ? 1 : 0), "emission: bound exactly on the emitter's triangles and lights");
                    bound_calls += e;
                }
                if (id == 2 || id == 3) {  // a light's triangle and the light read the same texel at the same coordinates
                    float t0[3], t1[3];
                    glrt_surface_emission(s, id, 0, u, v, t0);
                    glrt_surface_emission(s, id - 2, 1, u, v, t1);
                    check(std::memcmp(t0, t1, 12) == 0 || (t0[0] != t0[0] && t1[0] != t1[0]) || (t0[1] != t0[1] && t1[1] != t1[1]) || (t0[2] != t0[2] && t1[2] != t1[2]),
                          "emission: the seen and the sampled side agree");
                }
            }
    glrt_surface_free(s);
}

void refusals() {
    const glrt_texture desc{0, 2, 2, GLRT_TEX_RGBA8_UNORM, 0, 0, 0};
    const std::vector<unsigned char> texels(16, 128);
    std::vector<float> vert(3 * GLRT_VERTEX_FLOATS, 0.0f), mat(GLRT_MATERIAL_FLOATS, 0.0f);
    mat[0] = 2.0f;
    const float tri[4] = {0, 1, 2, 0}, bad_tri[4] = {0, 1, 3, 0}, bad_mat[4] = {0, 1, 2, 1};
    const int32_t bind = 0, past = 1;
    glrt_surface *s = nullptr;
    check(glrt_surface_create(vert.data(), 3, tri, 1, nullptr, 0, mat.data(), 1, &desc, 1, texels.data(), 16, &bind, nullptr, nullptr, nullptr) == GLRT_HOST_EINVAL, "a NULL result is refused");
    check(glrt_surface_create(vert.data(), 3, bad_tri, 1, nullptr, 0, mat.data(), 1, &desc, 1, texels.data(), 16, &bind, nullptr, nullptr, &s) == GLRT_HOST_EINDEX && !s, "a corner past the vertices");
    check(glrt_surface_create(vert.data(), 3, bad_mat, 1, nullptr, 0, mat.data(), 1, &desc, 1, texels.data(), 16, &bind, nullptr, nullptr, &s) == GLRT_HOST_EINDEX && !s, "a material past the materials");
    check(glrt_surface_create(vert.data(), 3, tri, 1, nullptr, 0, mat.data(), 1, &desc, 1, texels.data(), 16, &past, nullptr, nullptr, &s) == GLRT_HOST_EINDEX && !s, "texture 1 of 1");
    check(glrt_surface_create(vert.data(), 3, tri, 1, nullptr, 0, mat.data(), 1, &desc, 1, texels.data(), 15, &bind, nullptr, nullptr, &s) == GLRT_HOST_EINVAL && !s, "a short blob");
    check(glrt_surface_create(vert.data(), 3, tri, 1, tri, 1, mat.data(), 1, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, &s) == GLRT_HOST_OK && s, "nothing bound, no set");
    if (s) {
        float rgb[3];
        check(glrt_surface_albedo(s, 0, 0.3f, 0.3f, rgb) == 0 && glrt_surface_accept(s, 0, 0.3f, 0.3f) == 1 && glrt_surface_emission(s, 0, 1, 0.3f, 0.3f, rgb) == 0, "nothing bound");
    }
    glrt_surface_free(s);
    glrt_surface_free(nullptr);
}

}  // namespace

int main() {
    const int sizes[][2] = {{1, 1}, {1, 7}, {3, 7}, {5, 4}};
    for (int format : {GLRT_TEX_RGBA32F, GLRT_TEX_RGBA8_UNORM, GLRT_TEX_RGBA8_SRGB})
        for (int filter : {GLRT_TEX_NEAREST, GLRT_TEX_BILINEAR})
            for (int wrap : {GLRT_TEX_REPEAT, GLRT_TEX_CLAMP})
                for (int kind = 0; kind < 2; kind++)
                    for (const auto &sz : sizes) drive(sz[0], sz[1], format, wrap, filter, kind, (sz[0] + kind) % 4);
    refusals();
    check(bound_calls > 0 && rejected > 0 && accepted > 0, "the calls looked textures up, and both decisions occurred");
    if (failures) return 1;
    std::printf("surface_sanitize ok\n");
    return 0;
}
