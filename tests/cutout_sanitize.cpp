// cutout_sanitize.cpp -- a stand-alone program that runs the host statements of the alpha cutouts (glrt_texture_channel, glrt_render_features_geom_cutout;
// host/texture.cpp, host/query.cpp, host/features.cpp) over hostile textures, coordinates and records.  tests/test_cutout_host.py compiles it together with
// those files under -fsanitize=address,undefined and runs it: every buffer is exactly as large as the header says.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "glrt_host.h"

namespace {

int failures = 0;
long total_hits = 0;  // pixels that kept a triangle, over all the feature calls: the rays do reach the quad
void check(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), den = 1e-40f;

struct Tex {
    glrt_texture desc;
    std::vector<unsigned char> texels;
};

// kind 0: noise; 1: NaN, inf and denormal floats among the texels (RGBA32F), bytes 0 and 255 (8-bit)
Tex make_tex(int w, int h, int format, int wrap, int filter, int kind) {
    Tex t;
    t.desc = glrt_texture{0, w, h, format, wrap, 1 - wrap, filter};
    const size_t texel = format == GLRT_TEX_RGBA32F ? 16 : 4;
    t.texels.assign((size_t)w * h * texel, 0);
    unsigned state = 777u + (unsigned)(w * 31 + h);
    const float hostile[] = {nan, inf, -inf, den, -den, 0.0f, -0.0f, 0.5f};
    for (size_t k = 0; k < (size_t)w * h; k++)
        for (int c = 0; c < 4; c++) {
            state = state * 1664525u + 1013904223u;
            if (format == GLRT_TEX_RGBA32F) {
                const float v = kind == 1 ? hostile[(state >> 9) & 7u] : (float)((state >> 8) & 255u) / 255.0f;
                std::memcpy(t.texels.data() + 16 * k + 4 * c, &v, 4);
            } else {
                t.texels[4 * k + c] = kind == 1 ? (unsigned char)(((state >> 9) & 1u) * 255u) : (unsigned char)((state >> 8) & 255u);
            }
        }
    return t;
}

void lookups(const Tex &t) {
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, den, -den, inf, -inf, nan, 1e30f, -1e30f, 0.5f, 0.999999f, 2.5f, -2.5f};
    std::vector<float> st;
    std::vector<int32_t> which, channel;
    for (float s : special)
        for (float q : special)
            for (int c = 0; c < 4; c++) { st.push_back(s); st.push_back(q); which.push_back(0); channel.push_back(c); }
    std::vector<float> out(which.size()), rgb(3 * which.size());
    check(glrt_texture_channel(&t.desc, 1, t.texels.data(), t.texels.size(), which.data(), channel.data(), st.data(), which.size(), out.data()) == GLRT_HOST_OK,
          "glrt_texture_channel");
    check(glrt_texture_lookup(&t.desc, 1, t.texels.data(), t.texels.size(), which.data(), st.data(), which.size(), rgb.data()) == GLRT_HOST_OK, "glrt_texture_lookup");
    for (size_t i = 0; i < which.size(); i++)
        if (channel[i] < 3) check(std::memcmp(&out[i], &rgb[3 * i + channel[i]], 4) == 0, "channels 0 .. 2 are the lookup's words");
    int32_t bad_channel = 4, bad_which = 1;
    check(glrt_texture_channel(&t.desc, 1, t.texels.data(), t.texels.size(), which.data(), &bad_channel, st.data(), 1, out.data()) == GLRT_HOST_EINDEX, "channel 4 is refused");
    check(glrt_texture_channel(&t.desc, 1, t.texels.data(), t.texels.size(), &bad_which, channel.data(), st.data(), 1, out.data()) == GLRT_HOST_EINDEX, "texture 1 of 1 is refused");
    check(glrt_texture_channel(&t.desc, 1, t.texels.data(), t.texels.size() - 1, which.data(), channel.data(), st.data(), 1, out.data()) == GLRT_HOST_EINVAL, "a short blob is refused");
    check(glrt_texture_channel(&t.desc, 1, t.texels.data(), t.texels.size(), which.data(), channel.data(), st.data(), 1, nullptr) == GLRT_HOST_EINVAL, "a NULL output is refused");
}

// Two triangles (a quad z = 0 in front of the camera, hostile coordinates at its corners) under one fork, one diffuse material
void features(const Tex &t, float cutoff, int channel, bool expect_hits) {
    const float uv[6][2] = {{0.0f, 0.0f}, {nan, 1.0f}, {1.0f, inf}, {-3.5f, 0.25f}, {den, -den}, {7.25f, -inf}};
    const float pos[6][3] = {{-1, -1, 0}, {1, -1, 0}, {1, 1, 0}, {-1, -1, 0}, {1, 1, 0}, {-1, 1, 0}};
    std::vector<float> vert(6 * GLRT_VERTEX_FLOATS, 0.0f);
    for (int k = 0; k < 6; k++) {
        float *v = &vert[GLRT_VERTEX_FLOATS * k];
        v[0] = pos[k][0]; v[1] = pos[k][1]; v[2] = pos[k][2];
        v[5] = 1.0f;
        v[6] = uv[k][0]; v[7] = uv[k][1];
    }
    const float tri[8] = {0, 1, 2, 0, 3, 4, 5, 0};
    const float nodes[27] = {-1, -1, 0, 1, 1, 0, 1, 2, -1, -1, -1, 0, 1, 1, 0, -1, -1, 0, -1, -1, 0, 1, 1, 0, -1, -1, 1};
    std::vector<float> mat(GLRT_MATERIAL_FLOATS, 0.0f);
    mat[0] = mat[1] = mat[2] = 2.0f;
    mat[6] = mat[7] = mat[8] = 0.5f;
    const float c2w[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 3, 1};  // column-major: the camera at z = 3, looking down -z
    const float s2c[16] = {0.46796167f, 0, 0, 0, 0, 0.3639702f, 0, 0, 0, 0, 0, -4.995f, 0, 0, -0.9999999f, 5.0049996f};  // the inverse of a 40-degree projection
    const int W = 9, H = 7;
    std::vector<float> n(4 * W * H), a(4 * W * H), g(4 * W * H);
    const int32_t bind = 0;
    glrt_cutout cut{0, channel, cutoff, 0};
    const int rc = glrt_render_features_geom_cutout(vert.data(), 6, tri, 2, nodes, 3, mat.data(), 1, c2w, s2c, W, H, 0, 1, 16, &t.desc, 1, t.texels.data(), t.texels.size(),
                                                    &bind, &cut, n.data(), a.data(), g.data());
    check(rc == GLRT_HOST_OK, "glrt_render_features_geom_cutout");
    int hits = 0;
    for (int i = 0; i < W * H; i++) {
        int32_t tr;
        std::memcpy(&tr, &g[4 * i], 4);
        check(tr >= -1 && tr < 2, "plane G names a triangle of the scene or a miss");
        hits += tr >= 0;
    }
    if (!expect_hits) check(hits == 0, "a cutoff nothing reaches rejects every candidate");
    total_hits += hits;
    cut.reserved = 1;
    check(glrt_render_features_geom_cutout(vert.data(), 6, tri, 2, nodes, 3, mat.data(), 1, c2w, s2c, W, H, 0, 1, 16, &t.desc, 1, t.texels.data(), t.texels.size(), &bind,
                                           &cut, n.data(), a.data(), g.data()) == GLRT_HOST_EINVAL, "reserved non-zero is refused");
    cut = glrt_cutout{0, channel, nan, 0};
    check(glrt_render_features_geom_cutout(vert.data(), 6, tri, 2, nodes, 3, mat.data(), 1, c2w, s2c, W, H, 0, 1, 16, &t.desc, 1, t.texels.data(), t.texels.size(), &bind,
                                           &cut, n.data(), a.data(), g.data()) == GLRT_HOST_EINVAL, "a NaN cutoff is refused");
    cut = glrt_cutout{1, channel, 0.5f, 0};
    check(glrt_render_features_geom_cutout(vert.data(), 6, tri, 2, nodes, 3, mat.data(), 1, c2w, s2c, W, H, 0, 1, 16, &t.desc, 1, t.texels.data(), t.texels.size(), &bind,
                                           &cut, n.data(), a.data(), g.data()) == GLRT_HOST_EINDEX, "texture 1 of 1 is refused");
}

}  // namespace

int main() {
    const int formats[] = {GLRT_TEX_RGBA32F, GLRT_TEX_RGBA8_UNORM, GLRT_TEX_RGBA8_SRGB};
    const int sizes[][2] = {{1, 1}, {1, 7}, {2, 3}, {5, 4}};
    for (int format : formats)
        for (int filter : {GLRT_TEX_NEAREST, GLRT_TEX_BILINEAR})
            for (int wrap : {GLRT_TEX_REPEAT, GLRT_TEX_CLAMP})
                for (int kind = 0; kind < 2; kind++)
                    for (const auto &sz : sizes) {
                        const Tex t = make_tex(sz[0], sz[1], format, wrap, filter, kind);
                        lookups(t);
                        for (int channel = 0; channel < 4; channel++) {
                            features(t, 0.5f, channel, true);
                            features(t, 0.0f, channel, true);
                            features(t, -0.0f, channel, true);
                            features(t, 3.0e38f, channel, kind == 1);  // (a hostile texture holds +inf, which passes any finite cutoff)
                        }
                    }
    check(total_hits > 0, "the feature calls hit the quad");
    if (failures) return 1;
    std::printf("cutout_sanitize ok\n");
    return 0;
}
