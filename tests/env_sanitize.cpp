// env_sanitize.cpp -- a stand-alone program that runs the host statements of the environment lighting (glrt_env_weights, glrt_env_alias, glrt_env_sample,
// glrt_env_eval, glrt_env_from_latlong; host/environment.cpp) over hostile maps, directions and uniforms.  tests/test_env_host.py compiles it together with
// host/environment.cpp and host/texture.cpp under -fsanitize=address,undefined and runs it: every output buffer is exactly as large as the header says.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "glrt_host.h"

namespace {

int failures = 0;
void check(bool ok, const char *what) {
    if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}

struct Map {
    glrt_texture desc;
    std::vector<unsigned char> texels;
};

Map make_map(int n, int format, int filter, int kind) {
    Map m;
    m.desc = glrt_texture{0, n, n, format, GLRT_TEX_CLAMP, GLRT_TEX_CLAMP, filter};
    const size_t texel = format == GLRT_TEX_RGBA32F ? 16 : 4;
    m.texels.assign((size_t)n * n * texel, 0);
    unsigned state = 12345u + (unsigned)n;
    for (size_t k = 0; k < (size_t)n * n; k++) {
        state = state * 1664525u + 1013904223u;
        const bool lit = kind == 2 || (kind == 1 && k == (size_t)n * (n / 2) + 1);  // 0: all zero, 1: one texel, 2: noise
        if (format == GLRT_TEX_RGBA32F) {
            float *p = reinterpret_cast<float *>(m.texels.data() + 16 * k);
            for (int c = 0; c < 4; c++) p[c] = lit ? (float)((state >> (8 * c)) & 255u) / 32.0f : 0.0f;
        } else {
            for (int c = 0; c < 4; c++) m.texels[4 * k + c] = lit ? (unsigned char)((state >> (8 * c)) & 255u) : 0;
        }
    }
    return m;
}

void run(const Map &m, int grid, float light_pick) {
    glrt_env_cfg cfg{0, grid, light_pick, {1.0f, 0.5f, 2.0f}, {0, 0, -1, 0, 1, 0, 1, 0, 0}};
    const int G = grid > 0 ? grid : (m.desc.width < 256 ? m.desc.width : 256);
    std::vector<float> w((size_t)G * G);
    int32_t g_out = 0;
    check(glrt_env_weights(&m.desc, m.texels.data(), m.texels.size(), &cfg, w.data(), &g_out) == GLRT_HOST_OK && g_out == G, "glrt_env_weights");
    std::vector<float> row_q(G), col_q((size_t)G * G), cell_p((size_t)G * G);
    std::vector<int32_t> row_alias(G), col_alias((size_t)G * G);
    check(glrt_env_alias(w.data(), G, row_q.data(), row_alias.data(), col_q.data(), col_alias.data(), cell_p.data()) == GLRT_HOST_OK, "glrt_env_alias");
    for (int k = 0; k < G; k++) check(row_alias[k] >= 0 && row_alias[k] < G, "row alias in range");
    for (size_t k = 0; k < (size_t)G * G; k++) check(col_alias[k] >= 0 && col_alias[k] < G, "column alias in range");

    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN(), den = 1e-40f, below1 = std::nextafter(1.0f, 0.0f);
    const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, den, -den, inf, -inf, nan, 1e30f, -1e-30f, 0.5f};
    std::vector<float> dirs;
    for (float x : special)
        for (float y : special)
            for (float z : special) { dirs.push_back(x); dirs.push_back(y); dirs.push_back(z); }
    std::vector<float> ev(dirs.size() / 3 * 4);
    check(glrt_env_eval(&m.desc, m.texels.data(), m.texels.size(), &cfg, dirs.data(), dirs.size() / 3, ev.data()) == GLRT_HOST_OK, "glrt_env_eval");
    for (float v : ev) check(v == v, "glrt_env_eval: no NaN for a finite map");

    const float us[] = {0.0f, below1, 0.5f, 0.25f, den, 1.0f / 3.0f, 1.0f, nan, -1.0f, 2.0f};  // (the last four lie outside what rand() returns: they must stay in bounds)
    std::vector<float> u;
    for (float a : us)
        for (float b : us)
            for (float c : us) { u.push_back(a); u.push_back(b); u.push_back(c); u.push_back(b); u.push_back(a); u.push_back(c); }
    std::vector<float> sm(u.size() / 6 * 8);
    check(glrt_env_sample(&m.desc, m.texels.data(), m.texels.size(), &cfg, u.data(), u.size() / 6, sm.data()) == GLRT_HOST_OK, "glrt_env_sample");
}

}  // namespace

int main() {
    const int formats[] = {GLRT_TEX_RGBA32F, GLRT_TEX_RGBA8_UNORM, GLRT_TEX_RGBA8_SRGB};
    for (int format : formats)
        for (int filter : {GLRT_TEX_NEAREST, GLRT_TEX_BILINEAR})
            for (int kind = 0; kind < 3; kind++) {
                run(make_map(2, format, filter, kind), 0, 1.0f);
                run(make_map(8, format, filter, kind), 4, 0.5f);
                run(make_map(10, format, filter, kind), 4, 0.0f);
                run(make_map(7, format, filter, kind), 3, 1.0f);
                run(make_map(4, format, filter, kind), 6, 0.75f);
            }
    run(make_map(64, GLRT_TEX_RGBA32F, GLRT_TEX_BILINEAR, 2), 0, 1.0f);

    // refusals read nothing
    const Map m = make_map(4, GLRT_TEX_RGBA32F, GLRT_TEX_NEAREST, 2);
    glrt_env_cfg cfg{0, 0, 0.5f, {1, 1, 1}, {1, 0, 0, 0, 1, 0, 0, 0, 1}};
    float w[16];
    int32_t g = 0;
    glrt_texture bad = m.desc;
    bad.height = 3;
    check(glrt_env_weights(&bad, m.texels.data(), m.texels.size(), &cfg, w, &g) == GLRT_HOST_EINVAL, "a map that is not square is refused");
    check(glrt_env_weights(&m.desc, m.texels.data(), m.texels.size() - 1, &cfg, w, &g) == GLRT_HOST_EINVAL, "a short blob is refused");
    check(glrt_env_weights(&m.desc, m.texels.data(), m.texels.size(), nullptr, w, &g) == GLRT_HOST_EINVAL, "a NULL configuration is refused");
    cfg.grid = 1025;
    check(glrt_env_weights(&m.desc, m.texels.data(), m.texels.size(), &cfg, w, &g) == GLRT_HOST_EINVAL, "grid 1025 is refused");

    // lat-long resampling
    std::vector<float> img(3 * 5 * 3, 0.5f), out(4 * 6 * 6);
    check(glrt_env_from_latlong(img.data(), 5, 3, 6, out.data()) == GLRT_HOST_OK, "glrt_env_from_latlong");
    check(glrt_env_from_latlong(img.data(), 1, 1, 2, out.data()) == GLRT_HOST_OK, "glrt_env_from_latlong of one pixel");
    for (int k = 0; k < 16; k++) check(out[k] == (k % 4 == 3 ? 1.0f : 0.5f), "a constant image stays constant");

    if (failures) return 1;
    std::printf("env_sanitize ok\n");
    return 0;
}
