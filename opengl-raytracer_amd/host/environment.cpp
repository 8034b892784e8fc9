// environment.cpp -- glrt_env_weights / glrt_env_alias / glrt_env_sample / glrt_env_eval / glrt_env_from_latlong (include/glrt_host.h): the CPU statement of the
// device's environment lighting (include/glrtx.h "Environment"; csrc/environment.hip.h), bit for bit.  Compiled with -ffp-contract=off and run under MXCSR
// FTZ | DAZ like the other statements: every operation is one rounded fp32 operation in the order the header writes it.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "env_tables.h"
#include "glrt_host.h"
#include "statement_math.h"
#include "texture_statement.h"

namespace {

using glrt_detail::EnvCfg;
using glrt_detail::EnvTables;
using glrt_detail::FlushDenormals;
using glrt_detail::TexRecord;

static_assert(sizeof(glrt_env_cfg) == sizeof(EnvCfg), "glrt_env_cfg is the wire configuration");

// A checked environment: the map (offset folded into the texel pointer), the configuration, and -- for sampling -- the tables
struct Env {
    TexRecord desc;
    const unsigned char *texels;
    const EnvCfg *cfg;
    int G;
    EnvTables tab;
};

float signed_of(float m, float of) { return of < 0.0f ? -m : m; }

bool dir_to_st(const float *R, float dx, float dy, float dz, float &s, float &t, float &n1) {
    const float ex = (R[0] * dx + R[1] * dy) + R[2] * dz;
    const float ey = (R[3] * dx + R[4] * dy) + R[5] * dz;
    const float ez = (R[6] * dx + R[7] * dy) + R[8] * dz;
    const float l = (std::fabs(ex) + std::fabs(ey)) + std::fabs(ez);
    s = t = n1 = 0.0f;
    if (!(l > 0.0f && l < INFINITY)) return false;
    float px = ex / l, pz = ez / l;
    const float py = ey / l;
    n1 = 1.0f / std::sqrt((pz * pz + py * py) + px * px);
    if (ey < 0.0f) {
        const float fx = signed_of(1.0f - std::fabs(pz), px);
        const float fz = signed_of(1.0f - std::fabs(px), pz);
        px = fx; pz = fz;
    }
    s = px * 0.5f + 0.5f;
    t = pz * 0.5f + 0.5f;
    return true;
}

void st_to_dir(const float *R, float s, float t, float &dx, float &dy, float &dz, float &n1) {
    const float u = s * 2.0f - 1.0f, v = t * 2.0f - 1.0f;
    const float au = std::fabs(u), av = std::fabs(v);
    const float y = (1.0f - au) - av;
    float x = u, z = v;
    if (y < 0.0f) {
        x = signed_of(1.0f - av, u);
        z = signed_of(1.0f - au, v);
    }
    const float r = 1.0f / std::sqrt((z * z + y * y) + x * x);
    const float qx = x * r, qy = y * r, qz = z * r;
    n1 = r * ((std::fabs(x) + std::fabs(y)) + std::fabs(z));
    dx = (R[0] * qx + R[3] * qy) + R[6] * qz;
    dy = (R[1] * qx + R[4] * qy) + R[7] * qz;
    dz = (R[2] * qx + R[5] * qy) + R[8] * qz;
}
float jacobian(float n1) { return 4.0f * ((n1 * n1) * n1); }

void lookup(const Env &e, float s, float t, float rgb[3]) {
    float c[3];
    glrt_detail::texture_lookup_one(e.desc, e.texels, s, t, c);
    for (int k = 0; k < 3; k++) rgb[k] = e.cfg->scale[k] * c[k];
}

int cell(float s, int G) {
    const float a = s * (float)G;
    return a >= 0.0f ? (a < (float)G ? (int)a : G - 1) : 0;
}
float pdf_of(const Env &e, int ci, int cj, float n1) {
    const float g2 = (float)e.G * (float)e.G;
    return ((e.tab.cell_p[(size_t)cj * e.G + ci] * g2) / jacobian(n1)) * e.cfg->light_pick;
}

void block(int c, int N, int G, int &lo, int &hi) {
    lo = (c * N) / G - 1;
    hi = ((c + 1) * N + G - 1) / G;
    lo = lo < 0 ? 0 : lo;
    hi = hi > N - 1 ? N - 1 : hi;
}

constexpr int kLanes = 64;  // env_weights_kernel: one wave a cell

void weights(const Env &e, float *out) {
    const int G = e.G, N = e.desc.width;
    for (int cj = 0; cj < G; cj++)
        for (int ci = 0; ci < G; ci++) {
            int x0, x1, y0, y1;
            block(ci, N, G, x0, x1);
            block(cj, N, G, y0, y1);
            const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
            float part[kLanes];
            for (int lane = 0; lane < kLanes; lane++) {
                float sum = 0.0f;
                for (int k = lane; k < n; k += kLanes) {
                    const int x = x0 + k % bw, y = y0 + k / bw;
                    float c[3];
                    glrt_detail::texture_texel_one(e.desc, e.texels, x, y, c);
                    const float s = ((float)x + 0.5f) / (float)N, t = ((float)y + 0.5f) / (float)N;
                    float dx, dy, dz, n1;
                    st_to_dir(e.cfg->rotation, s, t, dx, dy, dz, n1);
                    const float w = glrt_detail::lum(e.cfg->scale[0] * c[0], e.cfg->scale[1] * c[1], e.cfg->scale[2] * c[2]) * jacobian(n1);
                    sum = sum + ((w > 0.0f && w < INFINITY) ? w : 0.0f);
                }
                part[lane] = sum;
            }
            for (int h = kLanes / 2; h >= 1; h >>= 1)
                for (int k = 0; k < h; k++) part[k] = part[k] + part[k + h];
            out[(size_t)cj * G + ci] = part[0];
        }
}

// The refusals of glrtx_upload_environment; on success e is ready for weights()
bool setup(Env &e, const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg) {
    const TexRecord *rec = reinterpret_cast<const TexRecord *>(map);
    const EnvCfg *c = reinterpret_cast<const EnvCfg *>(cfg);
    if (!glrt_detail::env_error(rec, texels, texel_bytes, c).empty()) return false;
    e.desc = *rec;
    e.texels = (const unsigned char *)texels + rec->offset;
    e.desc.offset = 0;
    e.cfg = c;
    e.G = glrt_detail::env_grid(c->grid, rec->width);
    return true;
}
void make_tables(Env &e) {
    std::vector<float> w((size_t)e.G * e.G);
    weights(e, w.data());
    e.tab = glrt_detail::env_tables(w.data(), e.G);
}

}  // namespace

int glrt_env_weights(const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg, float *weights_out, int32_t *grid_out) {
    Env e;
    if (!weights_out || !grid_out || !setup(e, map, texels, texel_bytes, cfg)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    weights(e, weights_out);
    *grid_out = e.G;
    return GLRT_HOST_OK;
}

int glrt_env_alias(const float *weights_in, int32_t grid, float *row_q, int32_t *row_alias, float *col_q, int32_t *col_alias, float *cell_p) {
    if (!weights_in || !row_q || !row_alias || !col_q || !col_alias || !cell_p || grid < 1 || grid > glrt_detail::kEnvGridMax) return GLRT_HOST_EINVAL;
    const EnvTables t = glrt_detail::env_tables(weights_in, grid);
    const size_t g = (size_t)grid;
    std::memcpy(row_q, t.row_q.data(), g * 4); std::memcpy(row_alias, t.row_alias.data(), g * 4);
    std::memcpy(col_q, t.col_q.data(), g * g * 4); std::memcpy(col_alias, t.col_alias.data(), g * g * 4);
    std::memcpy(cell_p, t.cell_p.data(), g * g * 4);
    return GLRT_HOST_OK;
}

int glrt_env_sample(const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg, const float *u, size_t n, float *out) {
    Env e;
    if ((n && (!u || !out)) || !setup(e, map, texels, texel_bytes, cfg)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    make_tables(e);
    const int G = e.G;
    for (size_t i = 0; i < n; i++) {
        const float *q = u + 6 * i;
        float *o = out + 8 * i;
        int cj = cell(q[0], G);
        cj = q[1] < e.tab.row_q[cj] ? cj : e.tab.row_alias[cj];
        int ci = cell(q[2], G);
        const size_t k = (size_t)cj * G + ci;
        ci = q[3] < e.tab.col_q[k] ? ci : e.tab.col_alias[k];
        const float s = ((float)ci + q[4]) / (float)G, t = ((float)cj + q[5]) / (float)G;
        float n1;
        st_to_dir(e.cfg->rotation, s, t, o[0], o[1], o[2], n1);
        o[3] = pdf_of(e, ci, cj, n1);
        lookup(e, s, t, o + 4);
        o[7] = 0.0f;
    }
    return GLRT_HOST_OK;
}

int glrt_env_eval(const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg, const float *dir, size_t n, float *out) {
    Env e;
    if ((n && (!dir || !out)) || !setup(e, map, texels, texel_bytes, cfg)) return GLRT_HOST_EINVAL;
    FlushDenormals ftz;
    make_tables(e);
    for (size_t i = 0; i < n; i++) {
        const float *d = dir + 3 * i;
        float *o = out + 4 * i;
        float s, t, n1;
        o[0] = o[1] = o[2] = o[3] = 0.0f;
        if (!dir_to_st(e.cfg->rotation, d[0], d[1], d[2], s, t, n1)) continue;
        o[3] = pdf_of(e, cell(s, e.G), cell(t, e.G), n1);
        lookup(e, s, t, o);
    }
    return GLRT_HOST_OK;
}

int glrt_env_from_latlong(const float *rgb, int32_t width, int32_t height, int32_t n, float *rgba_out) {
    if (!rgb || !rgba_out || width < 1 || height < 1 || n < 2 || n > glrt_detail::kTexMaxDim) return GLRT_HOST_EINVAL;
    const double pi = 3.14159265358979323846;
    for (int32_t j = 0; j < n; j++)
        for (int32_t i = 0; i < n; i++) {
            const double u = 2.0 * ((i + 0.5) / n) - 1.0, v = 2.0 * ((j + 0.5) / n) - 1.0;
            const double y = 1.0 - std::fabs(u) - std::fabs(v);
            double x = u, z = v;
            if (y < 0.0) {
                x = (1.0 - std::fabs(v)) * (u < 0.0 ? -1.0 : 1.0);
                z = (1.0 - std::fabs(u)) * (v < 0.0 ? -1.0 : 1.0);
            }
            const double r = 1.0 / std::sqrt(x * x + y * y + z * z);
            const double fx = (0.5 + std::atan2(x * r, -z * r) / (2.0 * pi)) * width - 0.5;
            const double fy = std::acos(std::min(1.0, std::max(-1.0, y * r))) / pi * height - 0.5;
            const double flx = std::floor(fx), fly = std::floor(fy);
            const double wx = fx - flx, wy = fy - fly;
            const auto col = [&](long long c) { return (size_t)(((c % width) + width) % width); };
            const auto row = [&](long long q) { return (size_t)std::min<long long>(std::max<long long>(q, 0), height - 1); };
            const size_t x0 = col((long long)flx), x1 = col((long long)flx + 1), y0 = row((long long)fly), y1 = row((long long)fly + 1);
            float *o = rgba_out + 4 * ((size_t)j * n + i);
            for (int c = 0; c < 3; c++) {
                const double t00 = rgb[3 * (y0 * width + x0) + c], t10 = rgb[3 * (y0 * width + x1) + c];
                const double t01 = rgb[3 * (y1 * width + x0) + c], t11 = rgb[3 * (y1 * width + x1) + c];
                const double c0 = t00 + wx * (t10 - t00), c1 = t01 + wx * (t11 - t01);
                o[c] = (float)(c0 + wy * (c1 - c0));
            }
            o[3] = 1.0f;
        }
    return GLRT_HOST_OK;
}
