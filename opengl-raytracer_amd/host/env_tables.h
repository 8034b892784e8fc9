// env_tables.h -- what an environment must satisfy and how its sampling tables are built from the importance grid's cell weights (include/glrtx.h
// "Environment"), stated once for the device library (glrtx_upload_environment, glrtx_set_environment_cfg, the glrtx_debug_env_* hooks) and the host library
// (glrt_env_*): both refuse the same maps and configurations with the same words, and both build the same tables word for word.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "texture_set.h"

namespace glrt_detail {

// == glrtx_env_cfg == glrt_env_cfg
struct EnvCfg {
    int32_t mode, grid;
    float light_pick;
    float scale[3];
    float rotation[9];
};
static_assert(sizeof(EnvCfg) == 60, "the environment configuration is 60 bytes on the wire");
constexpr int32_t kEnvGridMax = 1024;

// "" for a map and a configuration an environment can be made of, else what is wrong and where.  cfg alone (map == nullptr, check_map false): the configuration's part.
inline std::string env_error(const TexRecord *map, const void *texels, size_t texel_bytes, const EnvCfg *cfg, bool check_map = true) {
    char msg[192];
    if (!cfg) return "NULL configuration";
    if (check_map) {
        if (!map || !texels) return "NULL map descriptor or texels";
        const std::string bad = texture_set_error(map, 1, texels, texel_bytes);
        if (!bad.empty()) return "map: " + bad;
        if (map->width != map->height || map->width < 2) {
            std::snprintf(msg, sizeof msg, "map: %d x %d texels (an octahedral map is square, 2 .. %d a side)", map->width, map->height, kTexMaxDim); return msg;
        }
        if (map->wrap_s != 1 || map->wrap_t != 1) { std::snprintf(msg, sizeof msg, "map: wrap mode %d / %d (an octahedral map clamps on both axes)", map->wrap_s, map->wrap_t); return msg; }
    }
    if (cfg->mode < 0 || cfg->mode > 1) { std::snprintf(msg, sizeof msg, "mode %d (0 escape, 1 sampled)", cfg->mode); return msg; }
    if (cfg->grid < 0 || cfg->grid > kEnvGridMax) { std::snprintf(msg, sizeof msg, "grid %d (1 .. %d, or 0 for min(N, 256))", cfg->grid, kEnvGridMax); return msg; }
    if (!(cfg->light_pick >= 0.0f && cfg->light_pick <= 1.0f)) { std::snprintf(msg, sizeof msg, "light_pick %g lies outside [0, 1]", cfg->light_pick); return msg; }
    for (int k = 0; k < 3; k++)
        if (!(cfg->scale[k] >= 0.0f && cfg->scale[k] < INFINITY)) { std::snprintf(msg, sizeof msg, "scale[%d] = %g is negative or not finite", k, cfg->scale[k]); return msg; }
    for (int k = 0; k < 9; k++)
        if (!(std::fabs(cfg->rotation[k]) < INFINITY)) { std::snprintf(msg, sizeof msg, "rotation[%d] = %g is not finite", k, cfg->rotation[k]); return msg; }
    return std::string();
}

inline int32_t env_grid(int32_t grid, int32_t n) { return grid > 0 ? grid : (n < 256 ? n : 256); }

// Vose's alias method in float64.  total = w[0] + w[1] + .. in index order.  total == 0 (or not finite): every threshold 1, every alias its own index.
// Otherwise p[i] = w[i] * n / total; indices with p < 1 go on the `small` stack and the others on the `large` stack, both in increasing index order; while
// neither is empty: s = small's top, l = large's top (both popped); q[s] = p[s], alias[s] = l; p[l] = (p[l] + p[s]) - 1; l goes back on small if p[l] < 1, else
// on large.  What is left on either stack gets threshold 1 and its own index.  Thresholds are rounded once to fp32.
inline void env_alias(const double *w, size_t n, float *q, int32_t *alias) {
    double total = 0.0;
    for (size_t i = 0; i < n; i++) total += w[i];
    for (size_t i = 0; i < n; i++) { q[i] = 1.0f; alias[i] = (int32_t)i; }
    if (!(total > 0.0) || !(total < INFINITY)) return;
    std::vector<double> p(n);
    std::vector<int32_t> small, large;
    for (size_t i = 0; i < n; i++) {
        p[i] = w[i] * (double)n / total;
        (p[i] < 1.0 ? small : large).push_back((int32_t)i);
    }
    while (!small.empty() && !large.empty()) {
        const int32_t s = small.back(), l = large.back();
        small.pop_back(); large.pop_back();
        q[s] = (float)p[s];
        alias[s] = l;
        p[l] = (p[l] + p[s]) - 1.0;
        (p[l] < 1.0 ? small : large).push_back(l);
    }
}

// The tables of a G x G grid of cell weights (row j, column i at j * G + i): a row table over the rows' sums (each summed in column order), one column table a
// row, and cell_p = (float)(w / total) with total the rows' sums added in row order (0 everywhere for an all-zero grid).
struct EnvTables {
    std::vector<float> row_q, col_q, cell_p;
    std::vector<int32_t> row_alias, col_alias;
};
inline EnvTables env_tables(const float *w, int32_t G) {
    EnvTables t;
    const size_t g = (size_t)G;
    t.row_q.resize(g); t.row_alias.resize(g); t.col_q.resize(g * g); t.col_alias.resize(g * g); t.cell_p.assign(g * g, 0.0f);
    std::vector<double> rows(g, 0.0), line(g);
    for (size_t j = 0; j < g; j++)
        for (size_t i = 0; i < g; i++) rows[j] += (double)w[j * g + i];
    double total = 0.0;
    for (size_t j = 0; j < g; j++) total += rows[j];
    env_alias(rows.data(), g, t.row_q.data(), t.row_alias.data());
    for (size_t j = 0; j < g; j++) {
        for (size_t i = 0; i < g; i++) line[i] = (double)w[j * g + i];
        env_alias(line.data(), g, t.col_q.data() + j * g, t.col_alias.data() + j * g);
    }
    if (total > 0.0 && total < INFINITY)
        for (size_t k = 0; k < g * g; k++) t.cell_p[k] = (float)((double)w[k] / total);
    return t;
}

}  // namespace glrt_detail
