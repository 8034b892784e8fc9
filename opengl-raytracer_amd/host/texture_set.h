// texture_set.h -- what a texture set must satisfy (include/glrtx.h "Textures"), stated once for the device library (glrtx_upload_textures,
// glrtx_debug_texture_lookup) and the host library (glrt_texture_lookup, glrt_texture_albedo): both refuse the same sets with the same words.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

namespace glrt_detail {

// == glrtx_texture == glrt_texture
struct TexRecord {
    uint64_t offset;
    int32_t width, height, format, wrap_s, wrap_t, filter;
};
static_assert(sizeof(TexRecord) == 32, "the texture descriptor is 32 bytes on the wire");
constexpr size_t kTexMax = 4096;
constexpr int32_t kTexMaxDim = 16384;
inline size_t tex_texel_bytes(int32_t format) { return format == 0 ? 16 : 4; }

// "" for a set that can be looked up in, else what is wrong with it and where
inline std::string texture_set_error(const TexRecord *tex, size_t n_tex, const void *texels, size_t texel_bytes) {
    char msg[192];
    if (n_tex > kTexMax) { std::snprintf(msg, sizeof msg, "%zu textures (at most %zu)", n_tex, kTexMax); return msg; }
    if (n_tex && (!tex || !texels)) return "NULL descriptors or texels with a non-zero count";
    uint64_t total = 0;
    for (size_t k = 0; k < n_tex; k++) {
        const TexRecord &d = tex[k];
        if (d.width < 1 || d.height < 1 || d.width > kTexMaxDim || d.height > kTexMaxDim) {
            std::snprintf(msg, sizeof msg, "texture %zu: %d x %d texels (each dimension 1 .. %d)", k, d.width, d.height, kTexMaxDim); return msg;
        }
        if (d.format < 0 || d.format > 2) { std::snprintf(msg, sizeof msg, "texture %zu: unknown format %d", k, d.format); return msg; }
        if (d.wrap_s < 0 || d.wrap_s > 1 || d.wrap_t < 0 || d.wrap_t > 1) { std::snprintf(msg, sizeof msg, "texture %zu: unknown wrap mode %d / %d", k, d.wrap_s, d.wrap_t); return msg; }
        if (d.filter < 0 || d.filter > 1) { std::snprintf(msg, sizeof msg, "texture %zu: unknown filter %d", k, d.filter); return msg; }
        if (d.offset % 16 != 0) { std::snprintf(msg, sizeof msg, "texture %zu: offset %llu is not a multiple of 16", k, (unsigned long long)d.offset); return msg; }
        const uint64_t n = (uint64_t)d.width * (uint64_t)d.height, bytes = n * tex_texel_bytes(d.format);
        if (d.offset > texel_bytes || bytes > texel_bytes - d.offset) {
            std::snprintf(msg, sizeof msg, "texture %zu: its last texel lies past the %zu texel bytes given", k, texel_bytes); return msg;
        }
        total += n;
        if (total > (uint64_t)INT32_MAX) { std::snprintf(msg, sizeof msg, "texture %zu: more than 2^31 - 1 texels in total", k); return msg; }
    }
    return std::string();
}

}  // namespace glrt_detail
