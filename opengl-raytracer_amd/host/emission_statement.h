// emission_statement.h -- what glrtx_bind_emission_maps refuses (include/glrtx.h "Emission maps"), stated once for the device layer (csrc/glrtx.hip) and
// the host library (host/texture.cpp: glrt_emission_bind_check).  Internal to the two libraries.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>

namespace glrt_detail {

// type(m): the material type of the scene's material m.  "" when the bindings may be bound; otherwise the refusal, the offender named.
template <class TypeOf>
inline std::string emission_bind_error(bool have_scene, size_t scene_mats, size_t n_tex, bool cutouts_bound, const int32_t *material_emission, size_t n_mat, TypeOf type) {
    char buf[200];
    if (!have_scene) return "no scene uploaded";
    if (n_tex == 0) return "no texture set is bound (call glrtx_upload_textures first)";
    if (n_mat != scene_mats) {
        std::snprintf(buf, sizeof buf, "%zu bindings, the scene has %zu materials", n_mat, scene_mats);
        return buf;
    }
    if (cutouts_bound) return "cutouts are bound (glrtx_bind_cutouts: the two do not combine yet; unbind them first)";
    for (size_t m = 0; m < n_mat; m++) {
        const int32_t k = material_emission[m];
        if (k < -1 || (k >= 0 && (size_t)k >= n_tex)) {
            std::snprintf(buf, sizeof buf, "material %zu: emission map %d of %zu textures", m, (int)k, n_tex);
            return buf;
        }
        if (k >= 0 && type(m) == 5) {
            std::snprintf(buf, sizeof buf, "material %zu has an emission map and is a medium (type 5)", m);
            return buf;
        }
    }
    return std::string();
}

}  // namespace glrt_detail
