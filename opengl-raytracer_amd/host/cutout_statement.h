// cutout_statement.h -- the CPU statement of the cutout rule (include/glrtx.h "Cutouts") inside glrt_trace_rays' walker (host/query.cpp), for the feature
// statement that searches with it (host/features.cpp: glrt_render_features_geom_cutout).  Internal to the host library.  glrt_trace_rays itself stays geometric.
#pragma once
#include <cstddef>

#include "glrt_host.h"
#include "texture_set.h"

namespace glrt_detail {

// A checked set and one record a material (the caller has validated both)
struct CutoutHook {
    const TexRecord *tex;
    const unsigned char *texels;
    const glrt_cutout *cut;
};

// glrt_trace_rays with the rule applied to every candidate that would become the closest hit (hook == nullptr: glrt_trace_rays)
int trace_rays_cutout(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *rays, size_t n, float *hits_out,
                      int flags, const CutoutHook *hook);

}  // namespace glrt_detail
