/*
 * glrt_host.h -- C ABI of libglrt_host.so: host-side (CPU) helpers that sit
 * next to the device path: BVH construction into the reference's flat
 * 'u_bvhBuffer' format and the camera matrices the reference computes with GLM.
 * No GPU, no HIP; loadable on any box.
 *
 * Reference interfaces replaced:
 *   glrt_bvh_build_sah      BVH::construct / constructRec   src/core/bvh.cpp:59-160
 *   glrt_bvh_build_reference  the same pair, restated rule for rule: the reference host's OWN tree (opt-in: exact ties and
 *                            grazing-ray box misses then fall where the reference host's would; parity unpinned, see below)
 *   glrt_bvh_build_lbvh     same role, linear BVH for large scenes (BASELINE config 5)
 *   glrt_bvh_build_chain    (no counterpart: expresses BASELINE config "brute force, no BVH"
 *                            in the same node format)
 *   glrt_look_at            glm::lookAt                     src/core/scene.cpp:93
 *   glrt_perspective        glm::perspective(radians(fov))  src/core/scene.cpp:113
 *   glrt_mat4_inverse/_mul  glm::inverse, operator*         src/core/window.cpp:230-233
 *   glrt_frame_seed         per-frame u_seed draw           src/core/window.cpp:226-238
 *                            (the reference draws from mt19937(random_device); this is the
 *                             deterministic sequence SURVEY.md section 8(d) fixes)
 * All matrices are column-major float[16] exactly as uploaded by
 * glUniformMatrix4fv(..., GL_FALSE, ...) (shader_program.cpp:151-156).
 */
#ifndef GLRT_HOST_H
#define GLRT_HOST_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLRT_HOST_OK 0
#define GLRT_HOST_EINVAL (-1) /* null pointer / empty input */
#define GLRT_HOST_EINDEX (-2) /* triangle references a vertex out of range */
#define GLRT_HOST_EDEPTH (-3) /* tree deeper than the 64-entry traversal stack allows */

/* floats per Vertex record in u_vertBuffer: pos, normal, uv, tangent, binormal (trimesh.h:15-25) */
#define GLRT_VERTEX_FLOATS 15
/* floats per Material record in u_matBuffer: 6 x vec3 (scene.h:28-35) */
#define GLRT_MATERIAL_FLOATS 18
/* floats per BVH node in u_bvhBuffer: 3 x vec3 (bvh.h:84-100) */
#define GLRT_BVHNODE_FLOATS 9

/* 2*n_tri-1 (one triangle per leaf), 0 for an empty scene. */
size_t glrt_bvh_node_count(size_t n_tri);

/* vert: n_vert * GLRT_VERTEX_FLOATS, tri: n_tri * 4 (i, j, k, material) as floats.
 * nodes_out: glrt_bvh_node_count(n_tri) * 9 floats.  max_depth_out may be NULL.
 * glrt_bvh_build_sah: 16 bins on each of the three axes; a subtree of n triangles is charged n^0.8 in the split cost (every subtree ends in one-triangle leaves, where the
 * surface-area heuristic's n overstates what a ray pays: headline -0.6 ... -0.8 % per frame, profiles/r06_sah_count_weight.txt; GLRT_SAH_ALPHA=1 restores the heuristic). */
int glrt_bvh_build_sah(const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out,
                       int *max_depth_out);
int glrt_bvh_build_chain(const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out);
/* The tree the reference's own host builds (BVH::constructRec, src/core/bvh.cpp:72-160 with bvh.h:11-82), restated rule for rule: longest centroid axis only,
 * std::nth_element at the middle for <= 8 triangles, 16 buckets + std::partition above, the cut at the unsorted middle when no bucket split pays, boxes accumulated from
 * +-1e8, nodes in pre-order.  A closest hit depends on the tree only at exact ties and at grazing-ray box misses: under this tree both fall where
 * the reference host's do -- to the extent that libstdc++'s nth_element / partition order is the reference build's (same toolchain: yes).  It is a worse tree than
 * glrt_bvh_build_sah's (one axis binned) and is never improved behind the caller's back: glrt::Scene applies neither glrt_bvh_lights_first nor any other re-ordering to it.
 * PARITY UNPINNED: the reference host is unbuildable here, no tree of its making exists to compare with.  Same arguments and return codes as
 * glrt_bvh_build_sah. */
int glrt_bvh_build_reference(const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out, int *max_depth_out);
/* Linear BVH (30-bit Morton order + Karras hierarchy), improved by GLRT_LBVH_ROTATION_PASSES bottom-up sweeps of tree
 * rotations (child <-> grandchild and grandchild <-> grandchild exchanges) and by rebuilding every maximal subtree of at most
 * GLRT_LBVH_REBUILD_LEAVES leaves with the exact sweep SAH.  Same output, bit for bit, as the GPU builder glrtx_build_lbvh (include/glrtx.h); internal node i at index i,
 * leaves after them in Morton order. */
#ifndef GLRT_LBVH_ROTATION_PASSES
#define GLRT_LBVH_ROTATION_PASSES 4
#endif
#ifndef GLRT_LBVH_REBUILD_LEAVES
#define GLRT_LBVH_REBUILD_LEAVES 64
#endif
int glrt_bvh_build_lbvh(const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out,
                        int *max_depth_out);
/* Binned SAH built level by level from the top (16 bins, 3 axes) down to segments of at most GLRT_LBVH_REBUILD_LEAVES triangles, which the exact sweep SAH of the
 * LBVH pass then builds from their leaves (host/bvh.cpp: "SAH by levels").  Same node layout as glrt_bvh_build_lbvh; same output, bit for bit, as the GPU builder
 * glrtx_build_bvh_sah (include/glrtx.h).  Quality: the CPU binned-SAH tree's or better (profiles/r05_tree_study.txt). */
int glrt_bvh_build_sah_levels(const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out, int *max_depth_out);
/* Post-pass over a tree of ANY of the builders above (or of the device builders, include/glrtx.h): at every fork where exactly one child's subtree contains emitting
 * triangles (material emission != 0: the rule of the light list, scene.cpp:246-248) that child is put into the slot the reference's traversal visits FIRST (children.y,
 * raytrace.frag:299-307), so that shadow rays -- half of all rays -- meet their light before anything else and cull the rest by its distance.  Two child references per
 * exchanged fork change, nothing else.  mat: n_mat records of 18 floats (scene.h:28-35).  Returns the number of forks exchanged (>= 0) or GLRT_HOST_E*.
 * glrt::Scene::parse and the Python scene builder apply it after their builder (GLRT_BVH_LIGHTS_FIRST=0 leaves the builder's order). */
int glrt_bvh_lights_first(float *nodes, size_t n_nodes, const float *tri, size_t n_tri, const float *mat, size_t n_mat);
/* The order of a fork's children from measured hits: tri_hits[t] = closest hits triangle t collected in a calibration frame (glrtx_hit_histogram, glrtx.h); at every
 * fork the child whose subtree collected more hits PER UNIT COST (a subtree of n triangles is charged n^0.5; GLRT_HITS_COST_EXP overrides, 0 = hits alone: round 6's first
 * form, which sent every ray through the bigger child first on unbalanced trees) goes into the slot the traversal visits first (raytrace.frag:299-307).  No box and no closest hit changes; exact ties between
 * two triangles may resolve to the other one.  Apply it last.  Returns the forks exchanged, or GLRT_HOST_E*. */
int glrt_bvh_order_by_hits(float *nodes, size_t n_nodes, const uint32_t *tri_hits, size_t n_tri);
/* The shadow rays' share of a calibration frame's hits, by the reference's sampling rule (raytrace.frag:341-343: a light triangle is drawn uniformly for every shaded
 * hit): (sum of tri_hits) / (number of emitting triangles) is added to every emitting triangle.  Call it on glrtx_hit_histogram's output before glrt_bvh_order_by_hits.
 * Returns the number of emitting triangles, or GLRT_HOST_E*. */
int glrt_bvh_add_shadow_hits(uint32_t *tri_hits, size_t n_tri, const float *tri, const float *mat, size_t n_mat);
/* Optimisation pass over a finished tree of any builder: every subtree is taken out and put back where the summed area of the forks' boxes grows least (insertion-based
 * optimisation, Bittner et al. 2013; host/bvh.cpp).  At most max_passes passes, stopping when one gains < 0.1 %.  The tree is renumbered in DFS pre-order.
 * cost_out (may be NULL): summed fork area / root area before [0] and after [1].  Returns the number of subtrees moved (>= 0; 0 and max_depth -1 for trees it leaves
 * alone: < 4 leaves, absent children, non-finite boxes) or GLRT_HOST_E*
 * -- GLRT_HOST_EDEPTH when the optimised tree would be deeper than the 64-entry traversal stack allows: `nodes` is then left exactly as it came in.  Apply glrt_bvh_lights_first AFTER it. */
int glrt_bvh_reinsert(float *nodes, size_t n_nodes, int max_passes, int *max_depth_out, double *cost_out);

/* Refit: new boxes for a wire-format tree (9 floats per node, root = node 0) after its triangles' vertices moved; topology, child refs and leaf triangles untouched.
 * Rule, over the nodes reachable from node 0 (the others are left as they are):
 *   leaf              the componentwise min / max of its triangle's three vertex positions;
 *   fork              the componentwise min / max of its present children's boxes (a fork with one child takes that child's box);
 *   fork, no children keeps its box.
 * Min and max are taken in a TOTAL order on float bit patterns, not with `<`: the ordered-integer key (all bits flipped when the sign is set, else the sign bit
 * set), so -0 < +0 and NaNs lie beyond +-inf by bit pattern, and the chosen value is kept bit for bit (denormals too).  A box is then a function of the set of
 * positions under it, whatever the association -- the device refit (glrtx_update_vertices, include/glrtx.h) folds in parallel and lands on the same bits.
 * For trees of the builders above (coordinates inside +-1e8) refitting unchanged vertices gives back every reachable fork box numerically (==; -0 and +0 may
 * trade places); glrt_bvh_build_chain's forks, which carry the global box by design, become tight suffix boxes.
 * Same checks and codes as the builders: GLRT_HOST_EINVAL for NULL / empty input or a malformed tree (a child or leaf triangle out of range, a node reached
 * twice), GLRT_HOST_EINDEX for a triangle with a vertex index out of range.  On error `nodes` is unchanged. */
int glrt_bvh_refit(const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes, size_t n_nodes);

/* Batched ray queries on a wire-format tree: the CPU statement of the device's glrtx_trace_rays (include/glrtx.h), with the same semantics, bit for bit.
 * rays: n x 8 floats {ox, oy, oz, tmin, dx, dy, dz, tmax}; hits_out: n x 4 words {t (float), tri (int32: the wire triangle index, -1 on a miss), u, v}.
 * flags: GLRT_TRACE_CLOSEST (the smallest t in (tmin, tmax); ties to the first triangle of the renderer's visiting order) or GLRT_TRACE_ANY (the first
 * accepted hit in that order).  A hit is what the renderer's triangle test accepts (|det| >= 1e-4) with t > tmin and t below the running limit, which starts
 * at tmax and also culls boxes; on a miss t = tmax, tri = -1, u = v = 0.  A ray with a NaN or infinite component, a zero direction or tmax <= tmin is not
 * searched (the miss record); denormal components are read as zeros of their sign (a denormal tmax is the limit 0, and is echoed as 0).  Runs with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 * n_nodes = 0: every ray misses.  GLRT_HOST_EINVAL: an unknown flag, NULL arrays with n > 0, a malformed tree (a child or leaf triangle out of range, a
 * node reached twice); GLRT_HOST_EINDEX: a reachable triangle with a vertex index out of range.  n = 0 succeeds and does nothing. */
#define GLRT_TRACE_CLOSEST 0
#define GLRT_TRACE_ANY 1
int glrt_trace_rays(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *rays, size_t n,
                    float *hits_out, int flags);

/* The feature pass: the CPU statement of the device's glrtx_render_features (include/glrtx.h "Denoising"), bit for bit.  Per pixel of the rows that rank
 * `rank` of `world` owns under `stripe`-row stripes (rank 0 of 1: the whole image), in the device's local row order: the primary ray through the pixel's
 * centre (the renderer's camera ray with both random numbers 0.5 and no thin lens; c2w / s2c: glrtx_params' matrices), its closest hit by glrt_trace_rays'
 * walker with tmin 1e-4 and tmax 1e8, and there
 *   out_n: {nx, ny, nz, t}   the renderer's shading normal (a NaN component stored as 0x7FC00000) and the hit distance; {0, 0, 0, 0} on a miss;
 *   out_a: {r, g, b, id}     param0 of a diffuse material (type 2), {1, 1, 1} for every other type and on a miss; id: the material index as int32 bits, -1 on a miss.
 * Both rows x width x 4 floats, rows packed.  mat: n_mat x GLRT_MATERIAL_FLOATS.  Errors: glrt_trace_rays', and GLRT_HOST_EINDEX for a material index out of range. */
int glrt_render_features(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                         const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, float *out_n, float *out_a);
/* The feature pass with the geometry plane: the CPU statement of the device's feature pass under glrtx_track_motion (include/glrtx.h "Reprojection across a
 * geometry move").  out_n / out_a as glrt_render_features writes them, bit for bit, and
 *   out_g: {tri, u, v, 0}    the walker's own hit: the wire triangle index as int32 bits and its barycentrics (glrt_trace_rays' words); {-1, 0, 0, 0} on a miss.
 * GLRT_HOST_EINVAL for a NULL out_g; otherwise glrt_render_features' errors. */
int glrt_render_features_geom(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                              const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, float *out_n, float *out_a, float *out_g);
/* The edge-avoiding a-trous filter: the CPU statement of the device's glrtx_denoise / glrtx_debug_denoise (include/glrtx.h "Denoising": the formulas are
 * there), bit for bit.  accum: float4(rgb sum, count); normal_depth / albedo_id: the two feature planes; out: float4(rgb, 1); all width x rows x 4 floats, rows
 * packed.  GLRT_HOST_EINVAL: a NULL array, a size outside 1..65536, iterations outside 1..6, a sigma that is not a positive finite number. */
int glrt_denoise_atrous(const float *accum, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations, float sigma_color,
                        float sigma_normal, float sigma_depth, int demodulate, float *out);
/* Variance guidance: the CPU statements of glrtx_render_moments' fold, of the variance pass and of glrtx_denoise_variance / glrtx_debug_denoise_variance
 * (include/glrtx.h "Variance guidance": the formulas are there), bit for bit (host/variance.cpp; tests/variance_math.py states them in numpy).  All images are
 * width x rows x 4 floats, rows packed; V0 is width x rows floats.  They run with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 *   glrt_fold_moments       folds n_planes sample planes (plane k at planes + k * width * rows * 4), in order, into `moments` in place:
 *                           l = (0.2126 r + 0.7152 g) + 0.0722 b;  M.x += l;  M.y += l * l;  M.w += 1.  n_planes = 0 changes nothing.
 *   glrt_variance_estimate  V0 from the accumulator, M and the feature planes.
 *   glrt_denoise_variance   the variance pass, then the filter; out: float4(rgb, 1); out_v0 (may be NULL): V0.
 * GLRT_HOST_EINVAL: a NULL array, a size outside 1..65536, a negative n_planes, iterations outside 1..6, a sigma that is not a positive finite number. */
int glrt_fold_moments(float *moments, const float *planes, int n_planes, int width, int rows);
int glrt_variance_estimate(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows, float sigma_normal,
                           float sigma_depth, int demodulate, float *out_v0);
int glrt_denoise_variance(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows, int iterations,
                          float sigma_lum, float sigma_normal, float sigma_depth, int demodulate, float *out, float *out_v0);
/* The selection of glrtx_render_adaptive_moments / glrtx_debug_adaptive_select_moments (include/glrtx.h "Adaptive sampling by variance": the formulas are
 * there), bit for bit (host/variance.cpp; tests/adaptive_moments_math.py states it in numpy).  moments: width x rows x 4 floats, rows packed; mask_out: a byte
 * (0 / 1) per 8x8 tile, ceil(width / 8) x ceil(rows / 8), row-major; err_out (may be NULL): E per tile, a NaN as 0x7FC00000.  Runs with denormals flushed.
 * GLRT_HOST_EINVAL: a NULL moments or mask_out, a size outside 1..65536. */
int glrt_adaptive_select_moments(const float *moments, int width, int rows, float threshold, int min_samples, uint8_t *mask_out, float *err_out);

/* Firefly re-weighting: the CPU statements of glrtx_render_cascades' fold and of glrtx_reweight / glrtx_debug_reweight (include/glrtx.h "Firefly
 * re-weighting": the formulas are there), bit for bit (host/reweight.cpp; tests/reweight_math.py states them in numpy).  cascades: the six planes C_0 .. C_5
 * back to back, each width x rows x 4 floats {sum w r, sum w g, sum w b, count}, rows packed.  They run with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 *   glrt_fold_cascades  folds n_planes sample planes (plane k at planes + k * width * rows * 4), in order, into `cascades` in place and -- like the device's
 *                       pass, after the cascades' own update -- into `accum` (width x rows x 4 floats {rgb sum, count}; may be NULL).  n_planes = 0 changes nothing.
 *   glrt_reweight       the resolve: out, width x rows x 4 floats {rgb, 1}; a NaN is stored as 0x7FC00000.
 * GLRT_HOST_EINVAL: a NULL array, a size outside 1..65536, a negative n_planes, a start outside 2^-20 .. 2^20 (a NaN included), a kappa that is not a positive
 * finite number. */
#define GLRT_CASCADES 6
int glrt_fold_cascades(float *cascades, float *accum, const float *planes, int n_planes, int width, int rows, float start);
int glrt_reweight(const float *cascades, int width, int rows, float kappa, float *out);

/* Temporal reprojection: the CPU statement of the device's glrtx_reproject / glrtx_debug_reproject (include/glrtx.h "Reprojection": the formulas are there), bit
 * for bit.  accum / n0 / a0: the old view's accumulator float4(rgb sum, count) and feature planes; n1 / a1: the new view's planes; out: the new accumulator; all
 * width x rows x 4 floats, rows packed.  c2w_prev / s2c_prev: the camera of the old view (inverted here with glrt_mat4_inverse's routine); c2w_cur / s2c_cur: the
 * new view's.  carried / hit_pixels (may be NULL): pixels that carried history over, pixels of the new view with a hit.  Runs with denormals flushed (MXCSR
 * FTZ | DAZ, restored on return).  GLRT_HOST_EINVAL: a NULL array, a size outside 1..65536, max_history < 1, a depth_tolerance that is not a positive finite
 * number, a normal_tolerance that is not finite, a singular c2w_prev or s2c_prev. */
int glrt_reproject(const float *accum, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev, const float *s2c_prev,
                   const float *c2w_cur, const float *s2c_cur, int width, int rows, int max_history, float depth_tolerance, float normal_tolerance, float *out,
                   int *carried, int *hit_pixels);
/* Reprojection across a geometry move: the CPU statement of the device's glrtx_reproject_motion / glrtx_debug_reproject_motion (include/glrtx.h "Reprojection
 * across a geometry move": the formulas are there), bit for bit.  accum / n0 / a0: the old view; g1 / a1: the new view's geometry and albedo planes (the new
 * view's camera enters through them alone); vert_prev (n_vert x GLRT_VERTEX_FLOATS): the vertices as they stood at the old view; tri (n_tri x 4): the wire
 * triangles.  Everything else as glrt_reproject.  The edges p1 - p0, p2 - p0 of the previous triangles are formed with denormals kept, as the scene upload
 * forms them; the per-pixel arithmetic runs with denormals flushed.  Errors: glrt_reproject's; GLRT_HOST_EINDEX for a triangle with a vertex index out of range. */
int glrt_reproject_motion(const float *accum, const float *n0, const float *a0, const float *g1, const float *a1, const float *vert_prev, size_t n_vert,
                          const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width, int rows, int max_history,
                          float depth_tolerance, float normal_tolerance, float *out, int *carried, int *hit_pixels);

/* The moments plane M through the two reprojections: the CPU statements of what glrtx_reproject / glrtx_reproject_motion write into the second M while
 * glrtx_track_moments is on, and of glrtx_debug_reproject_moments / glrtx_debug_reproject_motion_moments (include/glrtx.h "Variance guidance": "Carrying M";
 * host/reproject_moments.h holds the shared steps), bit for bit.  glrt_reproject / glrt_reproject_motion with two more arrays: moments (the old view's M) and
 * moments_out (the new view's), width x rows x 4 floats each; `out`, carried and hit_pixels are what those calls give, bit for bit.  GLRT_HOST_EINVAL also for a
 * NULL moments or moments_out. */
int glrt_reproject_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev,
                           const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows, int max_history, float depth_tolerance,
                           float normal_tolerance, float *out, float *moments_out, int *carried, int *hit_pixels);
int glrt_reproject_motion_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *g1, const float *a1,
                                  const float *vert_prev, size_t n_vert, const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width,
                                  int rows, int max_history, float depth_tolerance, float normal_tolerance, float *out, float *moments_out, int *carried,
                                  int *hit_pixels);

/* Tone mapping: the CPU statements of the device's glrtx_exposure_measure and of glrtx_tonemap / glrtx_resolve_tonemapped_rgba8 (include/glrtx.h "Tone mapping":
 * the formulas are there), bit for bit (host/tonemap.cpp; tests/tonemap_math.py states them in numpy).  src: width x rows x 4 floats {rgb sum, count}, rows
 * packed.  They run with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 *   glrt_exposure_measure   one measurement: hist_out (256 counts), counted = N, kept = K, mean_log2, target and the new E in exposure_out (each but hist_out may
 *                           be NULL).  exposure_in: the previous E, or NULL for a first measurement (E = target).
 *   glrt_tonemap            the curve with s = auto_exposure ? E * exposure : exposure into t_out (width x rows x 4 floats, {y, 1}), and the resolve of that
 *                           plane -- clamp, gamma, rounding, rows flipped with flip_y -- into rgba8_out (width x rows x 4 bytes); either may be NULL.
 * GLRT_HOST_EINVAL: a NULL src or hist_out, a size outside 1..65536, and what glrtx_tonemap_cfg's checks refuse (key, adapt, the window; op, exposure, white, gamma). */
int glrt_exposure_measure(const float *src, int width, int rows, float key, int low_permille, int high_permille, float adapt, const float *exposure_in,
                          uint32_t *hist_out, uint64_t *counted, uint64_t *kept, float *mean_log2, float *target, float *exposure_out);
int glrt_tonemap(const float *src, int width, int rows, int op, int auto_exposure, float exposure, float E, float white, float gamma, int flip_y, float *t_out,
                 uint8_t *rgba8_out);

/* Bloom: the CPU statement of the device's glrtx_bloom / glrtx_debug_bloom (include/glrtx.h "Bloom": the formulas are there), bit for bit (host/bloom.cpp;
 * tests/bloom_math.py states them in numpy).  src: width x rows x 4 floats {rgb sum, count}, rows packed; threshold, strength and levels are glrtx_bloom_cfg's
 * (its source has no meaning here).  d_out: the planes D_1 .. D_levels back to back, 4 floats a texel {rgb, 0} (the sum of w_k * h_k texels, w_{k+1} =
 * (w_k + 1) >> 1); b_out: width x rows x 4 floats {x + strength * glow, 1}; either may be NULL.  Runs with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 * GLRT_HOST_EINVAL: a NULL src, a size outside 1..65536, levels outside 1..8, a threshold that is not finite and >= 0, a strength outside [0, 1e4]. */
int glrt_bloom(const float *src, int width, int rows, float threshold, float strength, int levels, float *d_out, float *b_out);

/* Posing: the CPU statement of the device's skinning pass (glrtx_pose / glrtx_debug_skin, include/glrtx.h "Posing": the arithmetic is there), bit for bit
 * (host/deform.cpp; tests/skin_math.py states it in numpy).  rest_vert: n_vert wire vertices of GLRT_VERTEX_FLOATS floats; bones4 / weights4: four bone indices and
 * four weights a vertex; matrices: n_bones x 12 floats, row-major 3x4; vert_out: n_vert wire vertices (may not overlap the inputs).  Runs with denormals flushed
 * (MXCSR FTZ | DAZ, restored on return).  Weights and matrices are NOT checked for finiteness here: the statement covers whatever the kernel can be handed.
 * GLRT_HOST_EINVAL: a NULL pointer (with n_vert > 0; matrices always), n_bones outside 1..GLRT_MAX_BONES, a bone index outside [0, n_bones). */
#define GLRT_MAX_BONES 65536
int glrt_skin_vertices(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *matrices, int n_bones,
                       float *vert_out);

/* Deforming: the CPU statement of the device's deform pass (glrtx_pose_morph / glrtx_pose_dualquat / glrtx_debug_deform, include/glrtx.h "Deforming": the
 * arithmetic is there), bit for bit (host/deform.cpp; tests/deform_math.py states it in numpy).  The rig is glrt_skin_vertices'; bone_data: mode 0, n_bones x 12
 * floats (matrices); mode 1, n_bones x 8 floats {r.x, r.y, r.z, r.w, d.x, d.y, d.z, d.w} (dual quaternions); deltas: n_targets x n_vert x 6 floats {dpos,
 * dnormal}, target-major; morph_weights: n_targets floats.  A target whose weight is a zero or a denormal is not read.  Runs with denormals flushed (MXCSR FTZ |
 * DAZ, restored on return).  Bone weights, bone data and deltas are NOT checked for finiteness.  GLRT_HOST_EINVAL: what glrt_skin_vertices refuses, a mode other
 * than 0 and 1, n_targets outside 0..GLRT_MAX_MORPH_TARGETS, NULL deltas or morph_weights with n_targets > 0, a morph weight that is not finite. */
#define GLRT_MAX_MORPH_TARGETS 64
int glrt_deform_vertices(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                         const float *deltas, const float *morph_weights, int n_targets, float *vert_out);
/* Sparse targets (include/glrtx.h "Deforming", SPARSE TARGETS: the wire form and the rules are there).  glrt_deform_vertices_sparse is glrt_deform_vertices over
 * a sparse set -- offsets[n_targets + 1], vertex[nnz], deltas[nnz x 6], n_targets <= GLRT_MAX_SPARSE_MORPH_TARGETS --, bit for bit the device's
 * deform_sparse_kernel; it runs under FTZ | DAZ and validates exactly as glrtx_upload_morph_targets_sparse does.  GLRT_HOST_EINVAL: what glrt_deform_vertices
 * refuses about the rig, the mode and the morph weights, n_targets outside 0..1024, a NULL array with entries to read (n_targets == 0 needs no array; nnz == 0
 * needs no vertex and no deltas), offsets[0] != 0, decreasing offsets, nnz >= 2^31, an index >= n_vert, indices not strictly ascending inside a target.
 * glrt_morph_sparsify makes a sparse set from dense deltas (n_targets x n_vert x 6, n_targets <= 1024 here): entry (k, v) is kept iff some component of its six
 * floats has a non-zero exponent field (a normal number, an Inf or a NaN).  It always fills offsets[n_targets + 1]; with vertex_out == NULL it only counts, so a
 * caller calls it twice: once for offsets[n_targets] = nnz, once with vertex_out[nnz] and deltas_out[nnz x 6]. */
#define GLRT_MAX_SPARSE_MORPH_TARGETS 1024
int glrt_deform_vertices_sparse(const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                                const uint64_t *offsets, const uint32_t *vertex, const float *deltas, const float *morph_weights, int n_targets, float *vert_out);
int glrt_morph_sparsify(const float *dense_deltas, int n_targets, size_t n_vert, uint64_t *offsets, uint32_t *vertex_out, float *deltas_out);
/* The dual quaternion {r.x, r.y, r.z, r.w, d.x, d.y, d.z, d.w} of a rigid 3x4 matrix (row-major; the rotation is taken as orthonormal): computed in double and
 * rounded once, with the sign that makes r.w >= 0.  d = 1/2 (t, 0) * r. */
void glrt_dualquat_from_matrix(const float m[12], float dq[8]);

/* Rebuilding normals: the CPU statements of the device's normal rebuild (glrtx_update_positions / glrtx_set_pose_normals / glrtx_debug_rebuild_normals,
 * include/glrtx.h "Rebuilding normals": the weld rule, the orientation rule and the arithmetic are there), bit for bit (host/normals.cpp, host/normal_topology.h;
 * tests/normals_math.py states them in numpy).  rest_vert / vert_inout: n_vert wire vertices of GLRT_VERTEX_FLOATS floats; tri: n_tri x 4 floats {i0, i1, i2,
 * material} as glrt_bvh_build_* take them.  The arithmetic runs with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 *   glrt_normal_topology        class_of_vertex_out[n_vert]: the weld class of every vertex, ids ascending with each class's smallest member (so the map is a
 *                               function of the input alone); flip_out[n_tri]: 1 for a triangle wound against its rest normals, else 0; n_classes_out may be
 *                               NULL.  flags: 0, or GLRT_NORMALS_WELD_POSITIONS to weld by position alone.
 *   glrt_rebuild_normals        rebuilds the normal words of vert_inout in place from its position words; every other word is left as it is.  class_of_vertex may
 *                               be any map with ids below n_vert (the rows of ids no vertex carries are empty); flip is n_tri bytes, zero or not.
 *   glrt_positions_to_vertices  vert_out = the rest records with their three position words replaced by pos (n_vert x 3 floats), moved as integers (vert_out may
 *                               not overlap the inputs).
 * GLRT_HOST_EINVAL: a NULL pointer with something to read or write, n_vert or n_tri >= 2^31, a corner index that is not an integer in [0, n_vert), an unknown
 * flag, a class id >= n_vert. */
#define GLRT_NORMALS_WELD_POSITIONS 1u
#define GLRT_NORMAL_CHUNK 256u
int glrt_normal_topology(const float *rest_vert, size_t n_vert, const float *tri, size_t n_tri, unsigned flags, uint32_t *class_of_vertex_out, uint8_t *flip_out,
                         size_t *n_classes_out);
int glrt_rebuild_normals(float *vert_inout, size_t n_vert, const float *tri, size_t n_tri, const uint32_t *class_of_vertex, const uint8_t *flip);
int glrt_positions_to_vertices(const float *rest_vert, const float *pos, size_t n_vert, float *vert_out);

/* Textures: the CPU statements of the device's texture lookup (glrtx_upload_textures / glrtx_debug_texture_lookup, include/glrtx.h "Textures": the set, the
 * formats, the coordinate and filter rules are there), bit for bit (host/texture.cpp; tests/texture_math.py states them in numpy).  glrt_texture is
 * glrtx_texture's layout and the GLRT_TEX_* values are the GLRTX_TEX_* ones.  The arithmetic runs with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 *   glrt_texture_lookup   rgb_out[3i..3i+2] = the lookup in texture which[i] at (st[2i], st[2i+1]).
 *   glrt_srgb_table       the 256 floats GLRT_TEX_RGBA8_SRGB decodes a byte with.
 *   glrt_texture_albedo   what plane A of the feature pass holds (rgb) for hit records as plane G stores them (hits: n x {wire triangle as int32 bits, u, v, 0}),
 *                         on the wire-format scene with material m bound to texture material_texture[m] (-1: none): the lookup at the interpolated
 *                         coordinates for a bound diffuse material, param0 for an unbound diffuse one, {1, 1, 1} otherwise and on a miss.
 * GLRT_HOST_EINVAL: a NULL pointer with something to read or write, or a set glrtx_upload_textures refuses.  GLRT_HOST_EINDEX: a texture, triangle, vertex or
 * material index out of range, or a binding on a material that is not diffuse. */
#define GLRT_TEX_RGBA32F 0
#define GLRT_TEX_RGBA8_UNORM 1
#define GLRT_TEX_RGBA8_SRGB 2
#define GLRT_TEX_REPEAT 0
#define GLRT_TEX_CLAMP 1
#define GLRT_TEX_NEAREST 0
#define GLRT_TEX_BILINEAR 1
typedef struct glrt_texture {
    uint64_t offset;
    int32_t width, height, format, wrap_s, wrap_t, filter;
} glrt_texture;
int glrt_texture_lookup(const glrt_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const float *st, size_t n,
                        float *rgb_out);
const float *glrt_srgb_table(void);
int glrt_texture_albedo(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat, const glrt_texture *tex, size_t n_tex,
                        const void *texels, size_t texel_bytes, const int32_t *material_texture, const float *hits, size_t n, float *rgb_out);

/* Cutouts: the CPU statements of the device's alpha test (glrtx_bind_cutouts / glrtx_debug_texture_channel, include/glrtx.h "Cutouts": the rule is there), bit
 * for bit (host/texture.cpp, host/query.cpp, host/features.cpp; tests/cutout_math.py states the lookup in numpy).  glrt_cutout is glrtx_cutout's layout.
 *   glrt_texture_channel  value_out[i] = channel channel[i] (0 .. 3) of the lookup in texture which[i] at (st[2i], st[2i+1]): channels 0 .. 2 are
 *                         glrt_texture_lookup's words; channel 3 is the texel's fourth float, or byte / 255.0f for both 8-bit formats, through the same filter.
 *   glrt_render_features_geom_cutout   glrt_render_features_geom with the set, the per-material bindings and one cutout record a material: the closest-hit
 *                         search rejects a candidate that would become the closest hit where its material's record says so (value >= cutoff accepts, a
 *                         NaN rejects; a record with texture -1 cuts nothing), and plane A carries the looked-up albedo of a bound diffuse material, as the
 *                         device's textured feature kernels write it.  With every record -1 and every binding -1 it is glrt_render_features_geom.
 *                         glrt_trace_rays and glrt_render_features_geom themselves are unchanged: queries stay geometric.
 * GLRT_HOST_EINVAL: a NULL pointer with something to read or write, a set glrtx_upload_textures refuses, a cutoff that is not finite, reserved non-zero, a
 * cutout on a material that is neither diffuse nor conductor.  GLRT_HOST_EINDEX: a texture or channel index out of range, a binding on a material that is not
 * diffuse; otherwise glrt_render_features_geom's errors. */
typedef struct glrt_cutout { int32_t texture, channel; float cutoff; int32_t reserved; } glrt_cutout;
int glrt_texture_channel(const glrt_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const int32_t *channel, const float *st,
                         size_t n, float *value_out);
int glrt_render_features_geom_cutout(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *nodes, size_t n_nodes, const float *mat, size_t n_mat,
                                     const float *c2w, const float *s2c, int width, int height, int rank, int world, int stripe, const glrt_texture *tex, size_t n_tex,
                                     const void *texels, size_t texel_bytes, const int32_t *material_texture, const glrt_cutout *cut, float *out_n, float *out_a,
                                     float *out_g);

/* Emission maps: the CPU statements of the device's textured emitters (glrtx_bind_emission_maps / glrtx_debug_light_emission, include/glrtx.h "Emission
 * maps": the rule is there), bit for bit (host/texture.cpp; tests/emission_math.py states the sampled side in numpy).  light: n_light x 4 floats {i0, i1, i2,
 * material}, the wire's light records.  material_emission: one texture index a material, -1 none.
 *   glrt_light_st         st_out[6l ..] = {s0, t0, s1, t1, s2, t2}: words 6 and 7 of light l's three vertices in wire order -- the device's light_st table.
 *   glrt_light_emission   out[5i ..] = {s, t, Le.rgb} of light lid[i] at the RAW uniforms (u[2i], u[2i + 1]): the flip at ua0 + ub0 > 1, w0 = (1 - ua) - ub,
 *                         s = (w0 * s0 + ua * s1) + ub * s2, t likewise, Le = emission * lookup(s, t) per channel (one rounded product); a light whose material
 *                         is not bound gives its plain emission.
 *   glrt_emission_albedo  glrt_texture_albedo, then rgb_out again for a hit on a bound material that is NOT diffuse: the looked-up texel c, without the
 *                         emission -- plane A of the device's feature pass while emission maps are bound, stated on plane G (hits).
 *   glrt_emission_bind_check  what glrtx_bind_emission_maps refuses of a scene with n_scene_mat materials and a set of n_tex textures (cutouts_bound: cutouts
 *                         are bound): GLRT_HOST_EINVAL and the device's message behind its "glrtx_bind_emission_maps: " in msg (cap bytes), or
 *                         GLRT_HOST_OK and "".
 * GLRT_HOST_EINVAL: a NULL pointer with something to read or write, a set glrtx_upload_textures refuses.  GLRT_HOST_EINDEX: a texture, vertex, material or
 * light index out of range, a binding on a material of type 5; otherwise glrt_texture_albedo's errors. */
int glrt_light_st(const float *vert, size_t n_vert, const float *light, size_t n_light, float *st_out);
int glrt_light_emission(const float *vert, size_t n_vert, const float *light, size_t n_light, const float *mat, size_t n_mat, const glrt_texture *tex, size_t n_tex,
                        const void *texels, size_t texel_bytes, const int32_t *material_emission, const int32_t *lid, const float *u, size_t n, float *out);
int glrt_emission_albedo(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat, const glrt_texture *tex, size_t n_tex,
                         const void *texels, size_t texel_bytes, const int32_t *material_texture, const int32_t *material_emission, const float *hits, size_t n,
                         float *rgb_out);
int glrt_emission_bind_check(const float *mat, size_t n_scene_mat, size_t n_tex, int cutouts_bound, const int32_t *material_emission, size_t n_mat, char *msg,
                             size_t cap);

/* A launch's route: which kernel a render call of a device context runs and what glrtx_stats reports about it, or why the call refuses -- the device layer's
 * own statement (host/route_statement.h; DESIGN.md "A launch's route"), as a function of the context fields and parameters that decide it.
 *   state   the context as the call finds it: n_spheres, n_tex and n_vine are counts (n_vine > 0: the uploaded tree is a vine), the have_* fields and the
 *           two switches are 0 or 1 -- vol_switch / tex_switch: glrtx_set_volume_wavefront / glrtx_set_texture_wavefront, or what GLRTX_VOLUME_WAVEFRONT /
 *           GLRTX_TEXTURE_WAVEFRONT put in their place.
 *   kind    the call: glrtx_render and glrtx_render_frames, glrtx_render_adaptive, glrtx_render_moments, glrtx_hit_histogram,
 *           glrtx_render_adaptive_moments, glrtx_render_cascades.
 * GLRT_HOST_OK: *route_out holds the kernel family (= variant_last), fallback_last, whether the launch counts in fallback_launches, the row of the family's
 * table of forms and the kernel's name as glrtx_debug_last_kernel gives it; msg is "".  GLRT_HOST_EINVAL: the call refuses, msg (cap bytes) holds the device's
 * message behind its "<function>: ", *route_out is zeroed.  GLRT_HOST_EINDEX: a NULL state or route_out, or no such kind. */
#define GLRT_ROUTE_ORDINARY 0
#define GLRT_ROUTE_ADAPTIVE 1
#define GLRT_ROUTE_MOMENTS 2
#define GLRT_ROUTE_CALIBRATION 3
#define GLRT_ROUTE_ADAPTIVE_MOMENTS 4
#define GLRT_ROUTE_CASCADES 5
typedef struct glrt_route_state {
    int32_t variant, ext_flags, n_spheres, n_tex, n_vine, have_volume, have_maps, have_cut, have_emit, have_env, vol_switch, tex_switch, max_depth, n_samples;
} glrt_route_state;
typedef struct glrt_route { int32_t family, variant_last, fallback_last, fallback_counts, form; char kernel[96]; } glrt_route;
int glrt_launch_route(const glrt_route_state *state, int kind, glrt_route *route_out, char *msg, size_t cap);

/* Surface context: the three lookups above -- the albedo of "Textures", the acceptance of "Cutouts", the texel of "Emission maps" -- as per-hit calls with C
 * linkage, for a CPU path tracer that takes them as callbacks (oracle/pt_oracle.c: pt_oracle_set_surface).  The lookups stay stated once: the calls are built
 * on the statements behind glrt_texture_lookup and glrt_texture_channel and mix the coordinates as glrt_texture_albedo and glrt_light_emission do,
 * s = (w0 * s0 + u * s1) + v * s2 with w0 = (1 - u) - v.
 *   glrt_surface_create    checks the wire scene (vert, tri, light, mat), the set and the three kinds of per-material bindings -- material_texture and
 *                          material_emission one texture index a material (-1: none), cut one record a material; each may be NULL: nothing of that kind is
 *                          bound -- and copies what the calls read: the coordinates are those of `vert` at this call, as the device's tables are the upload's.
 *   glrt_surface_free      releases a context (NULL: nothing).
 *   glrt_surface_albedo    1 and rgb = the lookup at (u, v) of wire triangle tri where its material is bound to a texture; 0, rgb untouched, otherwise.
 *   glrt_surface_accept    0 where wire triangle tri's material has a cutout record and the channel's value at (u, v) is not >= cutoff (a NaN rejects); else 1.
 *   glrt_surface_emission  1 and texel = the lookup c (Le = emission * c is the caller's product) where the material is bound to an emission map; 0 otherwise.
 *                          light == 0: index is a wire triangle and (u, v) the hit's; light != 0: index is a light and (u, v) sampleDirect's flipped uniforms.
 * The per-hit calls take the context as void *, only read it, and flush denormals for their own duration: any number of threads may call them at once.  An
 * index outside the scene is unbound (albedo, emission: 0; accept: 1); any float is a valid u or v.
 * GLRT_HOST_EINVAL / GLRT_HOST_EINDEX: as glrt_texture_albedo, glrt_render_features_geom_cutout and glrt_light_emission refuse the same arguments. */
typedef struct glrt_surface glrt_surface;
int glrt_surface_create(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *light, size_t n_light, const float *mat, size_t n_mat,
                        const glrt_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *material_texture, const glrt_cutout *cut,
                        const int32_t *material_emission, glrt_surface **surface_out);
void glrt_surface_free(glrt_surface *surface);
int glrt_surface_albedo(void *surface, int tri, float u, float v, float rgb[3]);
int glrt_surface_accept(void *surface, int tri, float u, float v);
int glrt_surface_emission(void *surface, int index, int light, float u, float v, float texel[3]);

/* Environment: the CPU statements of the device's environment lighting (glrtx_upload_environment / glrtx_debug_env_*, include/glrtx.h "Environment": the
 * octahedral mapping, its inverse, the solid-angle factor, the importance grid and the sampling rule are there), bit for bit (host/environment.cpp;
 * tests/env_math.py states them in numpy).  glrt_env_cfg is glrtx_env_cfg's layout.  The arithmetic runs with denormals flushed (MXCSR FTZ | DAZ, restored).
 *   glrt_env_weights       weights_out[j * G + i] = the weight of cell (row j, column i) of the G x G importance grid, in the device's summation order;
 *                          *grid_out = G (cfg.grid, or min(N, 256) for 0).  weights_out holds 1024 * 1024 floats at most.
 *   glrt_env_alias         the five tables of a G x G grid of weights (Vose's method in float64, thresholds rounded once to fp32): row_q / row_alias [G],
 *                          col_q / col_alias / cell_p [G * G].
 *   glrt_env_sample        out[8i..] = {direction, pdf, Le.rgb, 0} of the six uniforms u[6i..], with p_env = cfg.light_pick.
 *   glrt_env_eval          out[4i..] = {Le.rgb, pdf} of the direction dir[3i..].
 *   glrt_env_from_latlong  resamples a lat-long image (height rows of width RGB float triples; +y is up, the top row is +y, the centre column is -z, +x lies
 *                          to its right) into an n x n octahedral RGBA32F map (alpha 1): evaluated at the texel centres with bilinear taps in float64, the
 *                          columns wrapping, the rows clamped.  Not a device statement: it prepares an input.
 * GLRT_HOST_EINVAL: a NULL pointer with something to read or write, or a map or configuration glrtx_upload_environment refuses. */
typedef struct glrt_env_cfg { int32_t mode; int32_t grid; float light_pick; float scale[3]; float rotation[9]; } glrt_env_cfg;
int glrt_env_weights(const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg, float *weights_out, int32_t *grid_out);
int glrt_env_alias(const float *weights, int32_t grid, float *row_q, int32_t *row_alias, float *col_q, int32_t *col_alias, float *cell_p);
int glrt_env_sample(const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg, const float *u, size_t n, float *out);
int glrt_env_eval(const glrt_texture *map, const void *texels, size_t texel_bytes, const glrt_env_cfg *cfg, const float *dir, size_t n, float *out);
int glrt_env_from_latlong(const float *rgb, int32_t width, int32_t height, int32_t n, float *rgba_out);

/* Material maps: the CPU statements of the device's tangent-space normal rule and roughness rule (glrtx_bind_material_maps / glrtx_debug_map_normal,
 * include/glrtx.h "Material maps": decode, frame, perturbation and the cases that keep the normal are there), bit for bit (host/maps.cpp; tests/maps_math.py
 * states them in numpy).  glrt_material_map is glrtx_material_map's layout.  The arithmetic runs with denormals flushed (MXCSR FTZ | DAZ, restored on return).
 *   glrt_map_decode   m_out[3i..] = rgb[3i..] * 2 + -1: a looked-up texel as the tangent-space vector.
 *   glrt_map_normal   normal_out[3i..] = n' of record i: GLRT_MAP_RECORD_FLOATS floats {n, e1, e2, (s0, t0), (s1, t1), (s2, t2), m}, m decoded.
 *   glrt_map_alpha    alpha_out[2i..] = (ax, ay) of the roughness texel rgb[3i..]: channels r and g, floored at GLRT_MAP_ALPHA_MIN.
 * GLRT_HOST_EINVAL: a NULL pointer with something to read or write. */
#define GLRT_MAP_ALPHA_MIN 1e-3f
#define GLRT_MAP_RECORD_FLOATS 18
typedef struct glrt_material_map { int32_t normal, roughness; float normal_scale; int32_t reserved; } glrt_material_map;
int glrt_map_decode(const float *rgb, size_t n, float *m_out);
int glrt_map_normal(const float *records, size_t n, float scale, float *normal_out);
int glrt_map_alpha(const float *rgb, size_t n, float *alpha_out);

void glrt_look_at(const float eye[3], const float center[3], const float up[3], float out[16]);
void glrt_perspective(float fovy_deg, float aspect, float z_near, float z_far, float out[16]);
void glrt_mat4_mul(const float a[16], const float b[16], float out[16]);
/* returns 0, or GLRT_HOST_EINVAL for a singular matrix */
int glrt_mat4_inverse(const float m[16], float out[16]);
/* frame f -> (fract(0.137 + 0.6180340 f), fract(0.731 + 0.3819660 f)) */
void glrt_frame_seed(uint32_t frame, float out[2]);

#ifdef __cplusplus
}
#endif
#endif
