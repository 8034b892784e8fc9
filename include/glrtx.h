/*
 * glrtx.h -- C ABI of libglrtx.so, the MI355X (gfx950) device layer that replaces the
 * GL side of tatsy/opengl-raytracer's per-pixel path-tracing pass.
 *
 * Drop-in boundary.  What each entry point replaces in the reference:
 *
 *   glrtx_create / glrtx_destroy     GL context + program setup: Window::Window, Window::initialize
 *                                    src/core/window.cpp:30-81, :185-211
 *   glrtx_upload_scene               the five TextureBuffer(size, fmt, usage) + setData(ptr) uploads
 *                                    src/core/scene.cpp:254-269, src/core/texture_buffer.h:8-12
 *                                    (byte layouts unchanged: scene.h:16-35, trimesh.h:15-25, bvh.h:84-100)
 *   glrtx_build_lbvh                 BVH::construct, src/core/bvh.cpp:59-160 (device-side linear BVH instead)
 *   glrtx_resize                     Window::resize -> resetBuffer (accumulators re-created, cleared)
 *                                    src/core/window.cpp:324-335, :366-381
 *   glrtx_clear                      glClear of the accumulation targets on reset (same lines)
 *   glrtx_render                     first half of Window::render(): uniform upload + the single
 *                                    glDrawArrays(GL_TRIANGLES, 0, 6) that runs raytrace.frag on every pixel
 *                                    src/core/window.cpp:213-295; shader src/shaders/raytrace.frag:565-614
 *   glrtx_render_frames              n consecutive iterations of the accumulation loop in Window::mainloop
 *                                    (src/core/window.cpp:121-169 calling render(), with the fresh u_seed of
 *                                    :226-238 per frame and a static camera), issued as one launch
 *   glrtx_params                     the uniforms set per frame, window.cpp:230-243, plus u_maxDepth which
 *                                    the reference leaves at its shader default 16 (raytrace.frag:47)
 *   glrtx_read_accum                 reading fbo[select] colour attachments 0/1 (RGB32F + R32F)
 *                                    src/core/window.cpp:366-381; fused here into float4(L.rgb, count)
 *   glrtx_resolve_rgba8              second half of Window::render() (screen.frag: rgb/count, clamp, gamma)
 *                                    + saveCurrentFrame's read-back and vertical flip
 *                                    src/shaders/screen.frag:15-25, src/core/window.cpp:297-317, :383-414
 *   glrtx_set_partition / glrtx_bind_accum / glrtx_set_stream
 *                                    no counterpart (reference is single-GPU): row-stripe sharding across
 *                                    one-process-per-GPU ranks, SURVEY.md section 8(e)
 *   glrtx_render_adaptive            no counterpart (the reference renders every pixel of every frame): glrtx_render_frames restricted
 *                                    to the 8x8 tiles that have not converged yet, each rendered pixel bit-identical to the full frame's
 *   glrtx_present_*                  the screen pass and saveCurrentFrame after EVERY frame of Window::mainloop, without a sync:
 *                                    src/core/window.cpp:157-164, src/shaders/screen.frag:15-25, window.cpp:383-414
 *   glrtx_stats / glrtx_timer_*      replaces the whole-frame Timer, src/core/timer.h:7-36, window.cpp:119-168
 *   glrtx_last_error                 replaces FatalError's stderr + abort(), src/core/common.h:88-94
 *
 * Conventions: plain C, no torch / HIP types in signatures.  Host pointers are borrowed for the
 * duration of a call and copied; the ctx owns all device memory it allocates; the caller owns
 * output buffers.  Return value 0 = ok, negative = GLRTX_E*; the message is available from
 * glrtx_last_error(ctx) (ctx may be NULL for create-time failures).  One host thread drives a ctx.
 * Image rows use GL orientation: row 0 is gl_FragCoord.y = 0.5 (bottom), like the reference's FBOs.
 */
#ifndef GLRTX_H
#define GLRTX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLRTX_OK 0
#define GLRTX_EINVAL (-1)   /* bad argument / call order */
#define GLRTX_EDEVICE (-2)  /* HIP runtime error or no usable gfx950 device */
#define GLRTX_ESCENE (-3)   /* scene buffers inconsistent (index out of range, BVH not a tree) */
#define GLRTX_EDEPTH (-4)   /* BVH needs more than the 64-entry traversal stack (raytrace.frag:284) */
#define GLRTX_ENOMEM (-5)
#define GLRTX_EBUSY (-6)    /* presentation: no free ring image for this call's frames (nothing was changed: retry after glrtx_present_release), or no image ready */

#define GLRTX_ABI_VERSION 10

typedef struct glrtx_ctx glrtx_ctx;

/* Per-frame uniforms (window.cpp:230-243).  Matrices are column-major, untransposed, exactly the
 * 16 floats glUniformMatrix4fv(..., GL_FALSE, ...) receives (shader_program.cpp:151-156). */
typedef struct glrtx_params {
    float c2w[16];   /* u_c2wMat = inverse(viewM * modelM) */
    float s2c[16];   /* u_s2cMat = inverse(projM) */
    float aperture;  /* u_apertureRadius */
    float focal;     /* u_focalLength */
    float seed[2];   /* u_seed */
    int32_t n_samples; /* u_nSamples (reference host sends 1, window.cpp:239) */
    int32_t max_depth; /* u_maxDepth ("k bounces" := k) */
} glrtx_params;

typedef struct glrtx_stats {
    uint64_t rays;          /* executions of intersect(Ray, out Intersection) since last clear/reset_stats;
                               only counted by launches made while ray counting is enabled */
    uint64_t rays_untraced; /* of `rays`: shadow rays the reference traces although both outcomes of its light test give the
                               same radiance bit for bit (a cosine <= 0, or a contribution too small to register); they are
                               counted above but resolved without a traversal */
    uint64_t paths;         /* pixel samples traced (owned pixels * n_samples per launch) */
    uint64_t launches;      /* frames rendered: glrtx_render calls + frames of glrtx_render_frames calls */
    uint64_t kernel_launches; /* launches of the render kernel (one per glrtx_render / glrtx_render_frames call) */
    double kernel_ms_total; /* sum over launches of the RENDER kernel's device time (HIP events on the ctx stream) */
    double accumulate_ms_total; /* sum of the plane-accumulation passes that follow glrtx_render_frames launches */
    float kernel_ms_last;   /* render kernel of the last launch */
    int32_t frames_last;    /* frames covered by the last launch */
    int32_t width, height;  /* full image */
    int32_t owned_rows;     /* rows of this ctx's partition */
    int32_t stack_entries;  /* traversal stack entries the uploaded BVH needs */
    int32_t lds_bytes;      /* dynamic LDS per workgroup of the render kernel */
    int32_t n_tri, n_fork, n_mat, n_light;
    int32_t variant_last;   /* kernel the last launch actually ran: 2 workgroup-local wavefront, 1 persistent megakernel, 0 tile megakernel */
    int32_t fallback_last;  /* 0, or why the last launch left the selected wavefront kernel (GLRTX_FALLBACK_* bits) */
    float resolve_ms_last;  /* device time of the last resolve kernel (glrtx_resolve_rgba8), without the copy to the host */
    int32_t node_fetch_last; /* wavefront kernel, last launch: 0 = one record per lane, 1 = pair-cooperative node fetch (large trees), 2 = the two in alternate
                                steps (small trees) -- all bit-identical; GLRTX_PAIR_FETCH=0/1/2 forces one (was reserved0) */
    uint64_t fallback_launches; /* launches since reset_stats that ran on the persistent megakernel although variant 2 was selected:
                                   ~2x slower per ray and without frames in flight -- visible here instead of silent */
    int32_t pipe_slots;         /* overlapped single-frame launches (glrtx_render): internal slots the last such launch could choose from -- GLRTX_PIPE_SLOTS
                                   (default 6), less when the memory budget or a failed allocation says so, 0 when such launches run un-piped */
    int32_t pipe_resident_max;  /* ... and the most of them that had a render kernel on the device at once (counted when a launch is issued) since
                                   reset_stats: 1 means consecutive launches did not overlap, whatever the reason (queue mapping, a caller that syncs) */
    int32_t device_error_pending; /* ABI 9: 1 while a launch that FAILED on the device sits unreported in the context's launch ring: glrtx_get_stats never blocks and
                                     never consumes such a record (its rc stays GLRTX_OK and the timing fields stop advancing); the error itself -- kernel, size, frame
                                     count, device -- is returned by the next glrtx_sync, or by the launch that needs the record's slot */
    int32_t wf_state_mib;       /* (was reserved1) MiB of path state the last wavefront launch ran on: an entry per workgroup OF THAT LAUNCH and path-queue position, two
                                   sets of six float4 planes -- 768 for a full grid on a 256-CU device whatever the frames in flight (384 for an overlapped single-frame
                                   launch at 1080p), 1 for a 9x9 image (ABI 10: sized by the launch, not by the device) */
    /* ABI 10 */
    int32_t shadow_limited;     /* which shadow-ray search the context's launches run: 0 the reference's own closest-hit search (default: bit-exact contract), 1 the
                                   range-limited one (glrtx_set_shadow_range_limit / GLRTX_SHADOW_LIMIT=1: outside the bit-exact contract).  bench.py prints it */
    int32_t node_layout_last;   /* (was reserved2) wavefront kernel or ray query (glrtx_trace_rays*), last launch: 1 = the compact node array (48-byte records at breadth-first positions, three loads per step,
                                   the children located through a rank table in LDS), 0 = the 64-byte records.  The compact layout serves node_fetch_last 0 when its rank table fits
                                   in LDS with four workgroups per CU; GLRTX_COMPACT_NODES=0/1 forces it.  Bit-identical either way */
    uint64_t feed_launches;     /* fed launches since reset_stats: launches that stayed open for the calls behind them (see glrtx_render) */
    uint64_t feed_appended;     /* frames of glrtx_render / glrtx_render_frames calls that a launch already running took by itself instead of a launch of their own */
} glrtx_stats;

/* glrtx_stats.fallback_last: the wavefront kernel packs depth and sample index into one word of its path state */
#define GLRTX_FALLBACK_DEPTH 1      /* u_maxDepth > 255 */
#define GLRTX_FALLBACK_SAMPLES 2    /* u_nSamples >= 2^20 (the volume on the wavefront kernel: >= 2^16) */
#define GLRTX_FALLBACK_EXTENSIONS 4 /* analytic spheres uploaded or extension flags set (the extension kernel is a megakernel) */

int glrtx_abi_version(void);

/* device_id: HIP ordinal, or -1 for the current device. */
int glrtx_create(glrtx_ctx **out, int device_id);
void glrtx_destroy(glrtx_ctx *ctx);
const char *glrtx_last_error(const glrtx_ctx *ctx);

/* Buffers in the reference wire format; counts are in records (vertices, triangles, materials,
 * light triangles, BVH nodes).  n_light may be 0.  The scene is validated and repacked for the
 * device; it replaces any previous scene. */
int glrtx_upload_scene(glrtx_ctx *ctx, const float *vert, size_t n_vert, const float *tri, size_t n_tri,
                       const float *mat, size_t n_mat, const float *light, size_t n_light, const float *bvh,
                       size_t n_nodes);

/* Moving geometry without a rebuild.  New positions and normals for the uploaded scene's vertices (wire format, GLRT_VERTEX_FLOATS = 15 floats each; n_vert
 * must be the count the scene was uploaded with); triangles, materials, lights' vertex indices and the tree's topology stay.  Every geometry-derived device
 * buffer is rewritten on the device -- leaf and light records, normals, the fork boxes of both node layouts, the vine list, the root box -- so that the scene is
 * byte for byte what glrtx_upload_scene(new vertices, the tree refitted by glrt_bvh_refit, include/glrt_host.h) would upload.  No host repack.
 *   glrtx_update_vertices         host memory
 *   glrtx_update_vertices_device  device memory on the context's device, read on the context's stream (glrtx_set_stream): the caller orders its producer
 *                                 there, or synchronises
 * The refit runs behind every launch of this context that may still read the scene (an open fed launch is sealed, as glrtx_upload_scene does), and the call
 * returns when it has run (the root box is a kernel argument and is read back): every later launch sees the new scene.  The accumulator is NOT cleared
 * (glrtx_clear is the caller's choice); adaptive state, spheres, volume and presentation are untouched.  GLRTX_EINVAL -- no scene, NULL vertices, a count
 * other than the uploaded one -- leaves the scene unchanged. */
int glrtx_update_vertices(glrtx_ctx *ctx, const float *vert, size_t n_vert);
int glrtx_update_vertices_device(glrtx_ctx *ctx, const void *dev_vert, size_t n_vert);

/* Batched ray queries against the uploaded scene: the renderer's own traversal (the same trees, node layouts and visiting order) for rays the caller hands in.
 *   ray: 8 floats {ox, oy, oz, tmin, dx, dy, dz, tmax};  hit: 4 words {t (float), tri (int32), u (float), v (float)}.
 * A triangle counts as hit exactly when the renderer's triangle test accepts it (raytrace.frag:226-257) with t > tmin in place of t > 1e-4, and only below the
 * running search limit, which starts at tmax: a hit has tmin < t < tmax, and tmax also culls boxes.  The test keeps the renderer's rejection of |det| < 1e-4
 * (det: the edge-1 dot of the direction x edge-2 cross product), so the query sees the scene exactly as the renderer does: very small triangles, and triangles
 * seen edge-on, are never hit.  t, u, v are in the units of the direction as given (directions are not normalised); the hit point is o + t d =
 * (1 - u - v) v0 + u v1 + v v2.  tri is the triangle's index in the uploaded wire format; on a miss tri = -1, t = tmax, u = v = 0.
 *   GLRTX_TRACE_CLOSEST  the smallest t; among equal t the first triangle in the renderer's visiting order.  With tmin = 1e-4f, tmax = 1e8f this is bit for
 *                        bit the hit the path tracer computes for the same ray under the same tree.
 *   GLRTX_TRACE_ANY      the first accepted hit in that visiting order (deterministic for a given tree): visibility and shadow tests.
 * A ray with a NaN or infinite component, a zero direction or tmax <= tmin is not searched: its answer is the miss record (t = tmax as given).  Denormal
 * components are read as zeros of their sign, as the device's arithmetic reads them -- tmax included: a denormal tmax is the limit 0 and comes back as 0 in
 * the miss record, and a direction whose components are all denormal is a zero direction.  A direction with a zero component is searched like any other:
 * 1 / 0 = +-inf in the slab test, and a slab product 0 * inf = NaN (the origin's coordinate equals a box bound on that axis) is dropped by min / max, which
 * return their other operand -- such a ray, lying in a face plane of a box, misses that box unless the box is flat on that axis.  Only the triangles are traced: spheres (GLRTX_EXT_*) and the volume
 * are not seen.  The result is what the CPU statement glrt_trace_rays (include/glrt_host.h) computes on the wire-format tree, bit for bit.
 *   glrtx_trace_rays         host arrays (n x 8 floats in, n x 4 words out); returns when the hits are in hits_out
 *   glrtx_trace_rays_device  device arrays on the context's device (16-byte aligned), read and written on the context's stream (glrtx_set_stream's, or the
 *                            context's own): the caller orders its producer there, or synchronises.  Returns once the query is enqueued; wait with glrtx_sync
 *                            or on that stream.
 * Both seal an open fed launch (glrtx_render), like glrtx_update_vertices, and leave the accumulator, frame numbering, adaptive state, presentation and the
 * ray counts of glrtx_stats untouched.  GLRTX_EINVAL, nothing changed: no scene uploaded, NULL buffers with n > 0, flags other than the two below,
 * n >= 2^31.  n = 0 succeeds and does nothing.  Groups: query a member, glrtx_group_ctx(grp, i) -- every member holds the whole scene. */
#define GLRTX_TRACE_CLOSEST 0
#define GLRTX_TRACE_ANY 1
int glrtx_trace_rays(glrtx_ctx *ctx, const float *rays, size_t n, float *hits_out, int flags);
int glrtx_trace_rays_device(glrtx_ctx *ctx, const void *dev_rays, size_t n, void *dev_hits, int flags);

/* Test hook: a copy of one device scene buffer as the kernels read it.  which: GLRTX_SCENE_NODES (the 64-byte node array, leaf records in reverse id
 * order then the forks), _CNODES (the compact records), _NRMS, _LIGHTS, _VINE (empty unless the tree is a vine), _ROOT (48 bytes: root box min {x, y, z, 0},
 * max {x, y, z, 0}, then the ints root_boxed, vine_uniform, root ref, vine records).  *bytes_out (may be NULL) gets the size; dst NULL asks for the size only.
 * Synchronises the context's stream. */
#define GLRTX_SCENE_NODES 0
#define GLRTX_SCENE_CNODES 1
#define GLRTX_SCENE_NRMS 2
#define GLRTX_SCENE_LIGHTS 3
#define GLRTX_SCENE_VINE 4
#define GLRTX_SCENE_ROOT 5
int glrtx_debug_read_scene(glrtx_ctx *ctx, int which, void *dst, size_t capacity_bytes, size_t *bytes_out);

/* Host-only (no device, no ctx): run the validation and repacking glrtx_upload_scene performs and
 * report the interior-node count and the traversal stack entries the BVH needs.  On failure the
 * message is available from glrtx_last_error(NULL). */
int glrtx_check_scene(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat,
                      const float *light, size_t n_light, const float *bvh, size_t n_nodes, int *n_fork_out,
                      int *stack_entries_out);

/* Host-only test hook (no device, no ctx): the repacked fork records as the kernels read them -- 16 floats per fork
 * {child L box min, ref L} {child L box max, ref R} {child R box min, -} {child R box max, -}, refs as int bit patterns
 * (>= 0 fork index; < 0 the record ~id of a LEAF of the tree, ids numbered from 1 in the order the traversal meets the leaves -- a hit carries this id,
 * not the wire triangle index; ref -1 = id 0 = the all-zero never-hit record that stands for an absent child).  A fork whose two children are both leaves
 * has no fork record: its triangle records are chained (children.y's names children.x's) and its parent refers to the first of them, so n_fork_out counts
 * only the forks that remain -- so that a test can replay
 * the traversal step's push/pop rules on the packed tree and check stack_entries against the deepest stack it reaches.
 * forks_out may be NULL (counts only).  No reference counterpart (the reference's stack is a fixed int[64], raytrace.frag:284). */
int glrtx_debug_pack_forks(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat,
                           const float *light, size_t n_light, const float *bvh, size_t n_nodes, float *forks_out,
                           size_t capacity_forks, int *n_fork_out, int *root_ref_out, int *stack_entries_out);

/* Host-only test hook (no device, no ctx): the compact node array the wavefront kernel walks when stats.node_layout_last is 1 -- 12 floats per position
 * (fork {child L box min, child R box max.x} {child L box max, child R box max.y} {child R box min, child R box max.z}; leaf {v0, id} {v1 - v0, next} {v2 - v0, 0},
 * id / next as int bit patterns: next is the position of the leaf chained behind this one, or INT32_MIN), the rank table (2 words per 32 positions: fork bits,
 * forks at smaller positions; the fork of rank k has its children at positions 2k + 1 and 2k + 2, the root is position 0), and the 64-byte leaf records by id
 * (16 floats each: {v0, material} {v1 - v0, next ref} {v2 - v0, -} {-}), so that a test can walk both layouts.  Any output may be NULL (counts only). */
int glrtx_debug_pack_compact(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat,
                             const float *light, size_t n_light, const float *bvh, size_t n_nodes, float *records_out, size_t capacity_positions,
                             int *n_positions_out, uint32_t *ranks_out, size_t capacity_words, float *leaves_out, size_t capacity_ids, int *n_ids_out);

/* Linear BVH built on the device (30-bit Morton order, Karras hierarchy, bottom-up fit), returned in the wire format
 * glrtx_upload_scene takes: nodes_out = (2*n_tri-1)*9 floats, root = node 0.  Takes the place of the reference's CPU
 * builder BVH::construct (src/core/bvh.cpp:59-160) for large scenes; identical, bit for bit, to glrt_bvh_build_lbvh
 * (glrt_host.h).  build_ms_out (may be NULL): device time of the build without the host<->device copies. */
int glrtx_build_lbvh(glrtx_ctx *ctx, const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out,
                     int *max_depth_out, float *build_ms_out);
/* Binned SAH built on the device, level by level from the top (16 bins, 3 axes), with the exact sweep SAH of the LBVH pass for the subtrees of <= 64 triangles
 * (csrc/sahl.hip.h; round 5).  Same contract and node layout as glrtx_build_lbvh; identical, bit for bit, to glrt_bvh_build_sah_levels (glrt_host.h).  The tree is as good
 * as the CPU binned-SAH builder's -- config 5 takes 80.5 instead of the LBVH's 84.4 traversal steps per ray (profiles/r05_tree_study.txt) -- for about twice the LBVH's
 * build time.  Replaces BVH::construct (src/core/bvh.cpp:59-160) like glrtx_build_lbvh does.
 * Neither device builder knows the materials: glrt_bvh_lights_first (glrt_host.h) on the returned nodes puts the child that holds the emitting triangles into the slot the
 * reference's traversal visits first -- worth 4 % per frame on the headline scene (profiles/r05_lights_first.txt); glrtx_upload_scene itself never reorders a tree. */
int glrtx_build_bvh_sah(glrtx_ctx *ctx, const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out,
                     int *max_depth_out, float *build_ms_out);

/* Full image size; (re)allocates and clears this ctx's accumulator rows. */
int glrtx_resize(glrtx_ctx *ctx, int width, int height);
int glrtx_clear(glrtx_ctx *ctx);

/* Row-stripe partition for multi-GPU: this ctx owns stripes s (of stripe_rows rows) with
 * s % world == rank; its accumulator holds only those rows, in increasing y, pixel coordinates
 * stay global.  stripe_rows: a multiple of 8 (whole 8x8 work tiles).  Default (rank 0, world 1) owns everything.
 * Must precede glrtx_resize. */
int glrtx_set_partition(glrtx_ctx *ctx, int rank, int world, int stripe_rows);
/* Global y of local accumulator row r (r in [0, owned_rows)), or -1. */
int glrtx_local_row_to_y(const glrtx_ctx *ctx, int local_row);

/* Optional: render into caller-owned device memory (e.g. a torch tensor that RCCL gathers)
 * instead of the ctx's own buffer: capacity_rows (>= owned_rows) rows of pitch_bytes, width float4 each.
 * While bound, glrtx_resize / glrtx_set_partition fail with GLRTX_EINVAL for a shape that does not fit
 * the buffer (the ctx cannot grow memory it does not own).  NULL unbinds. */
int glrtx_bind_accum(glrtx_ctx *ctx, void *device_ptr, size_t pitch_bytes, int capacity_rows);
/* Optional: launch on a caller-owned hipStream_t (passed as void*); NULL restores the ctx stream. */
int glrtx_set_stream(glrtx_ctx *ctx, void *hip_stream);

/* Kernel variant (tuning knob, no reference counterpart): 2 = workgroup-local wavefront (default: one
 * persistent launch; each workgroup runs traverse/shade trips over its own pixel blocks), 1 = persistent
 * megakernel with path regeneration, 0 = megakernel, one 16x16 tile per workgroup.  All three produce
 * bit-identical images.  The default can also be set with the environment variable GLRTX_VARIANT. */
int glrtx_set_variant(glrtx_ctx *ctx, int variant);

/* Shadow rays (sampleDirect, raytrace.frag:337-403).  Default (0): every light sample is resolved by the reference's own closest-hit search -- tHit
 * starts at INFTY, boxes are culled by the hits found, in the reference's visiting order -- and only ends early once an occluder in front of the
 * light is known (exact: tHit can only shrink).  1 opts in to the RANGE LIMIT of rounds 1-4: the search starts with tHit just beyond the light
 * sample's distance, which also culls boxes beyond the light (3-4 % fewer node visits per frame).  The limit gives the reference's verdict unless a
 * triangle test's computed t falls below the limit while the computed entry distance of one of its ancestors' boxes lies above it -- an
 * ill-conditioned (grazing) triangle test near the edge of a light lying flush in its box; no margin in terms of the distance bounds that error,
 * so the mode is NOT part of the bit-exact contract (csrc/pt_kernel.hip.h: shadow_limit).  Also: environment variable GLRTX_SHADOW_LIMIT=1 at
 * glrtx_create.  Takes effect with the next launch.  Group members: through glrtx_group_ctx. */
int glrtx_set_shadow_range_limit(glrtx_ctx *ctx, int enable);

/* Enable/disable per-launch ray counting (one atomic per wavefront); default off. */
int glrtx_count_rays(glrtx_ctx *ctx, int enable);

/* Asynchronous: accumulates n_samples new samples per owned pixel.  Returns as soon as the launch is enqueued (up to 16 launches may be
 * outstanding per context).  Consecutive calls overlap on the device: the render kernel of a call runs on one of six internal streams with
 * buffers of its own and hands its samples over in planes; only the pass that adds them to the accumulator runs on the context's stream
 * (glrtx_set_stream), in call order -- so everything a caller orders behind the call on that stream (resolve, read-back, a collective on the
 * rows) sees the finished accumulator, and per pixel the additions happen in the order of the calls.
 * FED LAUNCHES (ABI 10; the context's own stream only): a call that follows another render call directly -- same camera, samples and depth, nothing in between
 * that reads the accumulator or changes what a launch depends on -- does not become a launch of its own while that launch is still running: its frame is published to
 * the running kernel in host-coherent memory and rendered by it (glrtx_stats.feed_appended).  The pixels, and what every later call sees, are the same; only the launch
 * boundaries go away (one ramp and one drain per burst).  glrtx_sync, glrtx_resolve_rgba8, glrtx_read_accum, glrtx_clear, ... seal the open launch: nothing issued
 * after them is appended to a launch queued in front of them.  GLRTX_NO_FEED=1 turns this off.  See INTEGRATION.md. */
int glrtx_render(glrtx_ctx *ctx, const glrtx_params *params);
/* Frames in flight.  Same result, bit for bit, as n_frames consecutive glrtx_render calls whose params differ only
 * in `seed` (seeds_xy = n_frames pairs; params->seed is ignored) -- the reference's accumulation loop with a static
 * camera, window.cpp:226-252 -- but issued as ONE launch, so that a small image (or one rank's share of it) still fills
 * the GPU and the tail of one frame overlaps the next.  Every sample is kept in its own plane and the planes are added
 * to the accumulator in frame order.  stats.launches counts n_frames.  Asynchronous; seeds_xy is copied. */
int glrtx_render_frames(glrtx_ctx *ctx, const glrtx_params *params, const float *seeds_xy, int n_frames);
int glrtx_sync(glrtx_ctx *ctx);

/* Copy the owned rows (owned_rows x width float4) to host memory; implies a sync. */
int glrtx_read_accum(glrtx_ctx *ctx, float *dst_rgba, size_t dst_pitch_bytes);
/* Device address / pitch of the accumulator currently rendered into (a successful glrtx_reproject changes the address: ask again after it). */
int glrtx_accum_device_ptr(const glrtx_ctx *ctx, void **ptr_out, size_t *pitch_bytes_out);

/* Tonemap the owned rows to RGBA8: clamp(rgb/count, 0, 1)^(1/gamma), alpha 255.  If flip_y, row 0 of
 * dst is the top image row (as written by the reference's saveCurrentFrame).  Implies a sync. */
int glrtx_resolve_rgba8(glrtx_ctx *ctx, uint8_t *dst, size_t dst_pitch_bytes, float gamma, int flip_y);

/* Profile of a calibration frame (ABI 10): hist_out[t] = how often triangle t of the uploaded scene was the closest hit of a path ray -- camera rays and bounces -- in
 * ONE frame of `p`, rendered by the wavefront kernel into a scratch accumulator (the context's accumulator and statistics are left as they were; the call waits for the
 * device).  n_tri must be the uploaded scene's triangle count.  Input of glrt_bvh_order_by_hits (glrt_host.h): the child that is hit more often goes into the slot the
 * reference's traversal visits first (raytrace.frag:299-307; which child is which is the builder's choice, bvh.cpp:72-160). */
int glrtx_hit_histogram(glrtx_ctx *ctx, const glrtx_params *p, uint32_t *hist_out, size_t n_tri);

/* Measurement aid (bench.py's roofline_aux): device time of ONE launch of the resolve kernel -- screen.frag:15-25 over the owned rows -- from `reps` launches back to
 * back between one pair of events (a single launch between two events also measures the command processor's latency on both sides). */
int glrtx_debug_resolve_burst(glrtx_ctx *ctx, float gamma, int reps, float *ms_per_launch);

int glrtx_get_stats(const glrtx_ctx *ctx, glrtx_stats *out);
int glrtx_reset_stats(glrtx_ctx *ctx);

/* ---- Presentation: every frame's image, without a sync.  Replaces the second half of Window::render() -- the screen pass, screen.frag:15-25 -- and
 * saveCurrentFrame's read-back (src/core/window.cpp:157-164, :297-317, :383-414), which the reference runs after EVERY frame of its main loop.
 * glrtx_present_enable gives the context a ring of ring_images RGBA8 images in pinned host memory (and a device mirror of them).  From then on every
 * frame rendered -- each glrtx_render call, each frame of glrtx_render_frames -- also produces its image: the pass that adds the frame's samples to the
 * accumulator resolves it in the same read (launches whose render kernel accumulates by itself -- a plain single frame, a caller's stream, variants 0 / 1,
 * the extension kernel -- are followed by the resolve kernel instead), and a copy stream of the context's own lands it in its pinned image behind that
 * pass.  Image `frame` k is the image after the k-th frame since the last glrtx_clear / glrtx_resize: byte for byte what glrtx_resolve_rgba8(ctx, ..., gamma,
 * flip_y) returns at that point (the owned rows, pitch width * 4).
 * Presentation does NOT seal a fed launch (glrtx_render): a burst of render calls stays one launch, and its images are handed over when that launch's
 * pass has run, i.e. when the launch ends -- not frame by frame inside it (the trade: full throughput against up to a launch of latency).
 * Every frame takes a ring image when it is issued: with none free, glrtx_render / glrtx_render_frames return GLRTX_EBUSY before they change anything (no
 * launch, no stats, no frame number), and the same call after a glrtx_present_release does what it would have done.  A call with more frames than the
 * ring holds fails with GLRTX_EINVAL.  glrtx_hit_histogram produces no images; glrtx_resize fails with GLRTX_EINVAL while an image is acquired; images
 * ready and not yet acquired keep their own size and frame number across glrtx_clear / glrtx_resize.
 *   glrtx_present_enable   ring_images >= 1: (re)start presentation (gamma > 0, flip_y as in glrtx_resolve_rgba8); 0: stop -- waits for the copies in
 *                          flight and drops the images not acquired.  Fails with GLRTX_EINVAL while an image is acquired.
 *   glrtx_present_acquire  the oldest image not yet acquired, in frame order; wait = 0: GLRTX_EBUSY unless it is ready; wait = 1: blocks until it is
 *                          (GLRTX_EBUSY if no frame is outstanding at all).  out->rgba stays valid, and is not rewritten, until released.
 *   glrtx_present_release  hands an acquired image's memory back to the ring. */
typedef struct glrtx_image {
    const uint8_t *rgba;   /* rows x width RGBA8 texels, pinned host memory owned by the context (group: by the group) */
    size_t pitch_bytes;
    int32_t width, rows;   /* a context: its owned rows; a group: the full image */
    uint64_t frame;        /* frames accumulated since the last glrtx_clear / glrtx_resize, this one included (from 1) */
} glrtx_image;
typedef struct glrtx_present_stats {
    uint64_t images;       /* images produced (one per frame rendered while presentation is on); the counters run over the context's life */
    uint64_t delivered;    /* ... of them acquired */
    uint64_t dropped;      /* ... of them never acquired: dropped by glrtx_present_enable(ctx, 0, ...) or a re-enable */
    uint64_t busy_returns; /* GLRTX_EBUSY returns: render calls that found no free ring image, and acquires with nothing ready */
    int32_t ring_images;   /* 0: presentation off */
    int32_t pending;       /* images produced and not yet acquired (ready or in flight) */
    int32_t held;          /* images acquired and not yet released */
    int32_t copies_last;   /* host copies of the last image (a context: 1; a group: per member one strided copy, plus one for a partial last stripe) */
    float pass_ms_last;    /* device time of the last presenting pass (fused accumulate + resolve, or the resolve kernel), once it has completed */
    int32_t reserved;
} glrtx_present_stats;
int glrtx_present_enable(glrtx_ctx *ctx, int ring_images, float gamma, int flip_y);
int glrtx_present_acquire(glrtx_ctx *ctx, int wait, glrtx_image *out);
int glrtx_present_release(glrtx_ctx *ctx, const glrtx_image *img);
int glrtx_present_get_stats(const glrtx_ctx *ctx, glrtx_present_stats *out);

/* HIP-event stopwatch on the stream launches go to: begin, N x render, end -> elapsed device ms. */
int glrtx_timer_begin(glrtx_ctx *ctx);
int glrtx_timer_end(glrtx_ctx *ctx, float *elapsed_ms_out);

/* ---- Extensions beyond the reference.  PARITY UNPINNED: the reference has no analytic primitive
 * (scenes are triangle meshes, raytrace.frag:226-257) and never branches on MTRL_DIELECTRIC (raytrace.frag:32), so there is no
 * reference output for any of this; it is checked against this build's own CPU restatement (oracle/pt_oracle.c, *_ext) and
 * against the tessellation limit of the pinned triangle path.  Off unless asked for; while active, launches run on the
 * persistent megakernel (no frames in flight) and everything the reference does define keeps its pinned arithmetic.
 *   glrtx_upload_spheres   n x {cx, cy, cz, radius, materialId}: analytic spheres next to the triangle BVH, tested one by
 *                          one (at most 1024); call after glrtx_upload_scene (which drops them); n = 0 removes them.
 *   glrtx_set_extensions   GLRTX_EXT_DIELECTRIC: materials of type 4 (MTRL_DIELECTRIC; param0 = tint, param1.x = index of
 *                          refraction) reflect / refract with the Fresnel reflectance as probability instead of being black.
 *                          GLRTX_EXT_WHITTED: Whitted-style transport -- a diffuse surface gathers its direct light and the
 *                          path ends; only specular bounces continue. */
#define GLRTX_EXT_DIELECTRIC 1
#define GLRTX_EXT_WHITTED 2
int glrtx_upload_spheres(glrtx_ctx *ctx, const float *spheres, size_t n_spheres);
int glrtx_set_extensions(glrtx_ctx *ctx, int flags);

/* ---- Participating media: the reference's volume branch (raytrace.frag:424-487, blackBody :125-142, lookups :144-152), which the
 * reference compiles out (ENABLE_VOLUME 0, raytrace.frag:4).  Off by default; GLRTX_EXT_VOLUME (glrtx_set_extensions) switches it on,
 * like the reference's define, and routes rendering to the persistent megakernel as the other extension flags do (or, with
 * glrtx_set_volume_wavefront, to the wavefront kernel).  PINNED: the images
 * are the reference shader's with the switch on and ONE edit -- densityLookup / temperatureLookup read textureLod(tex, uvw, 0.0), the
 * trilinear magnification filter with GL_REPEAT, instead of texture(tex, uvw), whose filter GL leaves to the 2x2 pixel quad (DESIGN.md
 * section 3, "Volumes").  Like the reference (window.cpp:271-286) only one volume exists: it applies to every media material.
 *   glrtx_upload_volume   two nx x ny x nz grids, x fastest (the order glTexSubImage3D reads; a grid file with several channels contributes
 *                         its first nx*ny*nz floats), copied to device memory; bbox_min / bbox_max = u_bboxMin / u_bboxMax (the scene's JSON,
 *                         not the grid file's header); density_max = u_densityMax (the largest value of the density file over all its
 *                         channels).  density == NULL or an empty grid (a zero dimension) removes the volume.  Kept across glrtx_upload_scene.
 *                         GLRTX_EINVAL: NULL ctx, a negative dimension, more than 2^29 texels, a NULL temperature grid or bbox, a bbox with zero
 *                         or non-finite extent on some axis.
 *   Rendering with GLRTX_EXT_VOLUME set and no volume uploaded fails with GLRTX_EINVAL.  Every trial ray of the Woodcock tracking counts as a
 *   ray (glrtx_count_rays).  Group members: glrtx_group_upload_volume, and the flag through glrtx_group_ctx. */
#define GLRTX_EXT_VOLUME 4
/*   glrtx_set_volume_wavefront   1: volume launches run on the wavefront kernel (variant 2) instead of the persistent megakernel -- frames in flight, fed
 *                         launches, the present ring and glrtx_render_adaptive then work with the volume on, and variant_last reports 2.  Taken when
 *                         the volume is the only extension (no GLRTX_EXT_DIELECTRIC / WHITTED, no spheres), variant 2 is selected, u_maxDepth <= 255 and
 *                         u_nSamples < 2^16 (beyond that: the megakernel, GLRTX_FALLBACK_SAMPLES); anything else runs as with the switch off.  The
 *                         images and ray counts are the megakernel's, bit for bit.  Default 0; GLRTX_VOLUME_WAVEFRONT=0/1 in the environment
 *                         overrides it at every launch.  Group members: through glrtx_group_ctx. */
int glrtx_set_volume_wavefront(glrtx_ctx *ctx, int enable);
int glrtx_upload_volume(glrtx_ctx *ctx, const float *density, const float *temperature, int nx, int ny, int nz, const float bbox_min[3],
                        const float bbox_max[3], float density_max);
/* Debug export (no ctx; the current HIP device): the device's statements of llvmpipe's log / exp / acos, and of blackBody, evaluated on n host
 * values.  op GLRTX_VMATH_LOG / _EXP / _ACOS: out[i] = f(in[i]); GLRTX_VMATH_BLACKBODY: out[3i..3i+2] = blackBody(100 * in[i]) (in = the
 * temperature grid's value, as temperatureLookup() returns it).  glrtx_debug_volume_lookup: out[i] = the density lookup of the grid at
 * pos[3i..3i+2].  Synchronous; errors are reported through glrtx_last_error(NULL). */
#define GLRTX_VMATH_LOG 0
#define GLRTX_VMATH_EXP 1
#define GLRTX_VMATH_ACOS 2
#define GLRTX_VMATH_BLACKBODY 3
int glrtx_debug_volume_math(int op, const float *in, size_t n, float *out);
int glrtx_debug_volume_lookup(const float *grid, int nx, int ny, int nz, const float bbox_min[3], const float bbox_max[3], const float *pos,
                              size_t n, float *out);

/* ---- Adaptive sampling: spend frames only on the 8x8 tiles that have not converged (no reference counterpart; off unless called).
 * A pixel's sample depends only on the pixel and the frame's seed (raytrace.frag:566, rand() :104-111), so rendering some pixels of a frame leaves each of them
 * bit-identical to the full frame, and the accumulator's per-pixel count already lets pixels resolve with different sample counts (screen.frag:15-25).
 *   glrtx_render_adaptive  at the start of the call, on the device, decides which tiles of the context's owned rows are ACTIVE; then renders n_frames frames
 *                          with the given seeds, only the pixels of active tiles, and adds their samples to the accumulator in frame and sample order -- the
 *                          chain of fp32 additions consecutive glrtx_render calls would form for those pixels.  Inactive tiles are not touched.  Tiles are the
 *                          wavefront kernel's: ceil(width / 8) x ceil(owned_rows / 8) in owned-row space, row-major, partial at the right and bottom edges.
 *                          The context gets a half buffer H (accumulator-sized, allocated on first use, zeroed by glrtx_clear / glrtx_resize): a sample is
 *                          added to H as well whenever the pixel's count BEFORE the add is odd (H holds every second sample).  The selection is stateless:
 *                          every call re-evaluates every tile from the accumulator and H as they stand when the call begins.  A tile is active if one of its
 *                          in-image pixels has count < min_samples or H.w == 0, or if its error E > threshold, or E is NaN, or threshold < 0 (nothing retires:
 *                          the call equals glrtx_render_frames bit for bit, plus H).  E is the mean over the tile's in-image pixels of
 *                              d = (|I.r - A.r| + |I.g - A.g| + |I.b - A.b|) / sqrt(I.r + I.g + I.b + 1e-3),  I = acc.rgb / acc.w,  A = H.rgb / H.w
 *                          (Dammertz et al.; fp32, order and summation in DESIGN.md).  Never a fed launch: an open one is sealed first.  n_frames = 0 selects only.
 *                          Issued without a sync.  GLRTX_EINVAL, nothing changed: min_samples < 2, presentation enabled, extensions or volume on, spheres
 *                          uploaded, variant != 2, or max_depth / n_samples beyond the wavefront kernel's path state (the megakernels have no tile list).
 *   glrtx_adaptive_active_tiles  syncs, then reports the last selection: active and total tiles.
 *   glrtx_read_tile_mask         syncs, then copies the last selection's mask, one byte (0 / 1) per tile, total bytes; GLRTX_EINVAL if the image has
 *                                changed shape (resize, partition) since that selection.  glrtx_bind_accum zeroes H, like glrtx_clear.
 *   glrtx_read_adaptive_half     syncs, then copies H (float4(rgb, count) per pixel, owned rows), like glrtx_read_accum.
 *   glrtx_debug_adaptive_select  the selection kernels on caller arrays (width x rows float4, rows packed): the mask, E per tile (NULL: not wanted; a NaN
 *                                is returned as 0x7FC00000), the ascending list of active tiles and its length (NULL: not wanted). */
typedef struct glrtx_adaptive {
    float threshold;  /* a tile retires once E <= threshold; < 0: nothing retires */
    int min_samples;  /* every pixel of a tile needs this many samples before it may retire (>= 2) */
} glrtx_adaptive;
int glrtx_render_adaptive(glrtx_ctx *ctx, const glrtx_params *params, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg);
int glrtx_adaptive_active_tiles(glrtx_ctx *ctx, int *active, int *total);
int glrtx_read_tile_mask(glrtx_ctx *ctx, uint8_t *dst);
int glrtx_read_adaptive_half(glrtx_ctx *ctx, float *dst_rgba, size_t dst_pitch_bytes);
int glrtx_debug_adaptive_select(const float *accum, const float *half, int width, int rows, float threshold, int min_samples, uint8_t *mask_out,
                                float *err_out, int *list_out, int *count_out);

/* ---- Denoising: feature planes and an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) for low-sample frames (no reference counterpart; off
 * unless called: no other call changes what it does, and nothing here ever writes the accumulator, the adaptive half buffer, the present ring or glrtx_stats.rays).
 *   glrtx_render_features  fills two context-owned float4 planes over the owned rows (allocated on first use, released by glrtx_resize and so by a partition
 *                          change), on the context's stream behind whatever was issued, sealing an open fed launch first:
 *                              plane N {nx, ny, nz, t}   shading normal (the renderer's, a NaN component stored as 0x7FC00000) and distance of the closest hit;
 *                                                        {0, 0, 0, 0} on a miss;
 *                              plane A {r, g, b, id}     param0 of a diffuse material (type 2), {1, 1, 1} for every other type and on a miss; id: the material
 *                                                        index as int32 bits, -1 on a miss.
 *                          The ray of pixel (x, y) is the renderer's primary ray with both pixel random numbers 0.5 and no thin lens, whatever params->aperture
 *                          is (only c2w and s2c are read); the search is a primary ray's (t in (1e-4, 1e8)), by the renderer's own traversal, in either node
 *                          layout and on vines.  GLRTX_EINVAL: no scene, no size, spheres uploaded (no triangle normal to report).
 *   glrtx_read_features    syncs, then copies the planes (owned rows, `pitch_bytes` per row in both destinations).
 *   glrtx_denoise          filters I = acc.rgb / acc.w, guided by the feature planes AS THEY STAND (render them again after a camera move or a vertex update),
 *                          into a context-owned float4 image D {rgb, 1}.  Issued on the context's stream without a sync; an open fed launch is sealed first.
 *                          A pixel is DEAD when acc.w is a zero or a denormal, or when its id is INT32_MIN (reserved); dead pixels come out {0, 0, 0} and weigh 0
 *                          as taps.  With demodulate, a = max(albedo, 1e-3) per channel (a > 1e-3 ? a : 1e-3) and c = I / a, else c = I.  Iteration i = 0 ..
 *                          iterations - 1, for every live centre p and the 25 taps q = p + 2^i (dx, dy), dx, dy in -2..2, dy outermost (row-major):
 *                              w(q) = (k[dy+2] k[dx+2]) * lp_exp(-((dc / sc_i + dn / sigma_normal) + min(dd, 80)))          k = {1, 4, 6, 4, 1} / 16
 *                              dc = (dr dr + dg dg) + db db  over c_q - c_p;   dn likewise over n_q - n_p;   sc_i = sigma_color * 4^-i (a denormal: 0)
 *                              dd = (r r) / sigma_depth,  r = (t_q - t_p) / max(t_p, 1e-6);   min(dd, 80) = dd < 80 ? dd : 80
 *                              c'_p = (sum w(q) c_q) / max(sum w(q), 1e-20)
 *                          over the taps that lie inside the image, are alive and carry p's id (the others are skipped, not added as zeros); both sums start at
 *                          0 and grow in tap order; max(s, 1e-20) = s > 1e-20 ? s : 1e-20.  After the last iteration c is multiplied by a again (demodulate).
 *                          lp_exp is the renderer's exponential (csrc/pt_kernel.hip.h).  Every fp32 operation is one correctly rounded operation, unfused,
 *                          denormals flushed; every value stored is 0x7FC00000 when it is a NaN.  glrt_denoise_atrous (glrt_host.h) and
 *                          tests/denoise_math.py state the same arithmetic; the three agree bit for bit.  "Inside the image" means inside the context's
 *                          owned rows, taken as one image in local row order: a partitioned context filters its own rows only, and groups have no denoise call
 *                          (out of scope).  GLRTX_EINVAL: iterations outside 1..6, a sigma that is not a positive finite number, no accumulator, no feature
 *                          planes, or planes of another shape than the image now has.
 *   glrtx_read_denoised    syncs, then copies D like glrtx_read_accum.
 *   glrtx_resolve_denoised_rgba8  D through glrtx_resolve_rgba8's kernel (D's count word is 1, so its division changes nothing): the 8-bit image of D.
 *   glrtx_debug_denoise    the filter on caller arrays (width x rows float4 each, rows packed) on the current HIP device, no context. */
typedef struct glrtx_denoise_cfg {
    int   iterations;    /* 1..6; iteration i uses tap spacing 2^i */
    float sigma_color;   /* iteration i uses sigma_color * 4^-i */
    float sigma_normal;
    float sigma_depth;
    int   demodulate;    /* 1: filter I / max(albedo, 1e-3), multiply back at the end */
} glrtx_denoise_cfg;
int glrtx_render_features(glrtx_ctx *ctx, const glrtx_params *params);
int glrtx_read_features(glrtx_ctx *ctx, float *normal_depth, float *albedo_id, size_t pitch_bytes);
int glrtx_denoise(glrtx_ctx *ctx, const glrtx_denoise_cfg *cfg);
int glrtx_read_denoised(glrtx_ctx *ctx, float *dst_rgba, size_t dst_pitch_bytes);
int glrtx_resolve_denoised_rgba8(glrtx_ctx *ctx, uint8_t *dst, size_t dst_pitch_bytes, float gamma, int flip_y);
int glrtx_debug_denoise(const float *accum, const float *normal_depth, const float *albedo_id, int width, int rows, const glrtx_denoise_cfg *cfg, float *out);

/* ---- Variance guidance: per-pixel luminance moments and SVGF's variance-guided a-trous filter (Schied et al. 2017; no reference counterpart; everything here is
 * off unless glrtx_track_moments switched it on, and while it is off no other call changes what it does or writes).  glrtx_denoise stops at colour edges with one
 * fixed sigma_color for a pixel with 1 sample and for one with 64; here the luminance edge term is scaled by the standard deviation of each pixel's own mean, so a
 * noisy pixel takes from its neighbours and a converged one is left alone.
 *   lum(r, g, b) = (0.2126 r + 0.7152 g) + 0.0722 b.  The rules are those of "Denoising": every fp32 operation is one correctly rounded operation in the order
 *   written, unfused (lp_exp carries the only fused ones), denormals flushed in and out; min / max are selects (max(x, 0) = x > 0 ? x : 0, so a NaN gives 0);
 *   sqrt is the correctly rounded one; a NaN that is stored is 0x7FC00000.  host/variance.cpp (glrt_host.h) and tests/variance_math.py state the same arithmetic;
 *   the three agree bit for bit.
 *   glrtx_track_moments(enable)  off by default.  While on, the context owns a float4 plane M of the accumulator's pitch, {sum l, sum l^2, 0, count}, l = lum of one
 *                          sample plane's rgb.  M is allocated (zeroed) on first use -- the first glrtx_render_moments or glrtx_read_moments --, zeroed by glrtx_clear
 *                          and glrtx_bind_accum, released by glrtx_resize (and so by a partition change).  Switching tracking off syncs and releases M.
 *                          glrtx_reproject and glrtx_reproject_motion zero the adaptive half buffer H; M they CARRY ("Carrying M" below): H's every-second-sample
 *                          rule is a property of the old pixel grid and loses its meaning under resampling, whereas a surface point's luminance moments come
 *                          along with its mean -- and the pixels with carried history are exactly the ones the filter should tighten on.
 *   glrtx_render_moments   renders like glrtx_render_frames: the accumulator comes out bit for bit what glrtx_render_frames gives (the same chain of additions, in
 *                          frame and sample order), and the same pass adds every sample to M: M.x += l; M.y += l * l; M.w += 1.  The launch shape is
 *                          glrtx_render_adaptive's without a selection: never a fed launch (an open one is sealed first), plain launches with sample planes on the
 *                          context's stream, in helpings of what the frames-in-flight budget allows.  n_frames = 0 only allocates M.  The adaptive half buffer is not
 *                          touched.  GLRTX_EINVAL, nothing changed: tracking off, presentation enabled, extensions or volume on, spheres uploaded, variant != 2,
 *                          max_depth / n_samples beyond the wavefront kernel's path state, and what glrtx_render_frames refuses.  Other rendering calls stay legal
 *                          while tracking is on: they add samples M does not see.  M's own count says how many samples M holds; everything below uses M's count,
 *                          never the accumulator's.
 *   glrtx_read_moments     syncs, then copies M like glrtx_read_accum.  GLRTX_EINVAL while tracking is off.
 *   glrtx_denoise_variance the variance pass, then the filter, into the same image D as glrtx_denoise (glrtx_read_denoised and glrtx_resolve_denoised_rgba8 serve
 *                          it unchanged).  Issued on the context's stream without a sync.  GLRTX_EINVAL: what glrtx_denoise refuses (sigma_lum in sigma_color's
 *                          place), tracking off, or before M exists (no first use since tracking was switched on or since a glrtx_resize).  Nothing here
 *                          writes the accumulator, M, the adaptive half buffer, the present ring or glrtx_stats.rays.
 *   glrtx_debug_denoise_variance  both passes on caller arrays (width x rows float4 each, rows packed) on the current HIP device, no context; v0_out (width x rows
 *                          floats, may be NULL) receives V0.
 * The variance pass: V0, a float per pixel -- the variance of the pixel's MEAN luminance, in the filter's colour space.  "Dead" is "Denoising"'s (acc.w a zero or a
 * denormal, or id INT32_MIN); a dead pixel gets V0 = 0.  Per pixel: if M.w is neither a zero nor a denormal, mu1 = M.x / M.w and mu2 = M.y / M.w; otherwise
 * mu1 = lum(acc.r / acc.w, acc.g / acc.w, acc.b / acc.w) and mu2 = mu1 * mu1.
 *     temporal, where M.w >= 4 (a NaN fails):   v = max(mu2 - mu1 * mu1, 0) / M.w
 *     spatial, elsewhere (every 1-spp frame):   over the 49 taps q = p + (dx, dy), dx, dy in -3..3, dy outermost, that lie inside the image, are alive and carry p's id
 *                                               (the centre is one of them), from 0 in tap order:
 *                                                   w = lp_exp(-(dn / sigma_normal + min(dd, 80)))        dn, dd exactly glrtx_denoise's
 *                                                   sw = sw + w;  s1 = s1 + w * mu1_q;  s2 = s2 + w * mu2_q
 *                                               S1 = s1 / max(sw, 1e-20), S2 = s2 / max(sw, 1e-20), v = max(S2 - S1 * S1, 0): the spread of neighbouring means already is a
 *                                               variance of means, so there is no division by a count.
 *     with demodulate: v = v / (la * la), la = lum(a), a = max(albedo, 1e-3) per channel as in "Denoising".      V0 = v (a NaN: 0x7FC00000).
 * The filter: c and the dead pixels as glrtx_denoise prepares them, V = V0.  Iteration i = 0 .. iterations - 1 is glrtx_denoise's with two changes.
 *     (1) g_p = (sum kw V_q) / (sum kw) over the 3x3 taps q = p + (dx, dy), dx, dy in -1..1, dy outermost, at unit spacing whatever i is, that lie inside the image, are
 *         alive and carry p's id; kw = k3[dy+1] * k3[dx+1], k3 = {1, 2, 1} / 4; both sums from 0 in tap order.  sl_p = sigma_lum * sqrt(g_p) + 1e-6.  The tap weight is
 *             w(q) = (k[dy+2] k[dx+2]) * lp_exp(-((|lum(c_q) - lum(c_p)| / sl_p + dn / sigma_normal) + min(dd, 80)))
 *         sigma_lum does not shrink with i: the variance does that job.
 *     (2) the variance is filtered alongside, over the same taps:  V'_p = (sum (w(q) * w(q)) * V_q) / (d * d),  d = max(sum w(q), 1e-20); a NaN is stored as 0x7FC00000,
 *         a dead pixel gets 0.
 *     After the last iteration c is multiplied by a again (demodulate), as there.
 * Carrying M.  While tracking is on and M exists, glrtx_reproject and glrtx_reproject_motion also write a second M, allocated (before anything changes) and swapped
 * as the second accumulator is, by the same kernel pass and the same taps ("Reprojection" steps 5-7; one function shared by both kernels: reproject.hip.h
 * moments_tap / moments_out).  A tap counts for M if it counts in step 5 and its M.w is neither a zero nor a denormal.  Over those taps, from 0, in tap order:
 *     sm = sm + w;   smc = smc + w * M.w;   s1 = s1 + w * (M.x / M.w);   s2 = s2 + w * (M.y / M.w)
 * "No moments" means {0, 0, 0, 0}; it applies unless sm > 1e-6.  nm = rint(smc / sm), capped at max_history (nm > max_history ? max_history : nm); no moments
 * unless nm >= 1 (a NaN fails); otherwise the new M is {(s1 / sm) * nm, (s2 / sm) * nm, 0, nm} (a NaN stored as 0x7FC00000).  A pixel with no accumulator history
 * has no moments either.  The accumulator output of both calls and their carried / hit_pixels counts are bit for bit what they are with tracking off.
 * glrtx_debug_reproject_moments / glrtx_debug_reproject_motion_moments are glrtx_debug_reproject / _motion with the old view's M in and the new view's M out
 * (width x rows float4, rows packed); glrt_reproject_moments / glrt_reproject_motion_moments (glrt_host.h) and tests/variance_math.py state them again.
 * Out of scope: groups (a partitioned context filters its own rows, as glrtx_denoise does); feeding M from fed
 * launches, the present ring, the megakernels or the volume forms; separate direct and indirect buffers.  (The adaptive selection made from M: "Adaptive
 * sampling by variance" below.) */
typedef struct glrtx_denoise_var_cfg {
    int   iterations;    /* 1..6; iteration i uses tap spacing 2^i */
    float sigma_lum;     /* the luminance edge stops at sigma_lum standard deviations of the pixel's mean */
    float sigma_normal;
    float sigma_depth;
    int   demodulate;    /* 1: filter I / max(albedo, 1e-3), multiply back at the end */
} glrtx_denoise_var_cfg;
int glrtx_track_moments(glrtx_ctx *ctx, int enable);
int glrtx_render_moments(glrtx_ctx *ctx, const glrtx_params *params, const float *seeds_xy, int n_frames);
int glrtx_read_moments(glrtx_ctx *ctx, float *dst_rgba, size_t dst_pitch_bytes);
int glrtx_denoise_variance(glrtx_ctx *ctx, const glrtx_denoise_var_cfg *cfg);
int glrtx_debug_denoise_variance(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows,
                                 const glrtx_denoise_var_cfg *cfg, float *out, float *v0_out);
struct glrtx_reproject_cfg;
int glrtx_debug_reproject_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev,
                                  const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows, const struct glrtx_reproject_cfg *cfg,
                                  float *out, float *moments_out, int *carried, int *hit_pixels);
int glrtx_debug_reproject_motion_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *g1, const float *a1,
                                         const float *vert_prev, size_t n_vert, const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev,
                                         int width, int rows, const struct glrtx_reproject_cfg *cfg, float *out, float *moments_out, int *carried, int *hit_pixels);

/* ---- Adaptive sampling by variance: glrtx_render_adaptive with the selection made from the moments plane M (no reference counterpart; off unless called: no
 * other call changes what it does or writes).  glrtx_render_adaptive estimates a tile's error from the half buffer H, and both reprojections zero H ("H.w = 0 makes
 * every tile active again"): after every camera or geometry move it renders the whole frame again.  M is carried by both reprojections ("Carrying M"), and it is
 * the direct estimate of what the two-buffer trick approximates: the variance of each pixel's mean.  With the selection made from M a call after a move spends its
 * frames on the disoccluded tiles -- no moments, therefore active -- and on the tiles that are still noisy, and the samples it adds feed the variance that
 * glrtx_denoise_variance reads afterwards.
 *   glrtx_render_adaptive_moments  is glrtx_render_adaptive step for step -- the selection at the start of the call, on the device; then n_frames frames of the
 *                          active tiles only, by the same kernel over the same tile list, plain launches with sample planes on the context's stream in helpings of
 *                          what the frames-in-flight budget allows, never fed, an open fed launch sealed first; issued without a sync -- with three differences.
 *                          (1) The selection reads M only, as M stands when the call begins (M gets its zeroed first-use allocation if needed, as in
 *                          glrtx_render_moments).  It neither reads nor allocates H.  It writes the context's one mask, list and count: glrtx_adaptive_active_tiles
 *                          and glrtx_read_tile_mask report this selection as they report glrtx_render_adaptive's, whichever came last.
 *                          (2) The accumulation pass adds each sample of an active tile's pixel to the accumulator and folds it into M exactly as
 *                          glrtx_render_moments does: M.x += l; M.y += l * l; M.w += 1, then acc.rgb += v.rgb; acc.w += 1, in frame and sample order.  Inactive
 *                          tiles are not touched in either buffer.
 *                          (3) H is not touched at all: not created, not read, not written.
 *                          The rules are those of "Variance guidance" (one correctly rounded fp32 operation at a time in the order written, unfused, denormals
 *                          flushed in and out, the correctly rounded sqrt, selects as written).  Per in-image pixel of an 8x8 tile:
 *                              force = !(M.w >= (float)min_samples)                    (a zero, a denormal, a negative or a NaN count forces)
 *                              mu1 = M.x / M.w;   mu2 = M.y / M.w
 *                              v = mu2 - mu1 * mu1;   v = v > 0 ? v : 0;   v = v / M.w   (glrtx_denoise_variance's temporal branch, without demodulation)
 *                              d = sqrt(v) / sqrt(mu1 + 1e-3)
 *                          d is 0 outside the image.  E is the tile's mean of d: lane k of the tile's wave holds pixel (k & 7, k >> 3), the 64 values are summed
 *                          as a tree -- s[k] = s[k] + s[k ^ h] for h = 32, 16, 8, 4, 2, 1 -- and s[0] is divided by the number of in-image pixels.  A tile is active
 *                          if one of its in-image pixels forces, if threshold < 0 (nothing retires: the accumulator and M come out bit for bit
 *                          glrtx_render_moments's), or if !(E <= threshold) (a NaN E keeps the tile active).
 *                          THRESHOLDS OF THE TWO FORMS ARE NOT INTERCHANGEABLE.  Here d is a standard error of the mean luminance over the root of that luminance;
 *                          in glrtx_render_adaptive it is a sum of three channel differences between two half-images over sqrt(r + g + b).  The same number means
 *                          different image quality in the two calls.
 *                          n_frames = 0 selects only.  min_samples >= 2 as there: one sample has no variance.  GLRTX_EINVAL, nothing changed: everything
 *                          glrtx_render_adaptive refuses and everything glrtx_render_moments refuses -- NULL params or cfg, min_samples < 2, bad seeds / n_frames,
 *                          tracking off, no scene, no accumulator, presentation enabled, extensions or volume on (the V form too: M is not fed by the volume
 *                          forms), spheres uploaded, variant != 2, max_depth / n_samples beyond the wavefront kernel's path state.  A partitioned context selects
 *                          and renders on its owned rows, as in glrtx_render_moments; there is no group call (groups are out of scope for M).
 *   glrtx_debug_adaptive_select_moments  the selection kernels on a caller array (width x rows float4, rows packed) on the current HIP device, no context: the mask, E
 *                          per tile (NULL: not wanted; a NaN is returned as 0x7FC00000), the ascending list of active tiles and its length (NULL: not wanted).
 * glrt_adaptive_select_moments (glrt_host.h) and tests/adaptive_moments_math.py state the selection again; the three agree bit for bit.
 * Out of scope: group calls and the present ring; a per-tile sample budget beyond the on/off decision; selecting by glrtx_denoise_variance's filtered variance; the
 * volume forms; feeding M from fed launches. */
int glrtx_render_adaptive_moments(glrtx_ctx *ctx, const glrtx_params *params, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg);
int glrtx_debug_adaptive_select_moments(const float *moments, int width, int rows, float threshold, int min_samples, uint8_t *mask_out, float *err_out, int *list_out,
                                        int *count_out);

/* ---- Reprojection: carry the accumulator across a camera move (the reprojection step of SVGF, Schied et al. 2017; no reference counterpart -- the reference
 * clears and starts again at one sample, window.cpp:366-381; off unless called).  The context remembers the c2w and s2c of its last glrtx_render_features: the
 * PREVIOUS camera, the one the accumulator and the feature planes belong to.
 *   glrtx_reproject(cur)   on the context's stream, without a host sync (but the first call allocates).  In order: (1) seals an open fed launch and waits, on the
 *                          device, for every pipe slot's outstanding launch, as glrtx_update_vertices does; (2) keeps the feature planes as the previous planes
 *                          N0 / A0 by a pointer swap (a second pair is allocated on first use and released by glrtx_resize); (3) renders the planes N1 / A1 for
 *                          `cur` exactly as glrtx_render_features(cur) does; (4) runs the reprojection kernel from the accumulator into a second, context-owned
 *                          accumulator of the same pitch (allocated on first use, released by glrtx_resize); (5) makes that second accumulator the one rendered
 *                          into: WHAT glrtx_accum_device_ptr RETURNS CHANGES with every successful call (the two buffers alternate) -- ask again after each one.
 *                          The remembered camera becomes `cur`, and the planes are cur's: a following glrtx_denoise needs no glrtx_render_features.  If the adaptive
 *                          half buffer exists it is zeroed (its every-second-sample rule has lost its meaning; H.w = 0 makes every tile active again);
 *                          the moments plane M of glrtx_track_moments is carried, not zeroed ("Variance guidance").  The present
 *                          ring, glrtx_stats.rays and the denoised image are not touched; the call is not a frame.
 *                          GLRTX_EINVAL, nothing changed: NULL arguments; no feature planes, or planes of another shape than the image now has; a partitioned
 *                          context (world > 1: the source pixel may belong to another rank; groups are out of scope, as for glrtx_denoise); a caller-bound
 *                          accumulator (glrtx_bind_accum); everything glrtx_render_features refuses; max_history < 1; a depth_tolerance that is not a positive
 *                          finite number; a normal_tolerance that is not finite; a previous camera whose c2w or s2c glrt_mat4_inverse (glrt_host.h) reports singular.
 *   glrtx_reproject_last   syncs, then reports the last call's counts: pixels that carried history over, and pixels of the new view with a hit (A1.id >= 0).
 *                          GLRTX_EINVAL before the first glrtx_reproject and after a glrtx_resize.
 *   glrtx_debug_reproject  the kernel on caller arrays (width x rows float4 each, rows packed; accum / N0 / A0: the old view, N1 / A1: the new view's planes) on the
 *                          current HIP device, no context.  carried / hit_pixels may be NULL.  The refusals of the cfg and of singular matrices as above; sizes
 *                          outside 1..65536 or more than 2^31 pixels.
 * The arithmetic (this text is the contract; glrt_reproject in glrt_host.h and tests/reproject_math.py state it again, and the three agree bit for bit).  Every fp32
 * operation is one correctly rounded operation in the order written, unfused, denormals flushed on the way in and out; a NaN that is stored is 0x7FC00000.
 *   On the host, once per call:  W = glrt_mat4_inverse(c2w_prev), S = glrt_mat4_inverse(s2c_prev) -- the host library's routine, compiled from the same source
 *   (host/mat4_inverse.h); o_prev = features' centre_ray origin for the previous camera, w_k = (C[k] * 0 + C[12 + k]) + C[4 + k] * 0 for the rows k = 0..3 of
 *   C = c2w_prev, o_prev = (w_0 / w_3, w_1 / w_3, w_2 / w_3); a denormal tolerance counts as 0.  W, S, cur's c2w and s2c are the arithmetic's matrix inputs.
 *   Per pixel (x, y) of the new view, `width` x `rows` pixels.  "No history" means out = {0, 0, 0, 0}.  "A positive finite number": sign bit clear, exponent
 *   field neither 0 nor 255.
 *     No history when A1.id < 0 (a miss; the reserved id INT32_MIN is negative too) or N1.t is not a positive finite number.  Otherwise:
 *     1  (o, d) = the feature pass's centre ray of (x, y) for cur (csrc/features.hip.h: centre_ray -- that function, not a copy).
 *     2  P = o + t d per component (o.x + t * d.x), t = N1.t.
 *     3  q = W (P, 1): q_k = ((W[k] * P.x + W[4 + k] * P.y) + W[8 + k] * P.z) + W[12 + k];  s = S q: s_k = ((S[k] * q.x + S[4 + k] * q.y) + S[8 + k] * q.z) + S[12 + k] * q.w
 *        (k = 0, 1, 3).  No history unless s.w is a positive finite number.  u = ((s.x / s.w + 1) * 0.5) * width + -1, v = ((s.y / s.w + 1) * 0.5) * rows + -1:
 *        the inverse of centre_ray's ((x + 0.5 + 0.5) / width) * 2 - 1, so an unmoved camera gives u ~ x.  No history unless -1 <= u < width and -1 <= v < rows
 *        (outside, no tap lies in the image; a NaN fails).
 *     4  The distance the old view should have seen: e = sqrt((dz dz + dy dy) + dx dx) over (dx, dy, dz) = P - o_prev.
 *     5  Taps (x0 + i, y0 + j), x0 = floor(u), y0 = floor(v), i, j in {0, 1}, j outermost; fx = u - x0, fy = v - y0; the tap's weight is w = wx_i * wy_j with
 *        wx_0 = 1 - fx, wx_1 = fx, wy likewise.  A tap COUNTS only if it lies inside the image, its accumulator count acc.w is neither a zero nor a denormal,
 *        A0.id == A1.id, dot(N1.n, N0.n) >= normal_tolerance with the renderer's dot (az bz + ay by) + ax bx (a NaN fails), and
 *        |N0.t - e| <= depth_tolerance * e (a NaN fails).
 *     6  Over the taps that count, from 0, in tap order:  sw = sw + w;  sc = sc + w * acc.w;  sI = sI + w * (acc.rgb / acc.w) per channel.
 *     7  No history unless sw > 1e-6.  r = rint(sc / sw) (to nearest, ties to even -- not floor: an unmoved camera keeps its counts whatever the last ulp of the
 *        weights is); n = r > max_history ? max_history : r (max_history converted to float); no history unless n >= 1 (a NaN fails).
 *        out = {(sI.r / sw) * n, (sI.g / sw) * n, (sI.b / sw) * n, n}.
 * Out of scope: reprojection assumes STATIC geometry between the two views -- after a glrtx_update_vertices only the depth, normal and id tests protect the
 * history (glrtx_reproject_motion below is the call for moved geometry); specular history is view-dependent and is carried as if it were diffuse; glrt_main has no moving camera, so the facade does not call it. */
typedef struct glrtx_reproject_cfg {
    int   max_history;       /* >= 1: cap on the count a pixel carries over */
    float depth_tolerance;   /* > 0, finite: relative */
    float normal_tolerance;  /* finite: least dot(n_new, n_old) */
} glrtx_reproject_cfg;
int glrtx_reproject(glrtx_ctx *ctx, const glrtx_params *cur, const glrtx_reproject_cfg *cfg);
int glrtx_reproject_last(glrtx_ctx *ctx, int *carried, int *hit_pixels);
int glrtx_debug_reproject(const float *accum, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev, const float *s2c_prev,
                          const float *c2w_cur, const float *s2c_cur, int width, int rows, const glrtx_reproject_cfg *cfg, float *out, int *carried, int *hit_pixels);

/* ---- Reprojection across a geometry move: the same carry-over when glrtx_update_vertices moved the surfaces between the two views (SVGF's motion vector; no
 * reference counterpart; everything here is off unless glrtx_track_motion switched it on, and no other call changes what it does).
 *   glrtx_track_motion(enable)  off by default.  While it is on:
 *                          (a) every feature pass -- glrtx_render_features and the passes inside glrtx_reproject and glrtx_reproject_motion -- also writes a third
 *                          context-owned plane G beside N and A, of the same packed layout, allocated and released as they are and double-buffered as they are
 *                          (the reprojections swap three pairs): on a hit {tri, u, v, 0} -- the wire triangle index as int32 bits, mapped as glrtx_trace_rays
 *                          maps it, and the traversal's own barycentrics --, on a miss {-1, 0, 0, 0}.  N and A are bit for bit what they are with tracking off.
 *                          (b) the context keeps the PREVIOUS geometry: per wire triangle the three positions and vertex normals as they stood at the last
 *                          feature pass.  The first glrtx_update_vertices / _device after a feature pass copies them out of the scene on the device, on the
 *                          context's stream, before the refit; later updates before the next feature pass leave that copy alone; if nothing moved since the
 *                          last feature pass, previous and current are the same data.  glrtx_upload_scene forgets the previous geometry (until the next feature
 *                          pass).  glrtx_group_update_vertices goes through the members' glrtx_update_vertices.
 *                          Switching it off syncs, forgets the previous geometry and releases G and the copy.  Switching it on makes nothing known: render the
 *                          features before the first move.
 *   glrtx_read_features_geom    syncs, then copies G like glrtx_read_features.  GLRTX_EINVAL while tracking is off or before a feature pass wrote a G.
 *   glrtx_reproject_motion(cur) glrtx_reproject step for step -- the seal, the waits, the swaps, the feature pass for `cur`, the kernel into the second accumulator,
 *                          the accumulator switch, the zeroed half buffer, the counts glrtx_reproject_last reports, the refusals -- with the arithmetic below.
 *                          It also refuses, nothing changed, while tracking is off, before a feature pass wrote a G, and when the previous geometry is not
 *                          known (a glrtx_upload_scene since the last feature pass).  With the camera moved as well, `cur` is the new camera: both moves are
 *                          carried at once.
 *   glrtx_debug_reproject_motion  the kernel on caller arrays, no context: glrtx_debug_reproject's with G1 in place of N1 (the new view's camera enters through
 *                          the planes alone, so it is not an argument), the previous vertices (n_vert x 15 floats, wire format) and the triangles (n_tri x 4).
 *                          Its refusals, and a triangle with a vertex index out of range.
 * The arithmetic (the contract; glrt_reproject_motion in glrt_host.h and tests/reproject_motion_math.py state it again, and the three agree bit for bit), under
 * the rules of "Reprojection" above: one correctly rounded fp32 operation at a time in the order written, unfused, denormals flushed in and out, a stored NaN
 * is 0x7FC00000; W, S and o_prev as there.  Per pixel of the new view:
 *     No history when A1.id < 0, or G1.tri < 0, or G1.tri is not below the number of triangles the previous geometry holds.  N1 is not read.  Otherwise:
 *     2' p0, p1, p2 and n0, n1, n2: the PREVIOUS positions and vertex normals of wire triangle G1.tri; (u, v) = (G1.y, G1.z).  e1 = p1 - p0, e2 = p2 - p0 as the
 *        scene upload forms a leaf record's edges: one IEEE subtraction each with denormals KEPT (they are flushed when the next line reads them).
 *        P = (p0 + u * e1) + v * e2 per component.  m = the renderer's shading normal (surf_tri, csrc/pt_kernel.hip.h -- that function) of (n0, n1, n2) at
 *        (u, v): w0 = (1 - u) - v, t = (w0 * n0 + u * n1) + v * n2 per component, m = t * (1 / sqrt((t.z t.z + t.y t.y) + t.x t.x)).
 *     3, 4  as there, with this P.
 *     5  as there, except that the normal test is dot(m, N0.n) >= normal_tolerance: m is what the old view should have seen at that point (the new normal
 *        of a turned object says nothing about its old one).
 *     6, 7  unchanged.
 * Out of scope: changes of topology; spheres and the volume; specular history (carried as if it were diffuse); lighting that changes because geometry moved
 * (shading near a moved object's shadow stays stale until new samples outweigh it); partitioned contexts and groups.  The facade calls this from
 * glrt_main --animate --carry-history ("Posing" below; host/window.h: setAnimation). */
int glrtx_track_motion(glrtx_ctx *ctx, int enable);
int glrtx_read_features_geom(glrtx_ctx *ctx, float *geom, size_t pitch_bytes);
int glrtx_reproject_motion(glrtx_ctx *ctx, const glrtx_params *cur, const glrtx_reproject_cfg *cfg);
int glrtx_debug_reproject_motion(const float *accum, const float *n0, const float *a0, const float *g1, const float *a1, const float *vert_prev, size_t n_vert,
                                 const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width, int rows, const glrtx_reproject_cfg *cfg,
                                 float *out, int *carried, int *hit_pixels);

/* ---- Tone mapping: a luminance histogram, an automatic exposure and a tone curve between the HDR buffers and a displayable image (no reference counterpart
 * beyond op 0: the reference's screen.frag is clamp(mean, 0, 1) and a gamma curve; off unless called: no other call changes what it does, and nothing here ever
 * writes the accumulator, the denoised image D, the moments, the adaptive half buffer, the present ring or the ray counts).  The SOURCE is the accumulator
 * (source = 0) or D (source = 1; glrtx_denoise or glrtx_denoise_variance must have run at the image's current shape), over the context's owned rows taken as
 * one image in local row order: a partitioned context measures and maps its own rows.  Every call here runs on the context's stream and seals an open fed launch
 * first.  The context owns an exposure block in device memory (allocated by the first call here) -- the histogram and the exposure E -- and a float4 plane T
 * (packed rows of `width`; allocated by the first glrtx_tonemap, released by glrtx_resize and so by a partition change; the exposure block survives both).
 *   glrtx_exposure_measure   histogram and reduce, below; updates E on the device.  No host sync.
 *   glrtx_exposure_reset     forgets E (stream-ordered): the next measurement jumps to its target, as the first one after glrtx_create does.
 *   glrtx_read_exposure      syncs, then copies the block: the histogram, counted = N, kept = K, mean_log2, target, exposure = E of the LAST measurement, and
 *                            the number of measurements since create / reset (0: nothing measured yet; hist and the rest are zeros, E counts as 1).
 *   glrtx_tonemap            writes T = {y.rgb, 1}, below.  No host sync.  The kernel reads E in device memory: measure-then-map needs no host round trip.
 *   glrtx_read_tonemapped    syncs, then copies T like glrtx_read_accum.  GLRTX_EINVAL before a glrtx_tonemap at the image's current shape.
 *   glrtx_resolve_tonemapped_rgba8   source -> bytes in one pass (T is neither read nor written): the curve, then glrtx_resolve_rgba8's own arithmetic on {y, 1}
 *                            with cfg's gamma and flip_y (flipped within the owned rows, as there).  Syncs and copies like glrtx_resolve_rgba8.
 *   glrtx_debug_tonemap      all of it on caller arrays on the current HIP device, no context: src is width x rows float4, rows packed (cfg->source is not read).
 *                            One measurement with *exposure_in as the previous E (NULL: there is none, the measurement is a first one), reported in exp_out
 *                            (measurements = 1); then the curve with the E just measured into t_out (width x rows float4) and the fused kernel into rgba8_out
 *                            (width x rows x 4 bytes).  exp_out, t_out and rgba8_out may each be NULL.
 *   GLRTX_EINVAL, nothing changed (every call that takes a cfg checks all of it): a NULL cfg; op outside 0..2; source outside 0..1; exposure, key, white or gamma
 *   that is not a positive finite number, or a white whose square is not a normal finite number; adapt outside (0, 1]; not 0 <= low_permille < high_permille
 *   <= 1000; no accumulator; source = 1 without a denoised image of the current shape.
 * The arithmetic (this text is the contract; glrt_exposure_measure / glrt_tonemap in glrt_host.h and tests/tonemap_math.py state it again, and the three agree
 * bit for bit).  Every fp32 operation is one correctly rounded operation in the order written, unfused, denormals flushed on the way in and out (lp_exp and the
 * resolve carry their own fused ones); min / max are selects as written.
 *   Pixel value.  I = src.rgb / src.w, the IEEE quotient per channel.  A pixel is DEAD when src.w is a zero, a denormal or a NaN.
 *   Histogram.  l = lum(I) = (0.2126 I.r + 0.7152 I.g) + 0.0722 I.b ("Variance guidance").  Not counted: dead pixels, and l that is NaN, +inf or <= 0 (after the
 *     flush).  Otherwise k = clamp((bits(l) >> 20) - 888, 0, 255) in integer arithmetic on l's bit pattern: eight bins an octave from 2^-16 to 2^16, no
 *     transcendental.  hist[k] is a uint32 count.
 *   Reduce.  N = sum hist;  lo = N * low_permille / 1000 and hi = N * high_permille / 1000, floored uint64.  With c_k the exclusive prefix sum,
 *     kept_k = max(0, min(c_k + hist[k], hi) - max(c_k, lo));  K = sum kept_k;  S = sum kept_k * (2 k + 1).
 *     mean_log2 = (float)((double)S / (double)(16 K) - 16.0)    (IEEE double quotient and difference, one rounding to float: the mean of the kept pixels' bin centres)
 *     target = key * lp_exp((0.0f - mean_log2) * 0x1.62e430p-1f)       lp_exp: the renderer's exponential (csrc/pt_kernel.hip.h)
 *     With K = 0: mean_log2 = 0 and target = the previous E, or 1 if there is none.
 *     The first measurement after glrtx_create / glrtx_exposure_reset sets E = target; later ones E = E + (target - E) * adapt.
 *   Curve.  s = auto_exposure ? E * exposure : exposure  (E = 1 while nothing has been measured).  Per channel: x = I * s;  x = x > 0 ? x : 0 (a NaN becomes 0);
 *     x = x < 65504 ? x : 65504;
 *         op 0 (screen.frag's clamp)     y = x
 *         op 1 (Reinhard extended)       y = (x * (1 + x / (white * white))) / (1 + x)
 *         op 2 (ACES fit, Narkowicz)     y = (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f)
 *     A dead pixel gives y = {0, 0, 0}.  T = {y, 1}.
 *   Bytes.  glrtx_resolve_tonemapped_rgba8 equals glrtx_resolve_rgba8's kernel applied to T, byte for byte (the resolve's clamp to [0, 1], gamma curve and
 *     rounding).  It follows that op 0 with exposure = 1 and auto_exposure = 0 gives glrtx_resolve_rgba8's own bytes on any accumulator whose live pixels are
 *     finite and whose dead pixels are zeros.
 * Out of scope: the present ring and groups (no group call); a luminance-only curve (the curve is per channel, so saturated colours desaturate towards white);
 * local operators. */
typedef struct glrtx_tonemap_cfg {
    int   op;             /* 0 = screen.frag's clamp, 1 = Reinhard extended, 2 = ACES fit (Narkowicz) */
    int   source;         /* 0 = accumulator mean, 1 = denoised image D (glrtx_denoise / _variance must have run) */
    int   auto_exposure;  /* 0: scale = exposure; 1: scale = E * exposure, E the context's measured exposure */
    float exposure;       /* linear multiplier, > 0, default 1 */
    float key;            /* default 0.18 */
    int   low_permille, high_permille;   /* histogram window, 0 <= low < high <= 1000, default 500 / 950 */
    float adapt;          /* (0, 1]: share of the way E moves towards its target per measurement; 1 jumps */
    float white;          /* Reinhard white point, default 4 */
    float gamma; int flip_y;
} glrtx_tonemap_cfg;
typedef struct glrtx_exposure { uint32_t hist[256]; uint64_t counted, kept; float mean_log2, target, exposure; int measurements; } glrtx_exposure;
int glrtx_exposure_measure(glrtx_ctx *ctx, const glrtx_tonemap_cfg *cfg);
int glrtx_exposure_reset(glrtx_ctx *ctx);
int glrtx_read_exposure(glrtx_ctx *ctx, glrtx_exposure *out);
int glrtx_tonemap(glrtx_ctx *ctx, const glrtx_tonemap_cfg *cfg);
int glrtx_read_tonemapped(glrtx_ctx *ctx, float *dst_rgba, size_t dst_pitch_bytes);
int glrtx_resolve_tonemapped_rgba8(glrtx_ctx *ctx, uint8_t *dst, size_t dst_pitch_bytes, const glrtx_tonemap_cfg *cfg);
int glrtx_debug_tonemap(const float *src, int width, int rows, const glrtx_tonemap_cfg *cfg, const float *exposure_in, glrtx_exposure *exp_out, float *t_out,
                        uint8_t *rgba8_out);
/* Device time of one pass by itself, like glrtx_debug_resolve_burst: `reps` launches back to back between one pair of events after a warm-up pass, per launch.
 * which: 0 glrtx_resolve_rgba8's kernel on the cfg's source (the yardstick, in the same run), 1 the fused tone-mapping resolve, 2 glrtx_tonemap's kernel, 3 one
 * measurement (histogram + reduce; E moves as after that many measurements). */
int glrtx_debug_tonemap_burst(glrtx_ctx *ctx, const glrtx_tonemap_cfg *cfg, int which, int reps, float *ms_per_launch);

/* ---- Bloom: a glow around over-bright pixels, added to the linear HDR image in front of the tone curve (no reference counterpart; off unless called: no other
 * call changes what it does, and nothing here ever writes the accumulator, the denoised image D, the plane T but through glrtx_tonemap_bloomed, the moments, the
 * exposure block, the adaptive half buffer, the present ring or the ray counts).  The SOURCE is the accumulator (source = 0) or D (source = 1), as in "Tone
 * mapping".  Every call here runs on the context's stream and seals an open fed launch first.  The context owns the plane B (float4, packed rows of `width`, in
 * the accumulator's {rgb, w} form with w = 1) and the pyramid D_1 .. D_levels; the first glrtx_bloom allocates them, glrtx_resize releases them.
 *   glrtx_bloom                    fills B, below: 2 * levels kernel launches.  No host sync.
 *   glrtx_read_bloomed             syncs, then copies B like glrtx_read_tonemapped.  GLRTX_EINVAL before a glrtx_bloom at the image's current shape.
 *   glrtx_tonemap_bloomed          glrtx_tonemap with B as its source: writes T.  cfg->source is not read.  GLRTX_EINVAL before a glrtx_bloom at the current shape.
 *   glrtx_resolve_bloomed_rgba8    glrtx_resolve_tonemapped_rgba8 with B as its source.  cfg->source is not read.  GLRTX_EINVAL before a glrtx_bloom likewise.
 *                                  The exposure E is still measured by glrtx_exposure_measure on the unbloomed source; the curve reads it as it always does.
 *   glrtx_debug_bloom              the kernels on caller arrays on the current HIP device, no context: src is width x rows float4, rows packed (cfg->source is
 *                                  not read).  d_out receives D_1 .. D_levels packed back to back as float4 with w = 0 (the sum of w_k * h_k texels), copied before
 *                                  the up chain runs; b_out receives B.  Either may be NULL.
 *   glrtx_debug_bloom_burst        device time of one glrtx_bloom from `reps` of them back to back between one pair of events after a warm-up pass.
 *   GLRTX_EINVAL, nothing changed: a NULL argument; source outside 0..1; a threshold that is not finite and >= 0; a strength that is not in [0, 1e4] (a NaN
 *   among them); levels outside 1..8; no accumulator; source = 1 without a denoised image of the current shape; a partitioned context (world > 1: a seam per
 *   stripe would be wrong); glrtx_debug_bloom's sizes outside 1..65536.  Groups: no call.
 * The arithmetic (this text is the contract; glrt_bloom in glrt_host.h and tests/bloom_math.py state it again, and the three agree bit for bit).  Every fp32
 * operation is one correctly rounded operation in the order written, unfused, denormals flushed on the way in and out, as in "Tone mapping"; selects are as written.
 *   Pixel value.  I = src.rgb / src.w.  A pixel is DEAD as in "Tone mapping" (src.w a zero, a denormal or a NaN): x = {0, 0, 0}.  Otherwise per channel
 *     x = I > 0 ? I : 0 (a NaN becomes 0);  x = x < 65504 ? x : 65504.
 *   Bright pass.  l = lum(x) ("Variance guidance");  n = l - threshold;  n = n > 0 ? n : 0;  m = l > 1e-4f ? l : 1e-4f;  g = n / m (the IEEE quotient);
 *     D_0 = x * g per channel.  From here on every value is finite and >= 0.
 *   Down chain, k = 0 .. levels - 1.  Level 0 has the image's size w_0 x h_0 (owned rows);  w_{k+1} = (w_k + 1) >> 1, likewise h.
 *     c5(a, b, c, d, e) = ((a + e) + 4 * (b + d)) + 6 * c.  Clamp to edge: X(i) = clamp(2x + i, 0, w_k - 1), Y(j) = clamp(2y + j, 0, h_k - 1).
 *     r_j = c5(D_k(X(-2), Y(j)), D_k(X(-1), Y(j)), D_k(X(0), Y(j)), D_k(X(1), Y(j)), D_k(X(2), Y(j)))  for j = -2 .. 2
 *     D_{k+1}(x, y) = c5(r_-2, r_-1, r_0, r_1, r_2) * 0x1p-8f        (Burt and Adelson's binomial kernel, horizontal first; every weight is dyadic)
 *   Up chain.  up(C, w, h) of a wc x hc plane C:  near = x >> 1;  far = (x & 1) ? near + 1 : near - 1, both clamped to [0, wc - 1];
 *     hz(x, cy) = 0.75f * C(near, cy) + 0.25f * C(far, cy);  vertically the same rule on hz:  up(x, y) = 0.75f * hz(x, near_y) + 0.25f * hz(x, far_y).
 *     U_levels = D_levels;  for k = levels - 1 down to 1:  U_k = D_k + up(U_{k+1}, w_k, h_k);  glow = up(U_1, w_0, h_0) * (1.0f / (float)levels).
 *   B = {x + strength * glow, 1}.
 *   It follows that (1) a uniform image {0.5, 0.5, 0.5, 1} with threshold 0, strength 1 and levels 1, 2, 4 or 8 gives B.rgb == 1.0f at every pixel of every
 *   size, bit for bit; (2) when no pixel's luminance exceeds the threshold, and whenever strength is 0, B.rgb is x, bit for bit; (3) B is finite for every input.
 * The defaults -- threshold 1, strength 0.25, five levels -- are conventional values, not tuned on anything.
 * Out of scope: the present ring, groups and partitioned contexts; lens dirt, anamorphic streaks, a soft knee; measuring the exposure on B. */
typedef struct glrtx_bloom_cfg {
    int   source;     /* 0 = accumulator mean, 1 = denoised image D (as glrtx_tonemap_cfg.source) */
    float threshold;  /* luminance above which a pixel glows; finite, >= 0; default 1 */
    float strength;   /* finite, 0 <= strength <= 1e4; default 0.25 */
    int   levels;     /* 1..8; default 5 */
} glrtx_bloom_cfg;
int glrtx_bloom(glrtx_ctx *ctx, const glrtx_bloom_cfg *cfg);
int glrtx_read_bloomed(glrtx_ctx *ctx, float *dst_rgba, size_t dst_pitch_bytes);
int glrtx_tonemap_bloomed(glrtx_ctx *ctx, const glrtx_tonemap_cfg *cfg);
int glrtx_resolve_bloomed_rgba8(glrtx_ctx *ctx, uint8_t *dst, size_t dst_pitch_bytes, const glrtx_tonemap_cfg *cfg);
int glrtx_debug_bloom(const float *src, int width, int rows, const glrtx_bloom_cfg *cfg, float *d_out, float *b_out);
int glrtx_debug_bloom_burst(glrtx_ctx *ctx, const glrtx_bloom_cfg *cfg, int reps, float *ms_per_call);

/* ---- Firefly re-weighting: luminance cascades beside the accumulator and a resolve that keeps a brightness level only as far as the neighbourhood expects it
 * (Zirr, Hanika and Dachsbacher, "Re-weighting Firefly Samples for Improved Finite-Sample Monte Carlo Estimates", CGF 37(6), 2018; no reference counterpart;
 * everything here is off unless called: with tracking off no other call changes what it does or writes).  Meant for the image accumulated for a second or two
 * -- tens to hundreds of samples per pixel -- where no spatial filter is wanted and the remaining error is a few dozen lone samples.
 *   glrtx_track_cascades           enable != 0: keep the cascade planes C with bounds b_k = start * 8^k.  C is allocated, zeroed, on first use; zeroed by glrtx_clear
 *                                  and glrtx_bind_accum; released by glrtx_resize; enabling again with another start zeroes it (the bins were the old bounds').
 *                                  enable = 0 syncs and releases C (start is not read).  glrtx_reproject and glrtx_reproject_motion ZERO C if it exists: the bins
 *                                  belong to the old pixel grid (H's rule, not M's).
 *   glrtx_render_cascades          glrtx_render_moments with the other sink: plain launches with sample planes on the context's stream, in helpings, never fed; each
 *                                  is folded by one pass into the accumulator -- bit for bit glrtx_render_frames' -- and into C.  n_frames = 0 only allocates.
 *                                  Feeds C only: with glrtx_track_moments on as well, each render call feeds its own plane.
 *   glrtx_read_cascades            syncs, then copies the six planes back to back, owned rows each, rows dst_pitch_bytes apart (plane k at k * owned_rows rows).
 *   glrtx_reweight                 the resolve, below, into the image D {rgb, 1} -- the one glrtx_denoise writes: glrtx_read_denoised, glrtx_resolve_denoised_rgba8
 *                                  and source = 1 of the tone-mapping and bloom calls serve it unchanged.  Needs no feature planes.  On the context's stream, no
 *                                  host sync; seals an open fed launch.
 *   glrtx_debug_fold_cascades      the pass kernel on packed caller arrays on the current HIP device, no context: accum (width x rows float4), cascades (six such
 *                                  planes back to back), frames (n_frames planes, one sample each) -> accum_out, cascades_out (either may be NULL).
 *   glrtx_debug_reweight           the resolve kernel on caller arrays likewise: cascades -> out (width x rows float4).
 *   glrtx_debug_reweight_burst     device time of one resolve from `reps` launches back to back between one pair of events after a warm-up pass.
 *   GLRTX_EINVAL, nothing changed: a NULL argument; a start that is not within 2^-20 .. 2^20 (a NaN among them); a kappa that is not a positive finite number;
 *   glrtx_render_cascades: everything glrtx_render_moments refuses, with cascade tracking in the place of moments tracking; glrtx_read_cascades, glrtx_reweight:
 *   tracking off, no accumulator; glrtx_reweight also: C not yet allocated at the current shape, a partitioned context (world > 1: a seam per stripe); the debug
 *   calls' sizes outside 1..65536, n_frames < 0.  Groups: no call.
 * The arithmetic (this text is the contract; glrt_fold_cascades / glrt_reweight in glrt_host.h and tests/reweight_math.py state it again, and the three agree bit
 * for bit).  The rules are those of "Variance guidance": every fp32 operation is one correctly rounded operation in the order written, unfused; denormals are
 * flushed in and out; selects are as written; lum(r, g, b) = (0.2126 r + 0.7152 g) + 0.0722 b.
 *   Cascade planes.  Six float4 planes C_0 .. C_5 of the accumulator's pitch, {sum w r, sum w g, sum w b, count}.  b_k = start * 8^k: start is scaled by powers of
 *     two, so every b_k is exact.
 *   Fold, per sample v, before the accumulator's own add.  With l = lum(v):
 *     j = 0;  for k = 1 .. 4: if (l >= b_k) j = k                        (a NaN leaves j = 0)
 *     lower = b_j;  upper = b_{j+1}
 *     if (!(l > lower))     { wl = 1; wu = 0; jc = j }                   (l <= start, negatives, NaN)
 *     else if (l >= upper)  { wl = 0; wu = 1; jc = 5 }                   (only j = 4: at or beyond the top bound, +inf)
 *     else { q = lower / l;  wl = (q - 0.125f) / 0.875f;  wl = wl > 0 ? wl : 0;  wl = wl < 1 ? wl : 1;  wu = 1.0f - wl;  jc = j }
 *     C_j.rgb += wl * v.rgb  (three products, three adds; always performed, also with wl = 0);  C_{j+1}.rgb += wu * v.rgb;  C_jc.w += 1.0f
 *     No other plane is touched by that sample.  The split is Zirr et al.'s, linear in 1 / l: a sample contributes exactly 1 to sum_k lum(C_k) / b_k.  The count
 *     word is this library's addition (the paper estimates counts from lum(C_k) / b_k; the fourth word is free and holds the exact integer): sum_k C_k.w is the
 *     number of samples folded, exactly, and while every sample has l <= start, C_0 is the accumulator's own chain (1 * v = v).
 *   Resolve, per pixel p, into D {rgb, 1}:
 *     T_5 = C_5.w;  T_k = T_{k+1} + C_k.w for k = 4 .. 0                  (samples at level k or brighter)
 *     n = T_0(p).  DEAD when n is a zero, a denormal or a NaN: D = {0, 0, 0, 1}.
 *     for j = 1 .. 5:  s = 0;  over the 3x3 taps q = p + (dx, dy), dy outermost, inside the image (the owned rows as one image):  s = s + T_{j-1}(q)
 *                      s = s - 1.0f;  s = s > 0 ? s : 0;  r_j = s / kappa;  r_j = r_j < 1 ? r_j : 1
 *     per channel:     a = C_0.c(p);  for j = 1 .. 5:  a = a + r_j * C_j.c(p);      D.c = a / n      (a NaN is stored as 0x7FC00000)
 *     Cascade 0 always counts in full.  A brighter level counts as far as the 3x3 neighbourhood holds kappa samples at that level's lower neighbour or brighter,
 *     other than one: a lone sample supports nothing.  Being dimmer than the surroundings is never a firefly, hence "or brighter" and not the paper's j - 1 .. j + 1
 *     window; the ramp to kappa replaces the paper's global / local pair.  With 1 spp an interior pixel's neighbourhood holds 8 other samples, so kappa <= 8
 *     passes a uniformly bright region unchanged at 1 spp.
 *   It follows that (1) when every folded sample had l <= start and C and the accumulator were cleared together, D.rgb == acc.rgb / acc.w, bit for bit; (2) a
 *   5x5 image of eight samples {0.5, 0.5, 0.5} per pixel plus a ninth that is {5000, 5000, 5000} at the centre and {0.5, ...} elsewhere, start 1, kappa 4: the
 *   centre's counts are [8, 0, 0, 0, 1, 0], the centre resolves to 4.0f / 9.0f exactly and every other pixel to 0.5f; (3) D is finite whenever C is finite with
 *   integer counts (and the six colours' sum does not overflow).
 * The estimate is consistent: as samples build up every level becomes supported and D converges to the mean; it never exceeds the mean of non-negative samples.
 * Out of scope: carrying C through the reprojections; feeding C and M in one pass; adaptive launches, fed launches, the present ring, the megakernels and the
 * volume forms; groups and partitioned resolves; re-weighting in front of the denoisers (they read the accumulator); the paper's local-reliability term; more or
 * fewer than six cascades, a base other than 8. */
typedef struct glrtx_reweight_cfg {
    float kappa;  /* samples a 3x3 neighbourhood must hold besides one for a level to count in full; finite, > 0; default 4 */
} glrtx_reweight_cfg;
int glrtx_track_cascades(glrtx_ctx *ctx, int enable, float start);
int glrtx_render_cascades(glrtx_ctx *ctx, const glrtx_params *params, const float *seeds_xy, int n_frames);
int glrtx_read_cascades(glrtx_ctx *ctx, float *dst, size_t dst_pitch_bytes);
int glrtx_reweight(glrtx_ctx *ctx, const glrtx_reweight_cfg *cfg);
int glrtx_debug_fold_cascades(const float *accum, const float *cascades, const float *frames, int n_frames, int width, int rows, float start, float *accum_out,
                              float *cascades_out);
int glrtx_debug_reweight(const float *cascades, int width, int rows, const glrtx_reweight_cfg *cfg, float *out);
int glrtx_debug_reweight_burst(glrtx_ctx *ctx, const glrtx_reweight_cfg *cfg, int reps, float *ms_per_launch);

/* ---- Posing: rigid objects and linear-blend skinning on the device, in front of the refit (no reference counterpart; off unless called: no other call's
 * behaviour changes).  "Object 3 turned by this matrix" without the host touching a vertex: the rest pose stays on the device, a pose is a few matrices, and
 * one pass (csrc/skin.hip.h) writes the posed vertices where glrtx_update_vertices would have copied them.  A rigid object is the one-bone case.
 *
 * A RIG belongs to the uploaded scene.  It holds
 *   - the rest pose: n_vert wire vertices of GLRT_VERTEX_FLOATS = 15 floats each {pos, normal, uv, tangent, binormal};
 *   - per vertex four bone indices int32 b[4] and four weights float w[4];
 *   - a bone count n_bones, between 1 and 65536.
 * A POSE is n_bones matrices of 12 floats, row-major 3x4: m[i][0..2] is the linear part, m[i][3] the translation.
 *
 * Arithmetic.  Every operation is a single fp32 operation, correctly rounded and unfused.  Denormals count as zeros of their sign into and out of every
 * operation (the library's flags; tests/adaptive_math.py: _op, ftz).  A NaN that is stored is 0x7FC00000.  dot(a, v) is (a2 v.z + a1 v.y) + a0 v.x, the
 * project's order.  Per vertex:
 *   Blend     B[i][j] = ((w0 M_b0[i][j] + w1 M_b1[i][j]) + w2 M_b2[i][j]) + w3 M_b3[i][j], all twelve entries.  All four terms are always formed, so the
 *             operation sequence does not depend on the data.
 *   Position  pos'[i] = dot(B[i][0..2], pos) + B[i][3].
 *   Cofactor matrix.  With L = B[:, 0..2], each entry of C is two rounded products and one subtraction:
 *               C00 = L11 L22 - L12 L21    C01 = L12 L20 - L10 L22    C02 = L10 L21 - L11 L20
 *               C10 = L21 L02 - L22 L01    C11 = L22 L00 - L20 L02    C12 = L20 L01 - L21 L00
 *               C20 = L01 L12 - L02 L11    C21 = L02 L10 - L00 L12    C22 = L00 L11 - L01 L10
 *             (rows 1 and 2 are row 0 with the row indices advanced cyclically).  C equals det(L) L^-T: it turns a normal the way the transformed triangle's
 *             own cross product turns -- (L a) x (L b) = C (a x b) --, reflections included, so a posed normal stays on the side of the posed face it was on.
 *   Normal    v[i] = dot(C[i], normal);  s = dot(v, v);  l = sqrt(s) (IEEE);  normal' = l > 0 ? v / l : v, three IEEE quotients.
 *   Tangent and binormal  tangent'[i] = dot(L[i], tangent), binormal' likewise.  Neither is normalised; the renderer reads neither.
 *   uv        its three words are moved as integers.
 * It follows that a vertex with w = {1, 0, 0, 0} and finite matrices gets B == M_b0 up to the sign of a zero, and that the identity pose returns positions,
 * tangents and binormals unchanged (up to the sign of a zero; denormals as zeros).  Normals come back renormalised, which can differ from the input in the last
 * place.  The CPU statement is glrt_skin_vertices (include/glrt_host.h), bit for bit.
 *
 *   glrtx_upload_rig  keeps the rest pose and the rig on the device.  GLRTX_EINVAL, nothing changed: no scene, n_vert other than the scene's, a NULL pointer,
 *                     n_bones outside 1..65536, a bone index outside [0, n_bones), a non-finite weight.  glrtx_upload_scene forgets the rig;
 *                     glrtx_update_vertices / _device keep it: the rest pose is the rig's own copy, not the scene's vertices.
 *   glrtx_pose        uploads the matrices (n_bones x 48 bytes), runs the skinning kernel into the context's vertex buffer and then takes exactly
 *                     glrtx_update_vertices_device's path: an open fed launch is sealed, the motion snapshot is taken if glrtx_track_motion asks for one, the
 *                     refit runs behind every launch that may still read the scene, and the call returns when it has run.  Afterwards every device scene buffer
 *                     is byte for byte what glrtx_update_vertices(ctx, glrt_skin_vertices(...)) leaves.  GLRTX_EINVAL, nothing changed: no rig, a bone count
 *                     other than the rig's, a NULL pointer, a non-finite matrix entry (the entries are checked on the host before anything is issued).
 *   glrtx_debug_skin  the kernel alone on host arrays on the current HIP device, no context: vert_out gets n_vert wire vertices.  Refuses what glrt_skin_vertices
 *                     refuses (weights and matrices are not checked: the hook takes whatever the kernel can be handed).
 *   glrtx_debug_skin_burst  device time of the kernel by itself from `reps` launches back to back between one pair of events after a warm-up pass (the rig with
 *                     the last pose's matrices into the vertex buffer, which holds exactly that already).  GLRTX_EINVAL before a first glrtx_pose.
 * Groups: no call.  Pose a member through glrtx_group_ctx(grp, i).  glrtx_pose blocks as glrtx_update_vertices does, for the same read-back words. */
int glrtx_upload_rig(glrtx_ctx *ctx, const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, int n_bones);
int glrtx_pose(glrtx_ctx *ctx, const float *matrices, int n_bones);
int glrtx_debug_skin(const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *matrices, int n_bones, float *vert_out);
int glrtx_debug_skin_burst(glrtx_ctx *ctx, int reps, float *ms_per_launch);

/* ---- Deforming: morph targets and dual-quaternion skinning on the device, in the same place as Posing (no reference counterpart; off unless called: no other
 * call's behaviour changes).  Two things bones of matrices cannot say: a shape that is no bone's -- a face, a cloth or fluid cache, an OBJ sequence: blend
 * shapes --, and a twist that keeps its volume (linear blending takes a joint turned by 180 degrees between two bones to radius 0 at its mid ring).  One pass
 * (csrc/skin.hip.h: deform_kernel, deform_sparse_kernel) in front of the refit does both; everything behind it sees a vertex update, as after glrtx_pose.
 *
 * Arithmetic.  The rules are Posing's: one correctly rounded fp32 operation at a time, unfused, in the order written; denormals are zeros of their sign into
 * and out of every operation; a stored NaN is 0x7FC00000; dot(a, v) = (a2 v.z + a1 v.y) + a0 v.x; blend(w, m) = ((w0 m0 + w1 m1) + w2 m2) + w3 m3.
 *
 * MORPH TARGETS.  A rig may carry n_targets <= GLRTX_MAX_MORPH_TARGETS = 64 targets.  Each target is n_vert x 6 floats {dpos, dnormal}, target-major, dense.
 * A pose carries n_targets weights; they are checked finite on the host (a non-finite weight is GLRTX_EINVAL and nothing is issued).
 *   Active    a target is active iff |w| >= 2^-126 (non-zero after the flush).  Inactive targets are not read at all: a NaN or Inf delta under a zero weight
 *             changes nothing (the case a careless 0 * delta gets wrong).
 *   Morph     per vertex, over the active targets in ascending index:  p[i] = p[i] + w_k * dpos_k[i]  and  n[i] = n[i] + w_k * dnormal_k[i]  -- a rounded
 *             product, then a rounded sum --, starting from the rest position and normal.
 * Morphing runs before skinning (glTF's order): the morphed p, n and the rest tangent, binormal and uv then go through the skinning stage.  With no active
 * target the result is Posing's, bit for bit.
 *
 * DUAL-QUATERNION POSE.  n_bones x 8 floats {r.x, r.y, r.z, r.w, d.x, d.y, d.z, d.w}; w is the scalar part; d = 1/2 (t, 0) * r for a rotation r and a
 * translation t.  The values are checked finite, not checked for unit length.  dot4(a, b) = ((a.w b.w + a.z b.z) + a.y b.y) + a.x b.x.  Per vertex:
 *   Sign      s0 = w0;  for k = 1..3: h = dot4(r_b0, r_bk), s_k = h < 0 ? -w_k : w_k.  The negation flips the sign bit; a NaN h keeps w_k.
 *   Blend     R[j] = blend(s, r_b.[j]) and D[j] = blend(s, d_b.[j]): eight blends, all terms always formed.
 *   Normalise l = sqrt(dot4(R, R));  each of the eight entries becomes l > 0 ? x / l : x, IEEE quotients.
 *   Rotation  the nine products xx, yy, zz, xy, xz, yz, wx, wy, wz of R's x, y, z, w;
 *               L00 = 1 - 2 (yy + zz)    L01 = 2 (xy - wz)        L02 = 2 (xz + wy)
 *               L10 = 2 (xy + wz)        L11 = 1 - 2 (xx + zz)    L12 = 2 (yz - wx)
 *               L20 = 2 (xz - wy)        L21 = 2 (yz + wx)        L22 = 1 - 2 (xx + yy)
 *   Translation  t.x = 2 (((R.w D.x - D.w R.x) + R.y D.z) - R.z D.y);  t.y and t.z follow with x -> y -> z advanced cyclically.
 * From there the vertex is Posing's with B = [L | t]: position, the normal through the cofactor matrix and the l > 0 normalisation, tangent and binormal, uv
 * as words -- the text is Posing's.  Negating all eight floats of a bone changes nothing unless an h is exactly 0.  The CPU statement is glrt_deform_vertices
 * (include/glrt_host.h), bit for bit; glrt_dualquat_from_matrix there makes a bone's eight floats from a rigid 3x4 matrix.
 *
 *   glrtx_upload_morph_targets  keeps the deltas on the device in the layout they come in.  Needs a rig with that n_vert; n_targets == 0 drops the targets.
 *                     GLRTX_EINVAL, nothing changed: no rig, another n_vert, n_targets outside 0..64, NULL deltas.  glrtx_upload_rig and glrtx_upload_scene
 *                     forget the targets; glrtx_update_vertices / _device keep them.  Deltas are not checked, as rest vertices are not.
 *   glrtx_pose_morph  glrtx_pose with morph weights: matrices as there.  glrtx_pose_dualquat: the same with a dual-quaternion pose.  n_targets must be the
 *                     rig's; 0 with a NULL pointer is allowed when the rig has none.  Both take exactly glrtx_pose's path behind the kernel: the seal, the
 *                     motion snapshot, the refit and the same blocking read-back; afterwards every device scene buffer is byte for byte what
 *                     glrtx_update_vertices(ctx, glrt_deform_vertices(...)) leaves.  GLRTX_EINVAL, every device buffer untouched: no rig, a bone or target
 *                     count other than the rig's, a NULL pointer, a non-finite pose entry or morph weight.
 *   glrtx_debug_deform  the kernel alone on host arrays on the current HIP device, no context.  mode 0: bone_data is n_bones x 12 (matrices), 1: n_bones x 8
 *                     (dual quaternions).  Refuses what glrt_deform_vertices refuses (bone weights, bone data and deltas are not checked; morph weights are,
 *                     because the host decides from them which targets the kernel reads).
 *   glrtx_debug_deform_burst  device time of the kernel by itself, as glrtx_debug_skin_burst: the last glrtx_pose_morph / glrtx_pose_dualquat launch again,
 *                     whichever kernel that was (dense or sparse).  GLRTX_EINVAL before a first one.
 *
 * SPARSE TARGETS.  A rig carries EITHER a dense set (above, <= GLRTX_MAX_MORPH_TARGETS = 64 targets) OR a sparse set of n_targets <=
 * GLRTX_MAX_SPARSE_MORPH_TARGETS = 1024 targets, each of which lists only the vertices it moves.  The set is handed in by target, as glTF's sparse accessors do:
 *   offsets[n_targets + 1]  uint64, offsets[0] = 0, non-decreasing; nnz = offsets[n_targets] < 2^31; target k's entries are [offsets[k], offsets[k + 1])
 *   vertex[nnz]             uint32, strictly ascending inside a target, each < n_vert
 *   deltas[nnz x 6]         float {dpos, dnormal}, not checked (as dense deltas are not)
 * The rules are the dense form's, in Posing's arithmetic:
 *   Active    as above: a target is active iff |w| >= 2^-126.
 *   Morph     per vertex, over the entries that list this vertex and belong to an active target, in ascending target index:  p = p + w_k * dpos  and
 *             n = n + w_k * dnormal  -- a rounded product, then a rounded sum --, starting from the rest position and normal.  A vertex that no active target
 *             lists keeps its rest p and n untouched: no + 0 is formed.
 *   Inactive entries  an entry of an inactive target never enters the arithmetic: a NaN or Inf under a zero weight changes nothing.  It MAY BE LOADED -- the one
 *             place this wording is weaker than the dense form's "not read at all": the entries of a vertex lie side by side whatever target they belong to.
 *   Then the skinning stage, matrices or dual quaternions, unchanged.  With no active target the result is Posing's, bit for bit.
 * Two relations to the dense form:
 *   1. A sparse set in which every target lists every vertex performs the dense form's operation sequence: it equals the dense form bit for bit on any data.
 *   2. Dropping an entry whose six floats are all zeros after the flush (exponent field 0) changes the result at most in the sign of a zero, and changes
 *      nothing at all when no rest position or normal component is a negative zero or a negative denormal (precondition).  A rounded sum is -0 only if both
 *      operands are -0, so under the precondition p never becomes -0 and p + (+-0) = p.  Without it the two forms are NOT equal: -0 + (+0) is +0.
 * The CPU statement is glrt_deform_vertices_sparse (include/glrt_host.h), bit for bit; glrt_morph_sparsify there drops exactly the entries of relation 2.
 *
 *   glrtx_upload_morph_targets_sparse  transposes the set on the host into a vertex-major inverted index -- row[n_vert + 1] and 32-byte entries {target, dpos}
 *                     {dnormal, 0}, ascending by target inside a row -- and keeps that on the device: 4 (n_vert + 1) + 32 nnz bytes.  Needs a rig with that
 *                     n_vert.  GLRTX_EINVAL, nothing changed: no scene or no rig, another n_vert, n_targets outside 0..1024, a NULL array with entries to read
 *                     (nnz == 0 with NULL vertex and deltas is a valid set; n_targets == 0 needs no array), offsets[0] != 0 or decreasing offsets, nnz >=
 *                     2^31, an index >= n_vert, indices not strictly ascending inside a target; the message names the target and the entry.  Uploading either
 *                     kind of set replaces the other; n_targets == 0 through either call drops whatever is there; glrtx_upload_rig and glrtx_upload_scene
 *                     forget the set; glrtx_update_vertices / _device keep it.
 *   glrtx_pose_morph, glrtx_pose_dualquat  work with whichever set the rig holds: n_targets up to 1024 with a sparse set, and the rig's count as before.  The
 *                     weight table (n_targets floats, +0 for an inactive target) goes up per pose beside the bone data.  With no active weight, or nnz == 0,
 *                     the dense kernel runs with no active target and reads no entry at all.
 *   glrtx_debug_deform_sparse  the sparse kernel alone on host arrays on the current HIP device, no context.  Refuses what glrt_deform_vertices_sparse refuses,
 *                     before it touches a device.
 * Groups: no call. */
#define GLRTX_MAX_MORPH_TARGETS 64
#define GLRTX_MAX_SPARSE_MORPH_TARGETS 1024
int glrtx_upload_morph_targets(glrtx_ctx *ctx, const float *deltas, int n_targets, size_t n_vert);
int glrtx_pose_morph(glrtx_ctx *ctx, const float *matrices, int n_bones, const float *morph_weights, int n_targets);
int glrtx_pose_dualquat(glrtx_ctx *ctx, const float *dualquats, int n_bones, const float *morph_weights, int n_targets);
int glrtx_debug_deform(const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                       const float *deltas, const float *morph_weights, int n_targets, float *vert_out);
int glrtx_debug_deform_burst(glrtx_ctx *ctx, int reps, float *ms_per_launch);
int glrtx_upload_morph_targets_sparse(glrtx_ctx *ctx, const uint64_t *offsets, const uint32_t *vertex, const float *deltas, int n_targets, size_t n_vert);
int glrtx_debug_deform_sparse(const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                              const uint64_t *offsets, const uint32_t *vertex, const float *deltas, const float *morph_weights, int n_targets, float *vert_out);

/* ---- Rebuilding normals: shading normals rebuilt on the device from the moved surface (no reference counterpart; off unless called: no other call's behaviour
 * changes).  A bone carries its normals exactly (Posing's cofactor matrix).  A morph target does not: its normal is n + sum w dnormal, only as good as the deltas
 * the file carried, and glTF targets very often carry none.  A simulation or a cache gives positions and nothing else.  Three passes (csrc/normals.hip.h) make
 * area-weighted smooth normals from the triangles as they stand; they serve a position-only vertex update and an opt-in stage between the deform kernels and
 * the refit.
 *
 * Arithmetic.  The rules are Posing's: one correctly rounded fp32 operation at a time, unfused, in the order written; denormals are zeros of their sign into
 * and out of every operation; a stored NaN is 0x7FC00000; dot(a, b) = (a.z b.z + a.y b.y) + a.x b.x.
 *
 * TOPOLOGY.  Built on the host, once, from the rest vertices (n_vert x 15 floats, wire format) and the wire triangles (n_tri x 4 floats {i0, i1, i2,
 * material}, as glrtx_upload_scene takes them).
 *   Weld classes  two vertices are the same smooth vertex iff the six words of their rest position and rest normal are equal as 32-bit patterns; +0 and -0
 *             differ.  This welds the unindexed three-vertices-a-triangle meshes of the facade's OBJ reader and of scenes.SceneBuilder, and keeps a box's
 *             corners apart, because their normals differ.  With the flag GLRTX_NORMALS_WELD_POSITIONS = 1 only the three position words are compared: for
 *             meshes that carry no normals worth keeping.  Class ids ascend with each class's smallest member.
 *   Face list     a class's list holds the triangles with at least one corner in the class, each once, in ascending triangle index.
 *   Orientation   triangle t is FLIPPED iff, in the rest pose, dot(f, m) < 0, where f is its face vector (below) and m = (n0 + n1) + n2 per component over its
 *             corners' rest normals in corner order.  A NaN or a zero does not flip.  With this, rebuilt normals keep the side the authored normals were on,
 *             whatever the winding.
 *
 * REBUILD.  In place on n_vert wire vertices.  Positions are only read; normal words are the only ones written; no word is both read and written.
 *   Face vector   of triangle t with corners i0, i1, i2:  e1 = p[i1] - p[i0]  and  e2 = p[i2] - p[i0]  per component;
 *               f.x = e1.y e2.z - e1.z e2.y    f.y = e1.z e2.x - e1.x e2.z    f.z = e1.x e2.y - e1.y e2.x
 *             -- two rounded products and one subtraction a component.  If t is flipped, the three sign bits are inverted.  The vector is not normalised: the
 *             sum is area-weighted.
 *   Sum           of a class, over its face list in order, in chunks of GLRTX_NORMAL_CHUNK = 256 entries.  Inside a chunk  c = f_first, then c = c + f_next
 *             per component; across chunks  s = c_0, then s = s + c_k  in chunk order.  A list of up to 256 faces is a plain sequential sum.  The chunk rule
 *             is part of the contract so that a later kernel may hand a long list's chunks to separate waves without changing a bit; today every class is
 *             summed on one lane, in that order.  An empty list has s = 0.
 *   Normal        l = sqrt(dot(s, s)).  If l == 0 the normal words in place are KEPT: an empty list, a degenerate or exactly cancelling neighbourhood, a vertex
 *             that no triangle names.  Otherwise n = s / l, three IEEE quotients; a NaN goes through as the canonical NaN; l = +Inf gives zeros or NaN.  Every
 *             member of the class receives the same three words.
 * Tangents and binormals are not touched: the renderer reads neither, and they keep their rest or posed words.  The CPU statements are glrt_normal_topology
 * and glrt_rebuild_normals (include/glrt_host.h), bit for bit; glrt_positions_to_vertices there makes the records of a position-only update.
 *
 *   glrtx_upload_normal_topology  builds the topology (glrt_normal_topology's routine) and keeps on the device a copy of rest_vert (60 n_vert bytes) and the
 *                     index: 16-byte triangle records {i0, i1, i2, flip}, a class id a vertex, the face lists as rows -- 16 n_tri + 4 n_vert +
 *                     4 (n_classes + 1) + 4 entries bytes, entries being the summed length of the face lists (at most 3 n_tri) -- and 16 (n_tri + n_classes)
 *                     bytes of scratch for a rebuild.  GLRTX_EINVAL, nothing changed: no scene, n_vert other than the scene's, a NULL pointer, a corner index
 *                     that is not an integer in [0, n_vert), n_tri >= 2^31, an unknown flag (or face lists of 2^32 entries or more).  glrtx_upload_scene
 *                     forgets the topology and the switch below; glrtx_upload_rig, glrtx_update_vertices / _device and the morph uploads keep both; a second
 *                     upload replaces the topology and keeps the switch.
 *   glrtx_update_positions, glrtx_update_positions_device  pos: n_vert x 3 floats, in host memory or on the context's GPU (read on the context's stream, as
 *                     glrtx_update_vertices_device reads its vertices).  One kernel writes each vertex's record into the context's vertex buffer -- the new
 *                     position words, moved as integers, and the other twelve words from the topology's rest copy --, the rebuild runs on that buffer, and the
 *                     call then takes exactly glrtx_update_vertices_device's path: the seal, the motion snapshot when glrtx_track_motion asks for one, the
 *                     refit, the blocking read-back.  Afterwards every device scene buffer is byte for byte what glrtx_update_vertices(ctx, V) leaves, V being
 *                     glrt_rebuild_normals applied to glrt_positions_to_vertices(rest, pos).  GLRTX_EINVAL, every buffer untouched: no topology, another
 *                     n_vert, a NULL pointer.  The positions are not checked, as vertices are not.
 *   glrtx_set_pose_normals  off by default.  While on, glrtx_pose, glrtx_pose_morph and glrtx_pose_dualquat run the rebuild on the vertex buffer between their
 *                     deform kernel and the refit, with dense and with sparse sets.  The result is then what glrtx_update_vertices leaves for: the CPU pose or
 *                     deform statement, followed by glrt_rebuild_normals with the topology of the RIG's rest pose (the caller passes that rest pose to both
 *                     uploads).  A class with l == 0 keeps its posed normal.  Enabling without a topology is GLRTX_EINVAL.  While off, nothing about a pose
 *                     changes, with or without a topology.
 *   glrtx_debug_rebuild_normals  the three passes alone on host arrays on the current HIP device, no context, with a caller-made class map (any ids below
 *                     n_vert) and flip bytes (zero or not), so that tests can hand in classes no weld would make.  vert_out gets the n_vert wire vertices.
 *                     Refuses what glrt_rebuild_normals refuses: a class id >= n_vert, a corner out of range, a NULL pointer.
 *   glrtx_debug_normals_burst  device time of the rebuild by itself, as glrtx_debug_skin_burst: the three passes on the context's vertex buffer.  GLRTX_EINVAL
 *                     without a topology or before anything has filled the vertex buffer.
 * Groups: no call.  Pose or update a member through glrtx_group_ctx(grp, i).  Spheres, the volume and partitioned contexts are not involved. */
#define GLRTX_NORMALS_WELD_POSITIONS 1u
#define GLRTX_NORMAL_CHUNK 256u
int glrtx_upload_normal_topology(glrtx_ctx *ctx, const float *rest_vert, size_t n_vert, const float *tri, size_t n_tri, unsigned flags);
int glrtx_update_positions(glrtx_ctx *ctx, const float *pos, size_t n_vert);
int glrtx_update_positions_device(glrtx_ctx *ctx, const void *dev_pos, size_t n_vert);
int glrtx_set_pose_normals(glrtx_ctx *ctx, int enable);
int glrtx_debug_rebuild_normals(const float *vert_in, size_t n_vert, const float *tri, size_t n_tri, const uint32_t *class_of_vertex, const uint8_t *flip,
                                float *vert_out);
int glrtx_debug_normals_burst(glrtx_ctx *ctx, int reps, float *ms_per_launch);

/* ---- Textures: a diffuse material's albedo looked up in an image at the hit's texture coordinates (no reference counterpart -- the reference's Vertex carries
 * uv and its Material ends in texIds, and nothing reads either; off unless called: no other call's behaviour changes).  gfx950 has no image-sampling path: a
 * lookup is address arithmetic and up to four gathers (csrc/texture.hip.h).  Only the extension megakernel shades with textures: while a set is bound, launches
 * run on the persistent megakernel exactly as with analytic spheres uploaded (variant_last 1, GLRTX_FALLBACK_EXTENSIONS) -- by default: with
 * glrtx_set_texture_wavefront (below) the wavefront kernel's T form shades them, bit for bit the same.  PINNED through the reference all the
 * same: a texture whose texels are constant over each triangle renders, bit for bit, the image of the same geometry with one diffuse material a triangle.
 *
 * Arithmetic.  Every operation is one correctly rounded fp32 operation in the order written, unfused; denormals are zeros of their sign into and out of every
 * operation.  Three statements agree bit for bit: tex_lookup (csrc/texture.hip.h), glrt_texture_lookup (include/glrt_host.h), tests/texture_math.py.
 *
 * SET.  n_tex <= GLRTX_TEX_MAX = 4096 descriptors over one texel blob.  A descriptor: the byte offset of its first texel in the blob (a multiple of 16), width
 * and height in 1 .. GLRTX_TEX_MAX_DIM = 16384, a format, a wrap mode per axis, a filter.  Texels run row-major, x fastest; row 0 is t = 0.  No mip levels: a path
 * tracer without ray differentials has no footprint to choose one by (the volume lookups read textureLod(.., 0) for the same reason).
 * FORMATS.  GLRTX_TEX_RGBA32F: four floats a texel.  GLRTX_TEX_RGBA8_UNORM: four bytes, a channel is (float)b / 255.0f (one IEEE quotient).
 *   GLRTX_TEX_RGBA8_SRGB: four bytes, a channel is entry b of a table of 256 floats -- the piecewise sRGB formula (b / 255 <= 0.04045 ? c / 12.92 :
 *   ((c + 0.055) / 1.055) ^ 2.4) evaluated in float64 and rounded once to fp32; the table is stated as constants on each side (glrt_srgb_table), there is no
 *   pow at run time.  Alpha is never read by this lookup (a cutout record that names channel 3 reads it: "Cutouts", below).
 * COORDINATES.  A non-finite s or t is 0.  Per axis with N texels and coordinate s:
 *   GLRTX_TEX_REPEAT  x = s - floor(s).       GLRTX_TEX_CLAMP  x = s > 0 ? s : 0, then x = x < 1 ? x : 1.       a = x * (float)N.
 *   GLRTX_TEX_NEAREST   i = (int)floor(a); under repeat i >= N becomes i - N, under clamp i > N - 1 becomes N - 1.
 *   GLRTX_TEX_BILINEAR  b = a - 0.5, fl = floor(b), f = b - fl, i0 = (int)fl, i1 = i0 + 1; each index: under repeat i < 0 becomes i + N and i >= N becomes
 *                       i - N; under clamp i < 0 becomes 0 and i > N - 1 becomes N - 1.
 * FILTER (bilinear), per channel, with txy the decoded texel at column ix, row iy:  c0 = t00 + fx * (t10 - t00),  c1 = t01 + fx * (t11 - t01),
 *   c = c0 + fy * (c1 - c0).  Four equal texels give that texel's words exactly (d = 0, f * 0 = 0, t + 0 = t for the finite texels a texture should hold).
 *   Nearest returns the decoded texel.
 * AT A HIT of a triangle with vertices 0, 1, 2 in wire order and barycentrics (u, v):  w0 = (1 - u) - v,  s = (w0 * s0 + u * s1) + v * s2, t likewise -- the
 *   order surf_tri mixes the normals in.  (s, t) = words 6 and 7 of a wire vertex (uv.x, uv.y); uv.z is ignored.
 * SHADING.  A diffuse (type 2) material bound to texture k takes its albedo from the lookup wherever the reference reads param0: the BSDF value is albedo / PI
 *   (the division the material staging performs), the light sample's f is the albedo itself.  The texture REPLACES param0, it does not multiply it.  Analytic
 *   spheres have no coordinates: a sphere with a bound material shades with param0.
 *
 *   glrtx_upload_textures  copies descriptors and blob to the device and binds material m to texture material_texture[m] (-1: untextured).  The per-triangle
 *                     table of the three corners' (s, t) is built in this call from the vertices glrtx_upload_scene was given, and is FROZEN from then on:
 *                     glrtx_update_vertices*, glrtx_pose* and glrtx_update_positions* move geometry, not the mapping (their uv words are carried along and
 *                     not read again).  n_tex = 0 unbinds: the context renders as before.  glrtx_upload_scene drops the set, as it drops spheres.
 *                     GLRTX_EINVAL, everything unchanged, the offender named in the message: no scene uploaded; n_mat other than the scene's material count;
 *                     a texture index out of range; a binding on a material that is not diffuse; a descriptor with a zero or oversized dimension, an unknown
 *                     format, wrap or filter, or a misaligned offset; a texture whose last texel lies past texel_bytes; more than 2^31 - 1 texels in total;
 *                     more than GLRTX_TEX_MAX textures; a NULL pointer.
 *   While a set is bound these refuse with GLRTX_EINVAL and a message that says "textures are bound": glrtx_render_adaptive*, glrtx_render_moments,
 *                     glrtx_render_cascades and glrtx_hit_histogram (the wavefront kernel's calls).  The present ring works as it does with spheres.
 *   Feature pass      with a set bound, plane A of glrtx_render_features carries the looked-up albedo of a textured diffuse hit (the material id is unchanged),
 *                     so `demodulate` keeps texture detail out of both denoisers' filters.  glrt_texture_albedo (include/glrt_host.h) states it on plane G.
 *   glrtx_debug_texture_lookup  tex_lookup on caller arrays on the current HIP device, no context: rgb_out[3i..] = lookup(which[i], st[2i], st[2i + 1]).
 *                     Refuses what glrtx_upload_textures refuses of a set, and a `which` out of range.  Errors through glrtx_last_error(NULL).
 *   glrtx_set_texture_wavefront  1: launches with a set bound run on the wavefront kernel (variant 2) -- its T form, or its TM form while material maps are bound
 *                     (below) -- instead of the persistent megakernel: variant_last reports 2, fallback_last 0, and the launch is not counted in
 *                     fallback_launches.  Frames in flight, overlapped and fed launches and the fused present ring then work with the set bound, and so do
 *                     glrtx_render_adaptive, glrtx_render_adaptive_moments, glrtx_render_moments and glrtx_render_cascades.  TAKEN when the set is all that
 *                     needs the extension kernel: variant 2 selected, no GLRTX_EXT_* flag, no spheres, no environment, the tree not a vine (the list scan has
 *                     no textured form), u_maxDepth <= 255 and u_nSamples < 2^20.  ANYTHING ELSE runs exactly as with the switch off -- the textured megakernel,
 *                     variant_last 1, GLRTX_FALLBACK_EXTENSIONS and the depth / sample bits where they apply -- and the wavefront kernel's calls then refuse
 *                     as above, the message naming the reason (the switch is off, spheres, an environment, ...).  glrtx_hit_histogram refuses while a set
 *                     is bound either way.  EQUALS the megakernel's textured kernels bit for bit: images, sample counts, rays, rays_untraced and paths (the
 *                     shade phase calls the same lookup and shading functions on the hit record the traverse phase left).  A forced GLRTX_PAIR_FETCH=2 is
 *                     served as 0 (node_fetch_last says what ran).  Default 0; GLRTX_TEXTURE_WAVEFRONT=0/1 in the environment overrides it at every launch.
 *                     NULL ctx: GLRTX_EINVAL.  Seals an open fed launch, as glrtx_upload_textures and glrtx_bind_material_maps do.
 * Groups: no call; a member is reached through glrtx_group_ctx(grp, i). */
int glrtx_set_texture_wavefront(glrtx_ctx *ctx, int enable);
#define GLRTX_TEX_MAX 4096
#define GLRTX_TEX_MAX_DIM 16384
enum glrtx_tex_format { GLRTX_TEX_RGBA32F = 0, GLRTX_TEX_RGBA8_UNORM = 1, GLRTX_TEX_RGBA8_SRGB = 2 };
enum glrtx_tex_wrap { GLRTX_TEX_REPEAT = 0, GLRTX_TEX_CLAMP = 1 };
enum glrtx_tex_filter { GLRTX_TEX_NEAREST = 0, GLRTX_TEX_BILINEAR = 1 };
typedef struct glrtx_texture {
    uint64_t offset;        /* bytes from the start of the blob; a multiple of 16 */
    int32_t width, height;  /* 1 .. GLRTX_TEX_MAX_DIM */
    int32_t format;         /* glrtx_tex_format */
    int32_t wrap_s, wrap_t; /* glrtx_tex_wrap */
    int32_t filter;         /* glrtx_tex_filter */
} glrtx_texture;
int glrtx_upload_textures(glrtx_ctx *ctx, const glrtx_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *material_texture,
                          size_t n_mat);
int glrtx_debug_texture_lookup(const glrtx_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const float *st, size_t n,
                               float *rgb_out);

/* ---- Environment: light from an HDR map where a ray leaves the scene (no reference counterpart -- the reference's misses return black; PARITY UNPINNED; off
 * unless called: no other call's behaviour changes).  One image, SQUARE, N x N with N in 2 .. GLRTX_TEX_MAX_DIM, described by a glrtx_texture (offset 0): any of
 * the three formats, nearest or bilinear, wrap GLRTX_TEX_CLAMP on both axes.  The layout is OCTAHEDRAL with +y as the fold axis, not lat-long: direction ->
 * (s, t) is three absolute values, one quotient and a few selects on a shading path that is bound by instruction issue; lat-long needs atan2 and acos, which
 * have no bit-exact statement here.  While an environment is bound, launches run on the persistent megakernel exactly as with analytic spheres uploaded
 * (variant_last 1, GLRTX_FALLBACK_EXTENSIONS), in kernels of their own (pt_render_persistent's ENV forms); textures, spheres, GLRTX_EXT_DIELECTRIC and
 * GLRTX_EXT_WHITTED combine with it, GLRTX_EXT_VOLUME does not.
 *
 * Arithmetic.  Every operation is one correctly rounded fp32 operation in the order written, unfused; denormals are zeros of their sign into and out of every
 * operation.  Three statements agree bit for bit: csrc/environment.hip.h, glrt_env_* (include/glrt_host.h), tests/env_math.py.
 *
 * DIRECTION TO (s, t).  d is the ray direction as the path carries it (not normalised along a path); R = rotation, row-major 3 x 3.
 *   e = R d, each row (R0 * dx + R1 * dy) + R2 * dz.   l = (|ex| + |ey|) + |ez|.   l zero or not finite: the radiance is 0.
 *   px = ex / l, pz = ez / l.   For ey < 0 (a -0 does not fold):  px' = (1 - |pz|) * sgn(px),  pz' = (1 - |px|) * sgn(pz),  sgn(0) = sgn(-0) = +1.
 *   s = px * 0.5 + 0.5,  t = pz * 0.5 + 0.5.   The L1 norm of the unit direction, for the pdf: py = ey / l, n1 = 1 / sqrt((pz * pz + py * py) + px * px), from the
 *   quotients before the fold.   So +y is the centre of the square, -y its four corners, +x the middle of the right edge, +z of the top edge.
 * RADIANCE.  Le = scale * lookup(map, s, t), per channel; the lookup is the one of "Textures", as it is.  Bilinear filtering across the fold seams is NOT
 *   corrected: at the square's edge a lookup reads what clamp gives it, not the texel on the other side of the fold.
 * INVERSE.  u = s * 2 - 1,  v = t * 2 - 1,  y = (1 - |u|) - |v|.   For y < 0:  x = (1 - |v|) * sgn(u),  z = (1 - |u|) * sgn(v);  else x = u, z = v.
 *   r = 1 / sqrt((z * z + y * y) + x * x),  q = (x, y, z) * r,  direction = R^T q, each component (R0c * qx + R1c * qy) + R2c * qz.
 * SOLID ANGLE.  dOmega = 4 n1^3 ds dt with n1 = r * ((|x| + |y|) + |z|), the L1 norm of the unit direction (an octahedron face lies at distance 1 / sqrt(3)
 *   from the origin, which gives dOmega = du dv / |p|^3); J = 4 * ((n1 * n1) * n1).  The integral over the square is 4 pi.
 *
 * ESTIMATORS (glrtx_env_cfg::mode).  The reference estimates direct light by next-event estimation without MIS and counts emission met by a path only at
 *   depth 0; the extension kernel also counts it behind a specular bounce.  Both modes keep that design and converge to the same image.
 *   GLRTX_ENV_ESCAPE   wherever a path's ray misses, L += beta * Le(d), at every depth.  No extra random number, no extra ray: with a map of zeros, or scale
 *                      0, image and ray count are those without a map, bit for bit.
 *   GLRTX_ENV_SAMPLED  the environment is one more light of sampleDirect.  At a miss Le is added only at depth 0 or behind a specular bounce (the emitter rule).
 *                      Light pick: rl = rand() as before; rl < p_env takes the environment, else lid = (int)(((rl - p_env) / (1 - p_env)) * nLights), clamped
 *                      as before, and the triangle light's pdf is multiplied by (1 - p_env).  p_env = light_pick, forced to 1 for a scene without lights; with
 *                      light_pick = 0 both expressions are the reference's exactly and so are the random stream and the image wherever no primary ray misses.
 *                      The environment branch draws six more numbers u0 .. u5: row cj = cell(u0), cj = u1 < row_q[cj] ? cj : row_alias[cj]; column
 *                      ci = cell(u2), k = cj * G + ci, ci = u3 < col_q[k] ? ci : col_alias[k]  (cell(u) = (int)(u * G) kept in 0 .. G - 1);
 *                      s = (ci + u4) / G, t = (cj + u5) / G; the direction w by INVERSE; Le by RADIANCE at that (s, t);
 *                      pdf = ((cell_p[cj * G + ci] * (G * G)) / J) * p_env;  the sample contributes Le * f * (n . w) / pdf when n . w > 0 and pdf > 0, with f
 *                      the BSDF VALUE (diffuse: albedo / PI, textured albedo included; conductor: the block the light sample evaluates) -- not the
 *                      reference's albedo without 1 / PI, which stays with the triangle lights, where it is pinned.  The shadow ray has no far end: the
 *                      sample is accepted when the ray hits nothing, spheres included.  It counts as one ray.
 *   WHY SAMPLED FOR A SUN.  The accumulation clamps each sample at 100.  In escape mode a path that finds a 50 000-nit sun is clamped: a bias.  In sampled
 *                      mode a sample is Le f cos / pdf, bounded by the irradiance, and stays under the clamp.
 * IMPORTANCE GRID.  G x G cells over the square; G = cfg.grid (1 .. 1024; 0: min(N, 256)).  The weight of cell (row j, column i) is the sum of
 *   max(lum(scale * texel), 0) * J at the texel centres ((x + 0.5) / N, (y + 0.5) / N) over the texels x in max(i * N / G - 1, 0) .. min(ceil((i + 1) * N / G),
 *   N - 1) (integer quotients) and y likewise from j: the texels that overlap the cell, WIDENED by one on every side -- a bilinear lookup inside the cell reads
 *   no texel outside that block, so the radiance is never positive where the pdf is zero.  lum(r, g, b) = (0.2126 r + 0.7152 g) + 0.0722 b.  A weight that is
 *   not finite counts as 0.  Order of the sum (env_weights_kernel, one wave a cell): partial sum k of 64 adds the block's texels k, k + 64, .. (row-major in
 *   the block) in that order from 0; then p[k] += p[k + h] for h = 32, 16, .. 1.  The tables are built on the host from those weights: Vose's alias method in
 *   float64 in a stated order (host/env_tables.h), thresholds rounded once to fp32; a row table over the rows' sums, one column table a row,
 *   cell_p = (float)(w / total).  An all-zero grid is legal: sampled mode then never contributes, and the miss rule still applies.
 *
 *   glrtx_upload_environment   copies the map and builds the tables; map == NULL unbinds (the context renders as before, variant_last back to what it was).  The
 *                     map does not depend on the scene and is KEPT across glrtx_upload_scene, as the volume is.
 *   glrtx_set_environment_cfg  changes the configuration of the bound environment: mode, light_pick and rotation freely (the weights do not depend on them); scale or grid rebuild the tables.
 *                     Both: GLRTX_EINVAL, everything unchanged, the offender named in the message, for a NULL context or configuration; a map that is not square
 *                     or smaller than 2 x 2; a wrap other than clamp; anything glrtx_upload_textures refuses of a descriptor; a mode other than 0 or 1; grid
 *                     outside 0 .. 1024; light_pick outside [0, 1] or NaN; a scale or rotation entry that is not finite, or a negative scale;
 *                     glrtx_set_environment_cfg with no environment bound.
 *   While an environment is bound these refuse with GLRTX_EINVAL and a message that says "an environment is bound": rendering with GLRTX_EXT_VOLUME set (the volume
 *                     branch has its own escape path), glrtx_render_adaptive*, glrtx_render_moments, glrtx_render_cascades and glrtx_hit_histogram (the
 *                     wavefront kernel's calls).  The present ring works as it does with spheres.  The feature pass is unchanged: a miss pixel keeps what it has.
 *   glrtx_debug_env_weights / _sample / _eval   the device statements on caller arrays on the current HIP device, no context.  weights_out: G * G floats,
 *                     *grid_out = G.  sample: out[8i..] = {direction, pdf, Le.rgb, 0} of the six uniforms u[6i..], with p_env = cfg.light_pick.  eval:
 *                     out[4i..] = {Le.rgb, pdf} of the direction dir[3i..].  They refuse what glrtx_upload_environment refuses.  Errors through glrtx_last_error(NULL).
 * NOT BUILT: seam-correct filtering, MIS between the two estimators, an environment beside the volume or under the wavefront kernel, the background in the
 *   feature planes and denoisers.  Groups: no call; a member is reached through glrtx_group_ctx(grp, i). */
enum glrtx_env_mode { GLRTX_ENV_ESCAPE = 0, GLRTX_ENV_SAMPLED = 1 };
typedef struct glrtx_env_cfg { int32_t mode; int32_t grid; float light_pick; float scale[3]; float rotation[9]; } glrtx_env_cfg;
int glrtx_upload_environment(glrtx_ctx *ctx, const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg);
int glrtx_set_environment_cfg(glrtx_ctx *ctx, const glrtx_env_cfg *cfg);
int glrtx_debug_env_weights(const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, float *weights_out, int32_t *grid_out);
int glrtx_debug_env_sample(const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, const float *u, size_t n, float *out);
int glrtx_debug_env_eval(const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, const float *dir, size_t n, float *out);

/* ---- Material maps: a tangent-space normal map on a diffuse or conductor material, a roughness map on a conductor (no reference counterpart; off unless
 * called: with no maps bound every launch runs the kernels it ran before).  The maps are textures of the set glrtx_upload_textures bound -- that set may bind no
 * albedo at all (all -1) --, looked up by "Textures"' rule at the hit's (s, t).  Shaded by MAPS instantiations of the extension megakernel's textured kernels
 * (pt_render_persistent's TEX and ENV forms), launched only while maps are bound.  PINNED through the reference all the same: a flat normal map and a
 * constant roughness map of the material's own alphas render the unmapped image bit for bit, and a roughness map that is constant over each cell renders the
 * image of one conductor material a cell.
 *
 * Arithmetic.  Every operation is one correctly rounded fp32 operation in the order written, unfused; denormals are zeros of their sign into and out of every
 * operation.  Dots are (x x' + y y') + z z'.  rsq(x) = 1 / sqrt(x), IEEE sqrt then IEEE reciprocal (surf_tri's).  Three statements agree bit for bit:
 * csrc/maps.hip.h, glrt_map_normal / glrt_map_alpha (include/glrt_host.h), tests/maps_math.py.
 *
 * INPUTS at a triangle hit.  n: the shading normal surf_tri returns.  e1 = v1 - v0, e2 = v2 - v0: the leaf record's words, in the wire's corner order, as the
 *   refit rewrote them after the last move -- a posed or updated mesh carries its frame along.  (s0, t0), (s1, t1), (s2, t2): the corners' coordinates, FROZEN
 *   when the set was uploaded.  c: the lookup of the bound map at the hit's (s, t).
 * DECODE.   m = c * 2 + -1 per channel, for every format.
 * FRAME.    ds1 = s1 - s0, ds2 = s2 - s0, dt1 = t1 - t0, dt2 = t2 - t0;  det = ds1 * dt2 - ds2 * dt1;
 *   Tr = e1 * dt2 - e2 * dt1,  Br = e2 * ds1 - e1 * ds2, per component; for det < 0 the sign bits of both are inverted.
 *   k = dot(n, Tr),  Tp = Tr - k * n,  l2 = dot(Tp, Tp),  T = Tp * rsq(l2);
 *   C = cross(n, T) = (ny Tz - nz Ty, nz Tx - nx Tz, nx Ty - ny Tx);  B = C, with its sign bits inverted iff dot(C, Br) < 0.
 *   TANGENTS ARE PER TRIANGLE AND ARE NOT INTERPOLATED: the wire's tangent / binormal words are not read.
 * PERTURBATION.  a = m.x * scale, b = m.y * scale;  p = (a * T + b * B) + m.z * n per component;  q = dot(p, p);  n' = p * rsq(q).
 * KEPT.     n is kept, word for word, when det is zero or not finite; when l2 or q is not a finite positive number; when a and b are both zero (either
 *   sign).  The last rule is part of the contract: an RGBA32F map of (0.5, 0.5, 1.0) renders the unmapped image bit for bit.
 * WHERE.    n' stands wherever the reference reads the shading normal: the local frame, woz, the spawn offset, the cosine of the light sample, the
 *   environment branch.
 * ROUGHNESS.  On a conductor (type 3) bound to a roughness map: ax = c.r > GLRTX_MAP_ALPHA_MIN ? c.r : GLRTX_MAP_ALPHA_MIN, ay likewise from c.g (a NaN gives
 *   the floor).  They REPLACE alpha.x / alpha.y at the three places the shading reads them: the BSDF sample, the triangle-light evaluation and the
 *   environment-light evaluation.  Channel b and alpha are not read.
 * Analytic spheres have no coordinates and shade unmapped, as with albedo.
 *
 *   glrtx_bind_material_maps  binds record m to material m: texture indices of the bound set (-1: none) and the normal map's scale.  maps == NULL or
 *                     n_mat == 0 unbinds.  glrtx_upload_textures and glrtx_upload_scene DROP the maps: a new set invalidates the indices.
 *                     GLRTX_EINVAL, everything unchanged, the offender named in the message: no texture set is bound; n_mat other than the scene's material
 *                     count; an index outside -1 .. n_tex - 1; a normal map on a material that is neither diffuse nor conductor; a roughness map on a
 *                     material that is not a conductor; a map whose texture has format GLRTX_TEX_RGBA8_SRGB; a scale that is not finite; reserved non-zero.
 *   The wavefront kernel's calls keep refusing with "textures are bound".  glrtx_upload_textures' own refusals are unchanged, the conductor binding included:
 *                     that is why this is a second call.  (With glrtx_set_texture_wavefront -- "Textures" -- launches with maps bound run on the wavefront
 *                     kernel's TM form, bit for bit the MAPS kernels' images and ray counts, and those calls work.)
 *   Feature pass      with maps bound, plane N of glrtx_render_features carries n' of the primary hit, so the denoisers' normal edge-stop and the
 *                     reprojections' normal test see the detail the image shows.  Albedo, material id, distance and plane G are unchanged.
 *   glrtx_debug_map_normal  the rule on caller arrays on the current HIP device, no context: record i is GLRTX_MAP_RECORD_FLOATS floats {n, e1, e2, (s0, t0),
 *                     (s1, t1), (s2, t2), m} with m the DECODED texel; normal_out[3i..] = n'.  Errors through glrtx_last_error(NULL).
 * NOT BUILT: emission maps (next-event estimation samples light triangles from a table that carries no coordinates), interpolated per-vertex tangents, maps
 *   on spheres and on the dielectric, mip levels, height / parallax maps.  Groups: no call; a member is reached through glrtx_group_ctx(grp, i). */
#define GLRTX_MAP_ALPHA_MIN 1e-3f
#define GLRTX_MAP_RECORD_FLOATS 18
typedef struct glrtx_material_map { int32_t normal, roughness; float normal_scale; int32_t reserved; } glrtx_material_map; /* 16 bytes; -1: none; reserved 0 */
int glrtx_bind_material_maps(glrtx_ctx *ctx, const glrtx_material_map *maps, size_t n_mat);
int glrtx_debug_map_normal(const float *records, size_t n, float scale, float *normal_out);

/* ---- Cutouts: an alpha test on triangle hits, decided INSIDE the closest-hit search (no reference counterpart; off unless called: with no cutouts bound
 * every launch runs the kernels it ran before).  Leaves, fences, grates and decals are a few quads whose shape lives in one channel of a texture: a material
 * may be bound to a cutout record {texture, channel, cutoff}, and a candidate hit on such a material counts only where the texture says so.  The decision
 * cannot be made above the ABI: it is taken per candidate, before the candidate updates the ray's record, in CUT instantiations of the traversal step
 * (csrc/pt_kernel.hip.h: trav_step<.., CUT>), launched only while cutouts are bound.  PINNED through the reference all the same: a rejected candidate
 * leaves the traversal exactly as if that piece of surface did not exist, so a cutout texture that is constant over each triangle renders, bit for bit and
 * ray for ray, the image of the same tree with the rejected triangles collapsed to a point.
 *
 * Arithmetic.  As "Textures".  Three statements agree bit for bit: tex_lookup_channel / cut_accepts (csrc/texture.hip.h), glrt_texture_channel
 * (include/glrt_host.h), tests/cutout_math.py.
 *
 * RECORD.   texture: an index into the bound set, or -1 (the material is not cut).  channel: 0 .. 3.  cutoff: a finite float.  reserved: 0.
 * VALUE.    At a triangle candidate hit (tri, u, v) on a bound material, (s, t) is "Textures"' AT A HIT expression.  The value is the chosen channel of
 *   the "Textures" lookup at (s, t): channels 0 .. 2 are what the lookup returns, sRGB decode included; channel 3 is the texel's fourth float for
 *   GLRTX_TEX_RGBA32F and (float)byte / 255.0f for BOTH 8-bit formats (alpha is never sRGB-decoded), filtered by the same FILTER expression, wrap and filter
 *   as the other channels.
 * TEST.     The candidate is accepted iff value >= cutoff.  A NaN value rejects.
 * WHERE.    The candidate is one that passed the triangle test and lies closer than the ray's closest hit so far.  A rejected candidate changes nothing in
 *   the ray's state: not t, tri, u, v, nor a shadow ray's stop test -- the search goes on as after a miss.  The rule applies to every ray of a launch: path
 *   rays, shadow rays to triangle lights (with or without the shadow range limit) and shadow rays to the environment.
 * Analytic spheres have no coordinates and are never cut.  Only diffuse (type 2) and conductor (type 3) materials may be bound: an emitter may not, because
 *   the light table that next-event estimation samples carries no coordinates.
 *
 *   glrtx_bind_cutouts  binds record m to material m.  cut == NULL or n_mat == 0 unbinds.  Needs a bound texture set, which may bind no albedo at all.
 *                     glrtx_upload_textures and glrtx_upload_scene DROP the records.  They survive glrtx_update_vertices*, glrtx_pose* and
 *                     glrtx_update_positions*: topology and the frozen coordinate table do not change.  A per-triangle table (the record index, or -1) is
 *                     built in this call from the triangles' materials: the traversal pays one 4-byte gather for every would-be-closest candidate, and
 *                     only a cut triangle goes on to its coordinates and the texels.  Seals an open fed launch.
 *                     GLRTX_EINVAL, everything unchanged, the offender named in the message: no texture set is bound; n_mat other than the scene's material
 *                     count; an index outside -1 .. n_tex - 1; a channel outside 0 .. 3; a cutoff that is not finite; a bound material that is neither
 *                     diffuse nor conductor; reserved non-zero; a vine tree (the list scan has no cutout form).
 *   ROUTING.          While cutouts are bound, launches run on the persistent megakernel (variant_last 1, GLRTX_FALLBACK_EXTENSIONS), in the CUT forms of its
 *                     textured kernels; glrtx_set_texture_wavefront does not take them.  glrtx_render_adaptive*, glrtx_render_moments,
 *                     glrtx_render_cascades and glrtx_hit_histogram refuse with "textures are bound" and the reason "cutouts are bound".  Rendering with
 *                     GLRTX_EXT_VOLUME set and a volume uploaded refuses with "cutouts are bound".  After unbinding everything routes as before, and images
 *                     are bit for bit what they were.
 *   Feature pass      with cutouts bound, the textured feature kernels walk with the same CUT step (both node layouts), so planes N, A and G of
 *                     glrtx_render_features describe the surface the image shows: the denoisers' edge stops and both reprojections follow the holes.
 *                     glrt_render_features_geom_cutout (include/glrt_host.h) states it.  Without cutouts bound the pass runs the kernels it ran before.
 *   glrtx_debug_texture_channel  tex_lookup_channel on caller arrays on the current HIP device, no context: value_out[i] = channel channel[i] of
 *                     lookup(which[i], st[2i], st[2i + 1]).  Refuses what glrtx_debug_texture_lookup refuses, and a channel outside 0 .. 3.
 * NOT BUILT: stochastic or blended transparency (this is an alpha test only); cutouts in glrtx_trace_rays (queries stay geometric); cutouts on the wavefront
 *   kernel, whose traversal step is hand-written assembly; cutouts on spheres, emitters, the dielectric, beside the volume, or on a vine tree; alpha read
 *   from image files (the facade's readers are three-channel: its "cutout" block names r, g or b); mip levels.  Groups: no call; a member is reached through
 *   glrtx_group_ctx(grp, i). */
typedef struct glrtx_cutout { int32_t texture, channel; float cutoff; int32_t reserved; } glrtx_cutout; /* 16 bytes; texture -1: none */
int glrtx_bind_cutouts(glrtx_ctx *ctx, const glrtx_cutout *cut, size_t n_mat);   /* NULL or 0 unbinds */
int glrtx_debug_texture_channel(const glrtx_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes,
                                const int32_t *which, const int32_t *channel, const float *st, size_t n, float *value_out);
/* The name of the render kernel the context's last launch ran, as error reports give it -- "pt_render_persistent (extensions, textures, cutouts)",
 * "pt_render_wgwf (textures)", ... --, "" before the first launch or for a NULL context.  Diagnostic: the tests name the launched form with it.  The string
 * is static. */
const char *glrtx_debug_last_kernel(const glrtx_ctx *ctx);

/* ---- Emission maps: a texture on the emitter, seen directly AND sampled as a light (no reference counterpart; off unless called: with no emission maps
 * bound every launch runs the kernels it ran before).  A screen, a sign, a stained-glass panel or a light card is one quad whose picture lives in a texture.
 * This section SUPERSEDES the two remarks above that say emission maps are not built ("Material maps": NOT BUILT; "Cutouts": "an emitter may not"): the light
 * table still carries no coordinates, and does not need to -- a light's wire record names three vertices, those vertices carry uv, and the binding call
 * builds a per-light coordinate table from them on the host.  An emitter still cannot be CUT.  PINNED through the reference: an emission map that is constant
 * over each triangle renders, bit for bit and ray for ray, the image of the same triangles with one emitter material each.
 *
 * Arithmetic.  As "Textures".  Three statements of the sampled-side rule agree bit for bit: emit_light_st / emit_radiance (csrc/texture.hip.h, used by
 * shade_core<.., EMIT> in csrc/pt_kernel.hip.h), glrt_light_emission (include/glrt_host.h), tests/emission_math.py.
 *
 * RADIANCE. Le = emission * c, per channel: c is the "Textures" lookup (sRGB decode included), emission is m0.xyz of the material, and the product is ONE
 *   rounded fp32 product, formed before anything else uses it.  The texture multiplies the emission; it does not replace it, unlike albedo: an 8-bit texel
 *   lies in [0, 1] and the material carries the intensity.
 * SEEN.     The renderer adds beta * emission at a triangle hit in two places: the general branch (depth 0, or behind a specular bounce) and the dielectric
 *   branch.  On a bound material both add beta * Le, c looked up at "Textures"' AT A HIT coordinates, and only where one of those conditions holds.  Both
 *   faces emit, as in the reference.
 * SAMPLED.  In next-event estimation's triangle-light branch the sample (ua, ub) -- after the flip at ua0 + ub0 > 1 -- of light lid has
 *   w0 = (1 - ua) - ub, s = (w0 * s0 + ua * s1) + ub * s2, t likewise, with (s0, t0) .. (s2, t2) the uv words of the light's three vertices in wire order
 *   (the per-light table light_st, read from global memory).  Where the light's material is bound, Le stands for the emission in the three contribution
 *   lines.  The lookup happens only for a sample that contributes (both cosines positive).  The random stream, the shadow ray and the ray counts do not
 *   change; the light pick stays uniform; the environment branch is untouched.
 * Analytic spheres have no coordinates and emit their plain emission.
 *
 *   glrtx_bind_emission_maps  binds material m to texture material_emission[m] of the bound set, -1: none.  NULL or n_mat == 0 unbinds.  Needs a bound
 *                     texture set, which may bind no albedo at all.  A material of any type except media (type 5) may be bound.  glrtx_upload_textures and
 *                     glrtx_upload_scene DROP the bindings.  They survive glrtx_update_vertices*, glrtx_pose* and glrtx_update_positions*: light_st is built
 *                     in this call from the vertices glrtx_upload_scene was given, and frozen, as "Textures" freezes its table.  Seals an open fed launch.
 *                     GLRTX_EINVAL, everything unchanged, the offender named in the message: a NULL context; no scene, or no texture set; n_mat other than
 *                     the scene's material count; an index outside -1 .. n_tex - 1; a bound material of type 5; cutouts are bound (the two do not combine
 *                     yet: glrtx_bind_cutouts likewise refuses while emission maps are bound).
 *   ROUTING.          While emission maps are bound, launches run on the persistent megakernel (variant_last 1, GLRTX_FALLBACK_EXTENSIONS), in the EMIT forms
 *                     of its textured kernels ("pt_render_persistent (.., emission maps)"); glrtx_set_texture_wavefront does not take them.
 *                     glrtx_render_adaptive*, glrtx_render_moments, glrtx_render_cascades and glrtx_hit_histogram refuse with "textures are bound" and the
 *                     reason "emission maps are bound".  Rendering with GLRTX_EXT_VOLUME set and a volume uploaded refuses with "emission maps are bound".
 *                     After unbinding everything routes as before, and images are bit for bit what they were.
 *   Feature pass      with emission maps bound, at a primary hit on a bound material whose type is not diffuse plane A's rgb carries c -- the looked-up
 *                     texel, without the emission -- where it holds zeros otherwise, so that the denoisers divide the emitter's picture out before they
 *                     filter and multiply it back afterwards.  A bound diffuse material keeps its albedo rule.  glrt_emission_albedo (include/glrt_host.h)
 *                     states it on plane G.  Without emission maps bound the pass runs the kernels it ran before.
 *   glrtx_debug_light_emission  the device statement of SAMPLED on the context's bound scene: out[5i ..] = {s, t, Le.rgb} of light lid[i] at the RAW uniforms
 *                     (u[2i], u[2i + 1]), the flip included; a light whose material is not bound gives its plain emission.  Refuses a context without
 *                     emission maps bound and a light index out of range.
 * NOT BUILT: picking lights by power (the pick stays uniform); emission maps on the wavefront kernel, beside the volume or beside cutouts; emission maps on
 *   spheres; MIS; mip levels; light_st staged into LDS beside the light records.  Groups: no call; a member is reached through glrtx_group_ctx(grp, i). */
int glrtx_bind_emission_maps(glrtx_ctx *ctx, const int32_t *material_emission, size_t n_mat);   /* NULL or 0 unbinds */
int glrtx_debug_light_emission(glrtx_ctx *ctx, const int32_t *lid, const float *u, size_t n, float *out);

/* ---- Groups: the same device layer on several GPUs of one node, behind one handle and one host thread.
 * No reference counterpart (the reference is single-GPU); SURVEY.md 8(b) sketches glrtx_create(ctx**, device_ids, n) with a
 * gathering read_accum -- this is that, kept apart from the single-context calls.  Member i owns the 8-row stripes s with
 * s % n == i (global pixel coordinates, resident accumulator rows, its own stream); rendering exchanges nothing; read_accum
 * and resolve_rgba8 first copy the stripes device-to-device into a full frame on member 0's GPU (one strided xGMI peer copy per member,
 * issued on the member's own stream so that the links work side by side), i.e. they
 * return the FULL image.  device_ids may name the same GPU more than once (partition emulation, used by the tests).
 * glrtx_group_ctx borrows a member for the per-context knobs (glrtx_set_variant, glrtx_count_rays, glrtx_get_stats);
 * do not resize, partition or destroy a member directly.  glrtx_group_get_stats sums rays / paths / rows and takes the
 * maximum of the kernel times (the members run concurrently). */
typedef struct glrtx_group glrtx_group;
int glrtx_group_create(glrtx_group **out, const int *device_ids, int n_devices);
void glrtx_group_destroy(glrtx_group *grp);
const char *glrtx_group_last_error(const glrtx_group *grp);
int glrtx_group_size(const glrtx_group *grp);
glrtx_ctx *glrtx_group_ctx(glrtx_group *grp, int i);
int glrtx_group_upload_scene(glrtx_group *grp, const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat,
                             size_t n_mat, const float *light, size_t n_light, const float *bvh, size_t n_nodes);
/* glrtx_update_vertices on every member. */
int glrtx_group_update_vertices(glrtx_group *grp, const float *vert, size_t n_vert);
/* glrtx_upload_volume on every member (the grids are replicated, like the scene). */
int glrtx_group_upload_volume(glrtx_group *grp, const float *density, const float *temperature, int nx, int ny, int nz, const float bbox_min[3],
                              const float bbox_max[3], float density_max);
int glrtx_group_resize(glrtx_group *grp, int width, int height);
int glrtx_group_clear(glrtx_group *grp);
int glrtx_group_render(glrtx_group *grp, const glrtx_params *params);
int glrtx_group_render_frames(glrtx_group *grp, const glrtx_params *params, const float *seeds_xy, int n_frames);
int glrtx_group_sync(glrtx_group *grp);
/* glrtx_render_adaptive on every member, each selecting on its own accumulator (refusals are checked on all members first); the active-tile
 * counts are summed over the members. */
int glrtx_group_render_adaptive(glrtx_group *grp, const glrtx_params *params, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg);
int glrtx_group_adaptive_active_tiles(glrtx_group *grp, int *active, int *total);
int glrtx_group_read_accum(glrtx_group *grp, float *dst_rgba, size_t dst_pitch_bytes);
int glrtx_group_resolve_rgba8(glrtx_group *grp, uint8_t *dst, size_t dst_pitch_bytes, float gamma, int flip_y);
int glrtx_group_get_stats(const glrtx_group *grp, glrtx_stats *out);
/* Device-to-device copies the last gather (read_accum / resolve_rgba8) issued: one strided copy per member, on the member's own
 * stream, plus one for a partial last stripe -- at most 2 x members (diagnostic; the tests pin it). */
int glrtx_group_gather_copies(const glrtx_group *grp);
/* Presentation of the FULL image (see glrtx_present_enable; window.cpp:157-164 on several GPUs).  The ring's pinned images are the group's; every member
 * resolves its own stripes into its own device images and lands them in place with one strided copy (an 8-row stripe is contiguous in the RGBA8 image; a
 * partial last stripe takes one more) on its own copy stream -- nothing is gathered on member 0.  The members' rings move in step: a group render call
 * returns GLRTX_EBUSY, before any member renders, when one of them has no free image.  glrtx_group_present_get_stats: member 0's counters, `copies_last`
 * summed over the members. */
int glrtx_group_present_enable(glrtx_group *grp, int ring_images, float gamma, int flip_y);
int glrtx_group_present_acquire(glrtx_group *grp, int wait, glrtx_image *out);
int glrtx_group_present_release(glrtx_group *grp, const glrtx_image *img);
int glrtx_group_present_get_stats(const glrtx_group *grp, glrtx_present_stats *out);

#ifdef __cplusplus
}
#endif
#endif
