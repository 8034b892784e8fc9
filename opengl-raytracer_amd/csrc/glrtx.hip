// glrtx.hip -- C-ABI host layer of libglrtx.so (include/glrtx.h): context, scene validation and
// repacking, accumulator management, kernel launch, timing.  This is the "thin C-ABI HIP host
// layer" that stands where GLFW/GL stood in the reference (src/core/window.cpp,
// src/core/texture_buffer.cpp, src/core/framebuffer_object.cpp).  gfx950 only.
#include "glrtx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <limits>
#include <string>
#include <vector>

#include "glrt_host.h"
#include "pt_kernel.hip.h"
#include "accumulate.hip.h"
#include "lbvh.hip.h"
#include "sahl.hip.h"
#include "refit.hip.h"
#include "skin.hip.h"
#include "normals.hip.h"
#include "query.hip.h"
#include "features.hip.h"
#include "denoise.hip.h"
#include "variance.hip.h"
#include "reproject.hip.h"
#include "reproject_motion.hip.h"
#include "tonemap.hip.h"
#include "bloom.hip.h"
#include "../host/reproject_setup.h"
#include "../host/morph_sparse.h"
#include "../host/normal_topology.h"
#include "../host/texture_set.h"
#include "../host/emission_statement.h"
#include "../host/route_statement.h"
#include "../host/env_tables.h"
static_assert(glrtx::lbvh::kRotationPasses == GLRT_LBVH_ROTATION_PASSES, "device and CPU LBVH statements must run the same rotation sweeps");
static_assert(glrtx::lbvh::kRebuildLeaves == GLRT_LBVH_REBUILD_LEAVES, "device and CPU LBVH statements must rebuild the same subtrees");

using namespace glrtx;

namespace {

constexpr int kStripeQuantum = 8;   // stripe heights are multiples of the 8x8 work tile
constexpr int kGroupStripe = 8;     // stripe height glrtx_group uses: 1080 rows over 8 members = 136 / 128 rows (16-row stripes: 144 / 128)
constexpr int kPairFetchMinRecords = 32768;  // forks + triangles (2 MiB of 64-byte records) from which the wavefront kernel fetches nodes pair-cooperatively
constexpr int kFramesBudgetGiB = 32;  // device memory one glrtx_render_frames launch may use for its sample planes (and the single-frame pipe slots for their buffers)
constexpr float kInf = std::numeric_limits<float>::infinity();
constexpr unsigned kPipeSlots = 8;    // most single-frame launches that may be in flight at once (each with its own stream, state, queues, planes); pipe_slots are used
constexpr unsigned kLaunchRing = 16;  // launches that may be outstanding per context before a new one waits for the oldest

thread_local std::string g_create_error;

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// An image plane a context owns beside its accumulator, and the shape of the image it was last written at: the accumulator's own (accum_shape: H, M, C) or packed rows
// of float4 (packed_shape: N / A / G, D, T, B).  Whoever writes a plane stamps it; a reader asks whether it is current; glrtx_resize and a tracking switched off drop it.
struct Shape {
    int width = 0;
    size_t pitch = 0;  // bytes from row to row
    int rows = -1;     // (-1: never stamped)
    bool operator==(const Shape &o) const { return width == o.width && pitch == o.pitch && rows == o.rows; }
};
struct Plane {
    DevBuf buf;
    Shape at;
    void stamp(const Shape &s) { at = s; }
    bool stamped() const { return at.rows >= 0; }
    bool current(const Shape &s) const { return buf.p && at == s; }
    void drop();
};

}  // namespace

struct glrtx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // Per launch: start, render kernel done, all done.  A RING of triples: a launch takes the next free one and never waits for an
    // earlier launch; finished launches are folded into the stats lazily (glrtx_sync, glrtx_get_stats, or -- without blocking -- at the
    // next launch).  Only with kLaunchRing launches outstanding does a new launch wait, for the oldest one.
    struct LaunchRec {
        hipEvent_t ev0 = nullptr, evm = nullptr, eva = nullptr, ev1 = nullptr;  // render start / end, accumulation start / end (eva recorded only by overlapped launches)
        bool has_eva = false;
        const char *kernel = "";
        int frames = 0;
    };
    LaunchRec ring[kLaunchRing];
    unsigned ring_head = 0, ring_tail = 0;  // launches [tail, head) are recorded and not yet folded
    hipEvent_t tm0 = nullptr, tm1 = nullptr;      // glrtx_timer_*
    hipEvent_t rs0 = nullptr, rs1 = nullptr;      // around the resolve kernel
    std::string err;

    DevBuf forks, cnodes, cranks, nrms, mats, lights, vine, accum_own, counter, rgba8, work;
    DevBuf spheres, sphereMat;  // extension kernel: analytic spheres
    int n_spheres = 0, ext_flags = 0;
    // Textures (glrtx_upload_textures; texture.hip.h), the scene's until the next glrtx_upload_scene: descriptors, the texel blob, the per-triangle coordinate
    // table and the per-material binding on the device; n_tex == 0: no set bound.  scene_st: the table's source -- six floats {s, t} x 3 a device triangle
    // (record 0 the never-hit one), taken from the vertices glrtx_upload_scene was given.
    DevBuf texDesc, texTexels, texSt, texBind;
    int n_tex = 0;
    std::vector<float> scene_st;
    // Material maps (glrtx_bind_material_maps; maps.hip.h), the set's until the next glrtx_upload_textures or glrtx_upload_scene: one MapRec a material on the
    // device; have_maps: the MAPS instantiations are launched.  tex_format: the bound set's formats (a map may not be sRGB).
    DevBuf texMaps;
    bool have_maps = false;
    std::vector<int> tex_format;
    // Cutouts (glrtx_bind_cutouts; texture.hip.h), the set's until the next glrtx_upload_textures or glrtx_upload_scene: one CutRec a material and tri_cut, the
    // record index of every device triangle (-1: not cut); have_cut: the CUT instantiations are launched, on the megakernel only.  scene_mat: the material of
    // every device triangle (record 0 the never-hit one), taken from the triangles glrtx_upload_scene was given -- tri_cut's source, as scene_st is tri_st's.
    DevBuf cutRec, cutTri;
    bool have_cut = false;
    std::vector<int32_t> scene_mat;
    // Emission maps (glrtx_bind_emission_maps; texture.hip.h: EmitSet), the set's until the next glrtx_upload_textures or glrtx_upload_scene: the texture index
    // of every material (-1: none) and light_st, three {s, t} a light; have_emit: the EMIT instantiations are launched, on the megakernel only.
    // scene_light_st: light_st's source -- words 6 and 7 of the light's three wire vertices, taken from the vertices glrtx_upload_scene was given.
    DevBuf emitMat, emitSt;
    bool have_emit = false;
    std::vector<float> scene_light_st;
    // Environment (glrtx_upload_environment; environment.hip.h), kept across glrtx_upload_scene: the map's texels, the importance grid's five tables, and what the
    // kernels take of it (env: its pointers are these buffers'; p_env is set at every launch).  env_cfg / env_desc: what it was made from.
    DevBuf envTexels, envRowQ, envRowAlias, envColQ, envColAlias, envCellP;
    EnvArgs env{};
    glrtx_env_cfg env_cfg{};
    bool have_env = false;
    DevBuf volDensity, volTemp;  // volume kernel (GLRTX_EXT_VOLUME): the two grids of glrtx_upload_volume
    VolArgs vol{};
    bool have_volume = false;
    bool vol_wavefront = false;  // glrtx_set_volume_wavefront: volume launches on the wavefront kernel's V form (GLRTX_VOLUME_WAVEFRONT=0/1 overrides it per launch)
    bool tex_wavefront = false;  // glrtx_set_texture_wavefront: textured launches on the wavefront kernel's T / TM forms (GLRTX_TEXTURE_WAVEFRONT=0/1 overrides it per launch)
    DevBuf wfState, wfQ;      // wavefront path state (kWfStatePlanes = 6 planes of float4 x ids) + per-workgroup queues (variant 2)
    DevBuf wfSeeds, wfPlanes;       // frames in flight: per-frame seeds, per-sample planes
    // Single-frame launches that overlap (launch_wgwf): pipe_slots (<= kPipeSlots) slots used in turn, each with its own stream, path state, queues, tile
    // counter and sample planes; the accumulator is only touched by the plane-accumulation pass, on the context's stream, in launch order.
    struct PipeSlot {
        hipStream_t stream = nullptr;
        hipEvent_t render_done = nullptr, acc_done = nullptr;
        bool used = false;
        DevBuf state, queues, planes, work;
        // fed launches (pt_kernel.hip.h: FeedHost / FeedDev): the host-coherent block the host publishes frames in, its device address, the launch's device mirror,
        // and the sample planes in chunks of kFeedChunkFrames frames, allocated as a burst grows and kept for the next one (chunk_bytes: what each was allocated with)
        FeedHost *feed_h = nullptr, *feed_h_dev = nullptr;
        DevBuf feed_d;
        DevBuf chunks[kFeedChunks];
        size_t chunk_bytes = 0;
    } pipe[kPipeSlots];
    // The launch that is still OPEN: a fed launch of this context that may still be running and that the next glrtx_render / glrtx_render_frames call with the same
    // camera appends its frames to (feed_append) instead of starting a launch of its own.  Every other entry point that orders something against the accumulator
    // or changes what a launch depends on SEALS it (seal_feed): nothing is appended any more, the launch finishes what it has.
    struct OpenFeed {
        PipeSlot *slot = nullptr;
        glrtx_params p{};       // the camera / sampling parameters the launch was started with (seed ignored)
        int frames = 0, cap = 0;  // frames published so far / the most this launch can take
        LaunchRec *rec = nullptr;
        size_t frame_bytes = 0;   // sample planes of one frame
        bool vol = false;         // the launch is the V form (kWgwfVolume)
    } open;
    bool feed_ok = true;            // cleared when the host-coherent blocks cannot be had; GLRTX_NO_FEED=1 (read at every launch, like the other switches) turns fed launches off (A/B, tests)
    bool last_was_render = false;   // the previous call on this context was glrtx_render / glrtx_render_frames (nothing has observed the accumulator since)
    glrtx_params last_p{};          // ... with these parameters
    hipEvent_t last_render_done = nullptr;  // ... and this is its render kernel's completion event (a slot's; not owned)
    unsigned pipe_next = 0;
    bool pipeline = true;           // GLRTX_NO_PIPELINE=1 switches it off (A/B)
    int pipe_share = 1;             // an overlapped launch issued while others still render takes 1 / pipe_share of the workgroup slots (GLRTX_PIPE_SHARE; 1: all)
    unsigned pipe_slots = 6;        // slots used in turn (GLRTX_PIPE_SLOTS, <= kPipeSlots)
    DevBuf bvhVert, bvhTri, bvhNodes;  // glrtx_build_lbvh staging
    lbvh::Workspace bvhWs;
    int variant = 2;          // 0 = tile megakernel, 1 = persistent megakernel with path regeneration, 2 = workgroup-local wavefront
    int n_cu = 256;
    DevScene sc{};
    bool have_scene = false;
    int n_tri = 0, n_fork = 0, n_mat = 0, n_light = 0;
    int budget_share = 1;     // contexts of one group on this device: each takes 1 / budget_share of the frames-in-flight memory budget

    int width = 0, height = 0;
    int rank = 0, world = 1, stripe = 16;
    int owned_rows = 0;
    float4 *accum = nullptr;  // own or bound
    size_t pitch_bytes = 0;
    bool bound = false;
    int bound_rows = 0;       // rows the caller's buffer holds (glrtx_bind_accum)

    // Four words of host-coherent memory the persistent kernel's trip guards report through ({code, workgroup, trips without a tile, live paths}; pt_render_wgwf):
    // read -- and cleared -- when a launch is folded.
    unsigned *guard_host = nullptr, *guard_dev = nullptr;
    hipEvent_t state_done = nullptr;  // the last render kernel that used wfState (plain launches on the context's stream, fed launches on their slot's) has ended
    bool state_used = false;

    std::vector<int> leaf_tri;  // leaf record k of the uploaded scene -> wire triangle (glrtx_hit_histogram)
    // Ray queries (glrtx_trace_rays, query.hip.h): leaf id -> wire triangle on the device (id 0: -1), uploaded with the scene; the ray counter; the
    // staging buffers of the host call
    DevBuf qwire, qcounter, qrays, qhits;
    // The refit plan (glrtx_update_vertices; refit.hip.h), kept beside the scene from its upload: the integer tables (`ints`), the wire boxes as keys with the
    // arrival counters and the read-back words (`keys`), a staging buffer for host vertices; `a`: the kernels' arguments with every pointer set
    struct Refit {
        DevBuf ints, keys, vert;
        refit::Args a{};
        size_t n_vert = 0;
        size_t bytes[5] = {0, 0, 0, 0, 0};  // the scene buffers' sizes as uploaded: nodes, cnodes, nrms, lights, vine (glrtx_debug_read_scene)
        hipEvent_t slot_ev = nullptr;      // recorded on each pipe slot's stream: the refit starts behind every launch that may still read the scene
    } rf;
    // The rig (glrtx_upload_rig; skin.hip.h), the scene's until the next glrtx_upload_scene: the rest pose, the {bones, weights} records and the pose matrices of
    // the last glrtx_pose.  n_bones == 0: no rig.
    // Deforming (glrtx_upload_morph_targets, glrtx_pose_morph, glrtx_pose_dualquat): the rig's morph targets as uploaded (n_targets x n_vert x 24 bytes; n_targets
    // == 0: none) and the dual quaternions of the last glrtx_pose_dualquat.
    // A rig holds a dense set (morph) or a sparse one (glrtx_upload_morph_targets_sparse: the inverted index srow / sent of nnz entries, and the weight table
    // swt of the last pose, whose host copy is wtab), never both.
    // One pose launch (pose_launch): which kernel of skin.hip.h, its mode (0: matrices, 1: dual quaternions; the skinning kernel has mode 0 only) and that kernel's
    // arguments.  The three argument structs begin alike -- rest, rig, pose, out, n_vert -- so n_vert is read through any of them; the constructor sets those
    // five and leaves the deform kernels' own (the targets) zero: no active target, no entry.
    struct PoseLaunch {
        enum Kernel { kNone, kSkin, kDeform, kSparse } kernel = kNone;
        int mode = 0;
        union {
            skin::Args skin;
            skin::DeformArgs deform{};
            skin::SparseArgs sparse;
        };
        PoseLaunch() = default;
        PoseLaunch(Kernel k, int m, const void *rest, const void *rig, const void *pose, void *out, size_t n_vert) : kernel(k), mode(m) {
            const skin::Args a{(const unsigned *)rest, (const uint4 *)rig, (const float4 *)pose, (unsigned *)out, n_vert};
            if (k == kSkin) skin = a;
            else if (k == kDeform) deform = skin::DeformArgs{a.rest, a.rig, a.pose, a.out, a.n_vert, nullptr, {}};
            else sparse = skin::SparseArgs{a.rest, a.rig, a.pose, a.out, a.n_vert, nullptr, nullptr, nullptr, 0};
        }
    };
    // last: the launch of the last glrtx_pose_morph / glrtx_pose_dualquat, for glrtx_debug_deform_burst (kNone: none since the rig or its targets were
    // uploaded; a glrtx_pose leaves it as it is).
    struct Rig {
        DevBuf rest, rig, pose, dq, morph, srow, sent, swt;
        int n_bones = 0, n_targets = 0;
        bool sparse = false;
        size_t nnz = 0;
        PoseLaunch last;
        std::vector<float> wtab;
    } sk;
    // Rebuilding normals (glrtx_upload_normal_topology; normals.hip.h), the scene's until the next glrtx_upload_scene: the topology's own copy of the rest
    // vertices, the index (tri, cls, row, face), the two scratch arrays of a rebuild (fvec, cnrm) and a staging buffer for host positions.  have: a topology is
    // uploaded; pose_on: glrtx_set_pose_normals.  `a`: the kernels' arguments but for the vertex buffer, which a call sets.
    struct Normals {
        DevBuf rest, tri, cls, row, face, fvec, cnrm, pos;
        bool have = false, pose_on = false;
        normals::Args a{};
    } nm;

    // Presentation (glrtx_present_enable): frame seq of the ring goes to image seq % ring -- device image (written by the presenting pass on the context's stream),
    // then pinned host image (copied on `copy`, behind pass_done, ending with the image's event).  An image is taken for a frame only while it is FREE: released by the
    // caller, whose acquire waited for the copy -- so neither side of an image is rewritten while anything still reads it.
    struct Present {
        int ring = 0;  // 0: off
        float inv_gamma = 1.0f;
        int flip = 1;
        bool full = false;  // a group member: lands its stripes in place in the group's full image (the group owns the host images)
        hipStream_t copy = nullptr;
        hipEvent_t pass_done = nullptr, t0 = nullptr, t1 = nullptr;
        bool timed = false;
        DevBuf dev;            // ring x (width x owned_rows) RGBA8
        struct Image {
            enum { FREE, PENDING, HELD } state = FREE;
            hipEvent_t ev = nullptr;
            uint8_t *host = nullptr;
            size_t host_bytes = 0;
            uint64_t frame = 0;
            int width = 0, rows = 0;
        };
        std::vector<Image> img;
        uint64_t seq = 0, acq = 0;  // frames given an image so far / acquired so far (acq <= seq: images [acq, seq) are pending)
        uint64_t frame = 0;         // frames accumulated since the last clear / resize
        int copies_last = 0;
        glrtx_present_stats st{};
    } pres;

    // Adaptive sampling (glrtx_render_adaptive): the half buffer H (every second sample; of the accumulator's shape, allocated on first use), and what the
    // last selection wrote -- a mask byte per tile, the ascending list of active tiles, their count in a device word -- for ad_tiles tiles.
    Plane adHalf;
    DevBuf adMask, adList, adCount;
    int ad_tiles = 0, ad_tiles_x = 0;  // (the tile grid of the last selection)
    bool ad_selected = false;

    // Denoising (glrtx_render_features / glrtx_denoise): the two feature planes, the filter's two ping-pong images and its result D, all packed rows of float4 --
    // ftN's stamp is the shape of the owned rows when the features were rendered (A and G share it); allocated on first use, released by glrtx_resize (and so by a
    // partition change).  D is stamped where it is written (glrtx_denoise, glrtx_denoise_variance, glrtx_reweight -- which needs no feature planes).
    Plane ftN, dnD;
    DevBuf ftA, ftCounter, dnP[2];
    // Reprojection (glrtx_reproject): the camera of the last glrtx_render_features (c2w[16], s2c[16]: the one the accumulator and the planes belong to), the spare
    // pair of feature planes and the spare accumulator (own pitch x owned rows) that the next call swaps in, and its two counters; allocated on first use,
    // released by glrtx_resize
    float ft_cam[32] = {};
    DevBuf ftN_spare, ftA_spare, accum_spare, rpCount;
    bool rp_have = false;         // rpCount holds a call's counts
    // Motion tracking (glrtx_track_motion): the third feature plane G and its spare (shape and release rules of N and A), and the PREVIOUS geometry per wire
    // triangle (motion::Args::prev_pos / prev_nrm: 3 float4 each) -- the scene as it stood at the last feature pass.  mt_geom: kMtNone, nothing is known (no
    // feature pass since tracking was switched on or a scene was uploaded); kMtCurrent, nothing moved since that pass: the scene's own records are the previous
    // geometry, and the next glrtx_update_vertices copies them out first; kMtSaved, that copy is what mtPos / mtNrm hold.
    enum { kMtNone, kMtCurrent, kMtSaved };
    bool mt_on = false, mt_g_have = false;  // mt_g_have: ftG holds the plane of the last feature pass
    int mt_geom = kMtNone;
    DevBuf ftG, ftG_spare, mtPos, mtNrm;

    // Variance guidance (glrtx_track_moments / glrtx_render_moments / glrtx_denoise_variance): the moments plane M {sum l, sum l^2, 0, count} at the accumulator's
    // shape (allocated on first use while tracking is on, zeroed with the accumulator, released by glrtx_resize and by switching tracking off),
    // and the filter's three variance planes (V0 and the ping-pong pair: packed floats of the features' shape, released with them).
    Plane mmM;
    DevBuf mmM_spare, dnV[3];  // (mmM_spare: the second M the reprojections write, of M's shape, swapped as accum_spare is)
    bool mm_on = false;

    // Firefly re-weighting (glrtx_track_cascades / glrtx_render_cascades / glrtx_reweight): the six cascade planes C_0 .. C_5 back to back, each of the accumulator's
    // shape (allocated on first use while tracking is on, zeroed with the accumulator and by the reprojections, released by glrtx_resize and by
    // switching tracking off), and the bounds' start.
    Plane rwC;
    bool rw_on = false;
    float rw_start = 1.0f;

    // Tone mapping (glrtx_exposure_measure / glrtx_tonemap): the exposure block (tonemap::Exposure: the working histogram, then glrtx_exposure's image; allocated and
    // zeroed on first use, kept across glrtx_resize) and the plane T (packed rows of float4; released by glrtx_resize)
    DevBuf tmExp;
    Plane tmT;

    // Bloom (glrtx_bloom): the plane B (packed rows of float4) and the pyramid D_1 .. D_8 behind it; both released by glrtx_resize
    Plane blB;
    DevBuf blPyr;

    bool count_rays = false;
    const char *last_kernel = "";  // name of the last render kernel launched (error reports)
    mutable bool counters_stale = false;          // a counting launch was issued since the device counters were last read
    mutable unsigned long long counters_host[2] = {0, 0};
    glrtx_stats st{};
};

namespace {

int fail(glrtx_ctx *c, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define HIP_TRY(c, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail(c, GLRTX_EDEVICE, "%s failed: %s", #call, hipGetErrorString(e_));     \
    } while (0)

int dev_upload(glrtx_ctx *c, DevBuf &b, const void *src, size_t bytes) {
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    const size_t alloc = std::max<size_t>(bytes, 64);
    HIP_TRY(c, hipMalloc(&b.p, alloc));
    b.bytes = alloc;
    if (bytes) HIP_TRY(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return GLRTX_OK;
}

void dev_free(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.bytes = 0;
}

void Plane::drop() { dev_free(buf); at = Shape{}; }

// The normal topology and the pose switch are forgotten (the stream is idle, as for morph_drop)
void normals_drop(glrtx_ctx *c) {
    for (DevBuf *b : {&c->nm.rest, &c->nm.tri, &c->nm.cls, &c->nm.row, &c->nm.face, &c->nm.fvec, &c->nm.cnrm, &c->nm.pos}) dev_free(*b);
    c->nm.have = c->nm.pose_on = false;
    c->nm.a = normals::Args{};
}

// The rig's morph targets, dense or sparse, are forgotten (the stream is idle: every caller has synchronised it or runs behind a blocking call)
void morph_drop(glrtx_ctx *c) {
    dev_free(c->sk.morph); dev_free(c->sk.srow); dev_free(c->sk.sent);
    c->sk.n_targets = 0;
    c->sk.sparse = false;
    c->sk.nnz = 0;
    c->sk.last = glrtx_ctx::PoseLaunch{};
}

Shape accum_shape(const glrtx_ctx *c) { return {c->width, c->pitch_bytes, c->owned_rows}; }
Shape packed_shape(const glrtx_ctx *c) { return {c->width, (size_t)c->width * sizeof(float4), c->owned_rows}; }

// diagnostic builds only: read and clear a device symbol (the traversal statistics, the step timing, the phase clocks)
template <class Sym>
int take_symbol(const Sym &sym, void *out) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(sym), sizeof(Sym)) != hipSuccess) return GLRTX_EDEVICE;
    static const Sym zero{};
    if (hipMemcpyToSymbol(HIP_SYMBOL(sym), &zero, sizeof(Sym)) != hipSuccess) return GLRTX_EDEVICE;
    return GLRTX_OK;
}

int owned_rows_of(int height, int rank, int world, int stripe) {
    int rows = 0;
    const int n_stripes = (height + stripe - 1) / stripe;
    for (int s = rank; s < n_stripes; s += world) rows += std::min(stripe, height - s * stripe);
    return rows;
}

inline float as_float(int v) { float f; std::memcpy(&f, &v, 4); return f; }

// Fold finished launches' event triples into the stats, oldest first.  block = false: only those whose events have already
// completed (hipEventQuery; nothing on the launch path ever waits for the device); block = true: all of them (the caller has
// synchronised the stream, or wants to).  A fault inside a kernel surfaces here, not at the launch call: say which launch it was.
int fold_launches(glrtx_ctx *c, bool block, unsigned keep = 0) {
    while (c->ring_head - c->ring_tail > keep) {
        glrtx_ctx::LaunchRec &r = c->ring[c->ring_tail % kLaunchRing];
        hipError_t e = block ? hipEventSynchronize(r.ev1) : hipEventQuery(r.ev1);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); return GLRTX_OK; }
        // a polling caller (glrtx_get_stats) must not swallow a device error: the record stays in the ring, and the next blocking fold -- glrtx_sync,
        // or a launch that needs the slot -- reports it with the launch it belongs to
        // -- but the poller is TOLD: glrtx_stats.device_error_pending stays set until that blocking fold has consumed the record
        const bool guard = e == hipSuccess && c->guard_host && __atomic_load_n(&c->guard_host[0], __ATOMIC_ACQUIRE) != 0u;  // (a trip guard's report: below)
        if ((e != hipSuccess || guard) && !block) { (void)hipGetLastError(); c->st.device_error_pending = 1; return GLRTX_OK; }
        c->ring_tail++;
        if (e != hipSuccess || guard) c->st.device_error_pending = 0;
        if (e != hipSuccess)
            return fail(c, GLRTX_EDEVICE, "render launch failed on the device (%s): %s, %dx%d (%d owned rows), %d frame(s), device %d", hipGetErrorString(e),
                        r.kernel, c->width, c->height, c->owned_rows, r.frames, c->device);
        if (guard) {  // a trip guard of the persistent kernel fired (pt_render_wgwf): the launch left paths unfinished
            const unsigned code = c->guard_host[0], wg = c->guard_host[1], trips = c->guard_host[2], alive = c->guard_host[3];
            std::memset(c->guard_host, 0, 16);
            return fail(c, GLRTX_EDEVICE, "render launch aborted by a trip guard (%s): workgroup %u, %u trips since its last tile, %u paths alive; %s, %dx%d (%d owned rows), %d frame(s), device %d",
                        code == 1u ? "two trips in which no ray was dealt and no path moved" : (code == 3u ? "a fed launch could neither claim a tile nor close its feed" : "trip limit exceeded"), wg, trips, alive, r.kernel, c->width, c->height,
                        c->owned_rows, r.frames, c->device);
        }
        float ms = 0.f, ms2 = 0.f;
        HIP_TRY(c, hipEventElapsedTime(&ms, r.ev0, r.evm));   // render kernel
        HIP_TRY(c, hipEventElapsedTime(&ms2, r.has_eva ? r.eva : r.evm, r.ev1));  // plane accumulation (frames in flight, overlapped single frames), else ~0
        c->st.kernel_ms_last = ms;
        c->st.kernel_ms_total += ms;
        c->st.accumulate_ms_total += ms2;
        c->st.kernel_launches++;
    }
    return GLRTX_OK;
}

// The event triple of the launch being issued.  Never blocks unless kLaunchRing launches are outstanding.
int next_launch_rec(glrtx_ctx *c, glrtx_ctx::LaunchRec *&out) {
    if (int rc = fold_launches(c, false)) return rc;
    if (c->ring_head - c->ring_tail >= kLaunchRing)
        if (int rc = fold_launches(c, true, kLaunchRing - 1)) return rc;
    out = &c->ring[c->ring_head % kLaunchRing];
    return GLRTX_OK;
}

int lds_bytes_for(const DevScene &sc) {
    return sc.lds_head_f4 * (int)sizeof(float4) + 2 * sc.stack_entries * kBlockThreads * (int)sizeof(int);  // materials and lights | traversal stacks
}

int pfail(glrtx_ctx *c, std::string *err_out, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err_out) *err_out = buf;
    else if (c) c->err = buf;
    else g_create_error = buf;
    return code;
}

// Validation + repacking of the wire-format scene; pure host code (no HIP calls), so it can be
// exercised without a GPU through glrtx_check_scene.
struct Packed {
    std::vector<float4> forks, tris, nrms, mats, lights, vine;
    int vine_uniform = 0;
    int n_vine = 0, vine_main = 0;  // records of the list (= triangles), index of the last one (the list is padded: see pack_scene)
    float4 root_lo = make_float4(0.f, 0.f, 0.f, 0.f), root_hi = make_float4(0.f, 0.f, 0.f, 0.f);
    int root_ref = REF_ABSENT;
    int root_boxed = 0;   // the wire root is a fork: its own box (root_lo / root_hi) is tested before anything else
    int stack_need = 0;
    std::vector<int> leaf_tri;  // leaf record k (id k + 1) -> wire triangle
    // The compact node array (pack_compact): 48-byte records at breadth-first positions, and the rank table that locates a fork's children
    std::vector<float4> cnodes;  // 3 float4 per position
    std::vector<uint2> cranks;   // per 32 positions {fork bits, forks in front of the group}
    // What the refit (glrtx_update_vertices, refit.hip.h) needs beside the buffers: leaf record k -> its wire node; fork record r -> the wire forks whose boxes
    // fill its left / right slot (-1: a leaf child or none); compact position -> its ref in the 64-byte layout; the vine's forks and leaves in list order
    std::vector<int> leaf_wire, cpos_ref, vine_fork, vine_leaf;
    std::vector<int2> fork_slot;
    bool tree = false;  // a tree was packed (root_ref was not REF_ABSENT)
};

// The compact node array, beside the 64-byte one.  Positions are numbered breadth-first from the root fork (position 0); the
// children of the fork of rank k -- k forks lie at smaller positions -- sit at positions 2k + 1 (left slot) and 2k + 2 (right slot), so a fork
// record needs no child refs and is exactly its children's twelve box floats: three dwordx4 loads instead of four loads of 56 bytes.
//   fork: {minL, maxR.x} {maxL, maxR.y} {minR, maxR.z}   (the step's registers: trav_asm.hip.h, GLRTX_TRAV_STEP_ASM_COMPACT)
//   leaf: {v0, id} {v1 - v0, next} {v2 - v0, 0}          (id: the triangle id a hit carries; next: the position of the leaf chained behind it, or REF_FIN)
// The same tree, boxes, triangle data and visiting order as the 64-byte array: a position holds the record the 64-byte ref held -- a fork, a leaf (the
// first leaf of a chained leaf pair: the second one lives in a tail region behind the tree) or the never-hit record of an absent child.
void pack_compact(Packed &P) {
    P.cnodes.clear();
    P.cranks.clear();
    std::vector<int> ref;  // position -> ref in the 64-byte layout
    ref.push_back(P.root_ref);
    for (size_t q = 0; q < ref.size(); q++) {  // (P.cpos_ref keeps the list for the refit)
        const int r = ref[q];
        if (r < 0) continue;
        int l, rr;
        std::memcpy(&l, &P.forks[4 * (size_t)r + 0].w, 4);
        std::memcpy(&rr, &P.forks[4 * (size_t)r + 1].w, 4);
        ref.push_back(l);   // 2k + 1
        ref.push_back(rr);  // 2k + 2
    }
    const size_t n_main = ref.size();
    std::vector<int> next_pos(n_main, REF_FIN);
    for (size_t q = 0; q < ref.size(); q++) {  // chained leaves: the tail (the loop runs on over the entries it appends)
        if (ref[q] >= 0) continue;
        int nx;
        std::memcpy(&nx, &P.tris[4 * (size_t)~ref[q] + 1].w, 4);
        if (nx == REF_FIN) continue;
        if (q >= next_pos.size()) next_pos.resize(q + 1, REF_FIN);
        next_pos[q] = (int)ref.size();
        ref.push_back(nx);
    }
    next_pos.resize(ref.size(), REF_FIN);
    const size_t n = ref.size();
    P.cpos_ref = ref;
    P.cnodes.assign(3 * n, make_float4(0.f, 0.f, 0.f, 0.f));
    P.cranks.assign((n + 31) / 32, make_uint2(0u, 0u));
    unsigned forks = 0;
    for (size_t q = 0; q < n; q++) {
        float4 *o = &P.cnodes[3 * q];
        if (q % 32 == 0) P.cranks[q / 32].y = forks;
        const int r = ref[q];
        if (r >= 0) {
            const float4 *f = &P.forks[4 * (size_t)r];
            o[0] = make_float4(f[0].x, f[0].y, f[0].z, f[3].x);
            o[1] = make_float4(f[1].x, f[1].y, f[1].z, f[3].y);
            o[2] = make_float4(f[2].x, f[2].y, f[2].z, f[3].z);
            P.cranks[q / 32].x |= 1u << (q % 32);
            forks++;
        } else {
            const float4 *t = &P.tris[4 * (size_t)~r];
            o[0] = make_float4(t[0].x, t[0].y, t[0].z, as_float(~r));
            o[1] = make_float4(t[1].x, t[1].y, t[1].z, as_float(next_pos[q]));
            o[2] = make_float4(t[2].x, t[2].y, t[2].z, 0.f);
        }
    }
}

int pack_scene(glrtx_ctx *c, std::string *err_out, Packed &P, const float *vert, size_t n_vert, const float *tri, size_t n_tri,
               const float *mat, size_t n_mat, const float *light, size_t n_light, const float *bvh, size_t n_nodes) {
    if ((n_vert && !vert) || (n_tri && !tri) || (n_mat && !mat) || (n_light && !light) || (n_nodes && !bvh))
        return pfail(c, err_out, GLRTX_EINVAL, "glrtx_upload_scene: NULL buffer with non-zero count");
    if (n_tri > (size_t)INT32_MAX / 4 || n_nodes > (size_t)INT32_MAX / 4 || n_vert > (size_t)INT32_MAX / 16)
        return pfail(c, err_out, GLRTX_EINVAL, "glrtx_upload_scene: scene too large for 32-bit indices");

    auto vidx = [&](float f, int &out) {
        if (!(f >= 0.0f) || (size_t)f >= n_vert) return false;
        out = (int)f;
        return true;
    };

    // ---- triangles: {v0, material} {v1-v0} {v2-v0}; normals {n0} {n1} {n2} -- staged per wire triangle here; the device gets one
    // record per LEAF of the tree (P.tris / P.nrms, filled behind the tree walk below)
    std::vector<float4> tris, nrms;
    tris.assign(4 * n_tri, make_float4(0.f, 0.f, 0.f, 0.f));  // 64-byte records, same shape as a fork record
    nrms.assign(3 * n_tri, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t t = 0; t < n_tri; t++) {
        int i[3];
        for (int k = 0; k < 3; k++)
            if (!vidx(tri[4 * t + k], i[k])) return pfail(c, err_out, GLRTX_ESCENE, "triangle %zu: vertex index %g out of range", t, tri[4 * t + k]);
        const float mf = tri[4 * t + 3];
        if (!(mf >= 0.0f) || (size_t)mf >= n_mat) return pfail(c, err_out, GLRTX_ESCENE, "triangle %zu: material %g out of range", t, mf);
        const float *p0 = vert + 15 * (size_t)i[0], *p1 = vert + 15 * (size_t)i[1], *p2 = vert + 15 * (size_t)i[2];
        tris[4 * t + 0] = make_float4(p0[0], p0[1], p0[2], as_float((int)mf));
        tris[4 * t + 1] = make_float4(p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2], 0.f);
        tris[4 * t + 2] = make_float4(p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2], 0.f);
        nrms[3 * t + 0] = make_float4(p0[3], p0[4], p0[5], 0.f);
        nrms[3 * t + 1] = make_float4(p1[3], p1[4], p1[5], 0.f);
        nrms[3 * t + 2] = make_float4(p2[3], p2[4], p2[5], 0.f);
    }

    // ---- materials: {emission, type} {param0, alpha.x} {param1, alpha.y}
    std::vector<float4> &mats = P.mats;
    mats.assign(3 * n_mat, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t m = 0; m < n_mat; m++) {
        const float *r = mat + 18 * m;
        mats[3 * m + 0] = make_float4(r[3], r[4], r[5], as_float((int)r[0]));
        mats[3 * m + 1] = make_float4(r[6], r[7], r[8], r[12]);
        mats[3 * m + 2] = make_float4(r[9], r[10], r[11], r[13]);
    }

    // ---- lights: {v0, material} {v1} {v2} {n0} {n1} {n2}
    std::vector<float4> &lights = P.lights;
    lights.assign(6 * n_light, make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t l = 0; l < n_light; l++) {
        int i[3];
        for (int k = 0; k < 3; k++)
            if (!vidx(light[4 * l + k], i[k])) return pfail(c, err_out, GLRTX_ESCENE, "light %zu: vertex index out of range", l);
        const float mf = light[4 * l + 3];
        if (!(mf >= 0.0f) || (size_t)mf >= n_mat) return pfail(c, err_out, GLRTX_ESCENE, "light %zu: material out of range", l);
        for (int k = 0; k < 3; k++) {
            const float *p = vert + 15 * (size_t)i[k];
            lights[6 * l + k] = make_float4(p[0], p[1], p[2], k == 0 ? as_float((int)mf) : 0.f);
            lights[6 * l + 3 + k] = make_float4(p[3], p[4], p[5], 0.f);
        }
    }

    // ---- BVH: walk the wire-format tree from node 0, fold leaves into refs, renumber forks in DFS order.
    // Leaf records.  Every leaf the walk reaches gets its own triangle record, numbered in the order the traversal meets them:
    // leaf record k has triangle id k + 1 and lies at record index ~(k + 1) (id 0 / index -1 is the all-zero never-hit record that
    // stands for an absent child).  The id -- not the wire triangle index -- is what the kernels carry in a hit.
    // Leaf pairs.  A fork whose two children are both leaves gets NO fork record: nothing of it is ever tested but its own box, and
    // that sits in its parent's record.  Its two triangle records are chained instead -- the first-visited child's record names the
    // other one's index (its predecessor in memory) in the spare word of its second float4, REF_FIN otherwise -- and the parent refers
    // to the first of them: the traversal step goes from one triangle to the next without a fork fetch, a push and a pop in
    // between (raytrace.frag:299-331: children.y is popped and tested first, then children.x; neither is box-tested).  With the
    // reference's builder 40 % of the forks are such pairs and 94 % of the headline config's triangle tests come through one.
    std::vector<float4> &forks = P.forks;
    forks.clear();
    std::vector<int> leaf_tri;   // leaf record k -> wire triangle
    std::vector<int> leaf_next;  // leaf record k -> ref of the record chained behind it, or REF_FIN
    int root_ref = REF_ABSENT;
    int stack_need = 0;
    const bool chain_pairs = std::getenv("GLRTX_NO_LEAF_CHAINS") == nullptr;  // (A/B switch)
    if (n_nodes > 0 && n_tri > 0) {
        std::vector<int> ref_of(n_nodes, 0);          // ref assigned to each wire node
        std::vector<unsigned char> seen(n_nodes, 0);
        struct Frame { int node; int stage; };
        std::vector<Frame> st;
        std::vector<int> need(n_nodes, 0);
        auto is_fork = [&](int n) { return bvh[9 * (size_t)n + 8] < 0.0f; };
        auto child = [&](int n, int k, int &out) {  // k = 0 left (children.x), 1 right (children.y)
            const float f = bvh[9 * (size_t)n + 6 + k];
            if (!(f >= 0.0f)) { out = -1; return true; }
            if ((size_t)f >= n_nodes) return false;
            out = (int)f;
            return true;
        };
        auto add_leaf = [&](int n, int &rc) {  // a leaf record for wire node n; returns its ref
            rc = GLRTX_OK;
            if (seen[n]) { rc = pfail(c, err_out, GLRTX_ESCENE, "BVH node %d is referenced more than once (not a tree)", n); return 0; }
            seen[n] = 1;
            const float tf = bvh[9 * (size_t)n + 8];
            if ((size_t)tf >= n_tri) { rc = pfail(c, err_out, GLRTX_ESCENE, "BVH leaf %d: triangle %g out of range", n, tf); return 0; }
            leaf_tri.push_back((int)tf);
            leaf_next.push_back(REF_FIN);
            P.leaf_wire.push_back(n);
            ref_of[n] = ~(int)leaf_tri.size();  // id = record count so far (ids start at 1)
            need[n] = 0;
            return ref_of[n];
        };
        st.push_back({0, 0});
        while (!st.empty()) {
            Frame &f = st.back();
            const int n = f.node;
            if (f.stage == 0) {
                if (!is_fork(n)) {
                    int rc;
                    add_leaf(n, rc);
                    if (rc) return rc;
                    st.pop_back();
                    continue;
                }
                if (seen[n]) return pfail(c, err_out, GLRTX_ESCENE, "BVH node %d is referenced more than once (not a tree)", n);
                seen[n] = 1;
                int l, r;
                if (!child(n, 0, l) || !child(n, 1, r)) return pfail(c, err_out, GLRTX_ESCENE, "BVH node %d: child index out of range", n);
                if (chain_pairs && l >= 0 && r >= 0 && l != r && !is_fork(l) && !is_fork(r)) {  // a leaf pair: children.y first, then children.x
                    int rc;
                    const int first = add_leaf(r, rc);
                    if (rc) return rc;
                    const int second = add_leaf(l, rc);
                    if (rc) return rc;
                    leaf_next[(size_t)~first - 1] = second;  // == first - 1: the record in front of it in memory
                    ref_of[n] = first;
                    need[n] = 0;
                    st.pop_back();
                    continue;
                }
                ref_of[n] = (int)(forks.size() / 4);
                // both children start out absent: the never-hit record (index -1) behind an infinite box (see put_box)
                for (int k = 0; k < 4; k++) { const float e = (k & 1) ? kInf : -kInf; forks.push_back(make_float4(e, e, e, as_float(-1))); }
                P.fork_slot.push_back(make_int2(-1, -1));
                // forks are numbered in the order the traversal meets them (children.y first, raytrace.frag:299-307):
                // the first-visited child's record directly follows its parent's
                f.stage = 1;
                if (r >= 0) { st.push_back({r, 0}); }
                continue;
            }
            if (f.stage == 1) {
                f.stage = 2;
                int l;
                child(n, 0, l);
                if (l >= 0) { st.push_back({l, 0}); }
                continue;
            }
            int l, r;
            child(n, 0, l);
            child(n, 1, r);
            const int fi = ref_of[n];
            // child box into the parent's record.  A LEAF child is never box-tested (raytrace.frag:310-331): it gets the box
            // (-inf, +inf), for which the slab test passes by itself with entry distance -inf -- the traversal step then needs no
            // test of the ref's sign (an absent child, the never-hit record, is treated the same way).  A leaf PAIR is a fork in the
            // wire format: its own box goes here like any fork's.
            auto put_box = [&](int slot, int child) {
                if (!is_fork(child)) return;
                (slot ? P.fork_slot[fi].y : P.fork_slot[fi].x) = child;
                const float *b = bvh + 9 * (size_t)child;
                forks[4 * fi + slot].x = b[0]; forks[4 * fi + slot].y = b[1]; forks[4 * fi + slot].z = b[2];
                forks[4 * fi + slot + 1].x = b[3]; forks[4 * fi + slot + 1].y = b[4]; forks[4 * fi + slot + 1].z = b[5];
            };
            // Traversal continues with the right child while the left one waits on the stack.  trav_step treats an absent child like a
            // leaf -- always "passed", never hit -- so a fork with one child still pushes one entry: its only child is stored in the
            // LEFT slot whichever wire slot it came from.  The step then continues with the never-hit record and pops the child right
            // after it, with tHit unchanged in between: the same visits in the same order, and the absent entry never sits on the
            // stack underneath a whole subtree (a chain of one-child forks needs ONE entry, like the reference's own stack).
            if (l >= 0 && r >= 0) {
                put_box(0, l); forks[4 * fi].w = as_float(ref_of[l]);
                put_box(2, r); forks[4 * fi + 1].w = as_float(ref_of[r]);
                need[n] = std::max(1 + need[r], need[l]);
            } else if (l >= 0 || r >= 0) {
                const int only = l >= 0 ? l : r;
                put_box(0, only); forks[4 * fi].w = as_float(ref_of[only]);
                need[n] = std::max(1, need[only]);  // the push of the child itself, then the child's own subtree from an empty stack
            } else need[n] = 1;  // both absent: the left never-hit record is pushed, the right one "visited"
            st.pop_back();
        }
        root_ref = ref_of[0];
        stack_need = need[0];
        P.root_boxed = is_fork(0) ? 1 : 0;  // the wire root's own box is tested first (:296-298) -- also when it is packed as a leaf pair

        // the per-leaf triangle records: id 0 the never-hit record, id k + 1 leaf record k
        P.tris.assign(4 * (leaf_tri.size() + 1), make_float4(0.f, 0.f, 0.f, 0.f));
        P.nrms.assign(3 * (leaf_tri.size() + 1), make_float4(0.f, 0.f, 0.f, 0.f));
        for (size_t k = 0; k < leaf_tri.size(); k++) {
            for (int j = 0; j < 4; j++) P.tris[4 * (k + 1) + j] = tris[4 * (size_t)leaf_tri[k] + j];
            for (int j = 0; j < 3; j++) P.nrms[3 * (k + 1) + j] = nrms[3 * (size_t)leaf_tri[k] + j];
            P.nrms[3 * (k + 1)].w = P.tris[4 * (k + 1)].w;  // the material id rides with the normals (round 6): the shade phase reads it there and no longer fetches the leaf record for one word
            P.tris[4 * (k + 1) + 1].w = as_float(leaf_next[k]);
        }
        P.tris[1].w = as_float(REF_FIN);

        // ---- vine: every fork has a leaf as children.y and the chain continues through children.x (what
        // glrt_bvh_build_chain emits for "brute force, no BVH").  Stored additionally as the list the traversal visits:
        // record i = {box of fork i, its children.y triangle}; the last record = the last fork's children.x leaf.
        if (is_fork(0) && leaf_tri.size() >= 2) {
            std::vector<float4> v;
            v.reserve(4 * leaf_tri.size());
            bool is_vine = true, uniform = true;
            int n = 0;
            auto rec = [&](const float *lo, const float *hi, int t) {  // t: triangle id of a leaf record
                const float4 *T = &P.tris[4 * (size_t)t];  // {v0, mat} {e1} {e2}
                v.push_back(make_float4(lo[0], lo[1], lo[2], T[0].x));
                v.push_back(make_float4(hi[0], hi[1], hi[2], T[0].y));
                v.push_back(make_float4(T[0].z, T[1].x, T[1].y, T[1].z));
                v.push_back(make_float4(T[2].x, T[2].y, T[2].z, as_float(t)));
            };
            const float inf = std::numeric_limits<float>::infinity();
            const float all_lo[3] = {-inf, -inf, -inf}, all_hi[3] = {inf, inf, inf};
            while (true) {
                int l, r;
                child(n, 0, l);
                child(n, 1, r);
                if (l < 0 || r < 0 || is_fork(r)) { is_vine = false; break; }
                const float *b = bvh + 9 * (size_t)n;
                if (std::memcmp(b, bvh, 6 * sizeof(float)) != 0) uniform = false;
                rec(b, b + 3, ~ref_of[r]);
                P.vine_fork.push_back(n);
                P.vine_leaf.push_back(r);
                if (!is_fork(l)) { rec(all_lo, all_hi, ~ref_of[l]); P.vine_leaf.push_back(l); break; }
                n = l;
            }
            if (is_vine && v.size() == 4 * leaf_tri.size()) {
                // Device layout (trav_scan): the n - 1 fork records in groups of four -- the last group filled up with never-hit records (an infinite box, an
                // all-zero triangle: det = 0) --, then the last leaf's record at index vine_main = roundup4(n - 1), then three more never-hit records: the scan
                // works through whole groups while the next ones are being fetched and reads up to three records past the one it needs.
                const size_t n = leaf_tri.size(), n_main = (n - 1 + 3) / 4 * 4;
                std::vector<float4> d(4 * (n_main + 4));
                const float4 pad[4] = {make_float4(-inf, -inf, -inf, 0.f), make_float4(inf, inf, inf, 0.f), make_float4(0.f, 0.f, 0.f, 0.f), make_float4(0.f, 0.f, 0.f, as_float(0))};
                for (size_t i = 0; i < n_main + 4; i++) {
                    const float4 *src = i < n - 1 ? &v[4 * i] : (i == n_main ? &v[4 * (n - 1)] : pad);
                    for (int j = 0; j < 4; j++) d[4 * i + j] = src[j];
                }
                P.vine.swap(d);
                P.n_vine = (int)n;
                P.vine_main = (int)n_main;
                P.vine_uniform = uniform ? 1 : 0;
            }
        }
    }
    // Renumbering: the forks of the tree's top levels (breadth-first from the root, kTopForks of them) take the first indices, the
    // others follow in the order the traversal meets them.  The top of the tree is then one contiguous, hot 8 KiB block.
    if (root_ref >= 0 && forks.size() / 4 > 1) {
        const int nf = (int)(forks.size() / 4);
        std::vector<int> newid(nf, -1), order;
        order.reserve(nf);
        order.push_back(root_ref);
        newid[root_ref] = 0;
        for (size_t q = 0; q < order.size() && (int)order.size() < kTopForks; q++) {
            const int f = order[q];
            int refs[2]; std::memcpy(&refs[0], &forks[4 * f + 0].w, 4); std::memcpy(&refs[1], &forks[4 * f + 1].w, 4);
            for (int k = 1; k >= 0; k--)  // children.y first, as the traversal
                if (refs[k] >= 0 && refs[k] != REF_ABSENT && newid[refs[k]] < 0 && (int)order.size() < kTopForks) { newid[refs[k]] = (int)order.size(); order.push_back(refs[k]); }
        }
        for (int f = 0; f < nf; f++) if (newid[f] < 0) { newid[f] = (int)order.size(); order.push_back(f); }
        std::vector<float4> re(forks.size());
        std::vector<int2> slot_re(P.fork_slot.size());
        for (int f = 0; f < nf; f++) slot_re[(size_t)newid[f]] = P.fork_slot[(size_t)f];
        P.fork_slot.swap(slot_re);
        for (int f = 0; f < nf; f++) {
            for (int k = 0; k < 4; k++) re[4 * (size_t)newid[f] + k] = forks[4 * (size_t)f + k];
            for (int k = 0; k < 2; k++) {
                int r; std::memcpy(&r, &forks[4 * (size_t)f + k].w, 4);
                if (r >= 0) { r = newid[r]; std::memcpy(&re[4 * (size_t)newid[f] + k].w, &r, 4); }
            }
        }
        forks.swap(re);
        root_ref = newid[root_ref];
    }
    P.tree = root_ref != REF_ABSENT;
    if (P.vine.empty()) { P.vine_fork.clear(); P.vine_leaf.clear(); }
    if (root_ref == REF_ABSENT) {  // empty scene: one childless fork, every ray misses
        forks.clear();
        P.fork_slot.assign(1, make_int2(-1, -1));
        for (int k = 0; k < 4; k++) { const float e = (k & 1) ? kInf : -kInf; forks.push_back(make_float4(e, e, e, as_float(-1))); }
        root_ref = 0;
        stack_need = 1;  // a ray that passes the (degenerate) root box pushes the left never-hit record
        P.root_boxed = 1;
        P.root_lo = make_float4(0.f, 0.f, 0.f, 0.f);
        P.root_hi = make_float4(0.f, 0.f, 0.f, 0.f);
        P.tris.assign(4, make_float4(0.f, 0.f, 0.f, 0.f));  // the never-hit record alone
        P.tris[1].w = as_float(REF_FIN);
        P.nrms.assign(3, make_float4(0.f, 0.f, 0.f, 0.f));
    } else if (P.root_boxed) {
        P.root_lo = make_float4(bvh[0], bvh[1], bvh[2], 0.f);
        P.root_hi = make_float4(bvh[3], bvh[4], bvh[5], 0.f);
    }
    if (stack_need > 63)
        return pfail(c, err_out, GLRTX_EDEPTH, "BVH needs %d traversal stack entries; the reference shader's stack holds 64", stack_need + 1);

    P.root_ref = root_ref;
    P.stack_need = stack_need;
    P.leaf_tri.swap(leaf_tri);
    pack_compact(P);
    return GLRTX_OK;
}


int ensure(glrtx_ctx *c, DevBuf &b, size_t bytes) {
    if (b.bytes >= bytes && b.p) return GLRTX_OK;
    dev_free(b);
    HIP_TRY(c, hipMalloc(&b.p, std::max<size_t>(bytes, 64)));
    b.bytes = std::max<size_t>(bytes, 64);
    return GLRTX_OK;
}

// `n_planes` planes of the accumulator's current shape back to back in P, zeroed on the context's stream: H, M and C on first use, at a clear, a bind or a
// reprojection -- whenever the accumulator they sit beside starts again or changes shape.
int plane_zero(glrtx_ctx *c, Plane &P, int n_planes = 1) {
    const size_t bytes = (size_t)n_planes * c->pitch_bytes * (size_t)std::max(c->owned_rows, 1);
    if (int rc = ensure(c, P.buf, bytes)) return rc;
    HIP_TRY(c, hipMemsetAsync(P.buf.p, 0, bytes, c->stream));
    P.stamp(accum_shape(c));
    return GLRTX_OK;
}

// P about to be written at the image's current shape, as packed rows of float4 (N, D, T, B): room for it, and its stamp.
int plane_packed(glrtx_ctx *c, Plane &P) {
    if (int rc = ensure(c, P.buf, (size_t)c->width * (size_t)std::max(c->owned_rows, 1) * sizeof(float4))) return rc;
    P.stamp(packed_shape(c));
    return GLRTX_OK;
}

// The tail of every read-back: behind everything issued, the owned rows of `n_planes` planes that lie back to back at `src` (rows src_pitch apart) into the caller's
// rows (dst_pitch apart, the planes back to back as well).  The caller has refused a dst_pitch below a row.
int read_back(glrtx_ctx *c, const void *src, size_t src_pitch, void *dst, size_t dst_pitch, int n_planes = 1) {
    if (int rc = glrtx_sync(c)) return rc;
    const size_t rows = (size_t)c->owned_rows;
    for (int k = 0; k < n_planes && rows > 0; k++)
        HIP_TRY(c, hipMemcpy2D((char *)dst + (size_t)k * rows * dst_pitch, dst_pitch, (const char *)src + (size_t)k * rows * src_pitch, src_pitch,
                               (size_t)c->width * sizeof(float4), rows, hipMemcpyDeviceToHost));
    return GLRTX_OK;
}

// The tail of every resolve to bytes: the context's byte image at the current shape, `launch` (the pass that fills it, on the context's stream), then the rows to the
// caller.  A member that owns no rows only waits.
template <class Launch>
int resolve_to_caller(glrtx_ctx *c, uint8_t *dst, size_t dst_pitch, Launch &&launch) {
    if (c->owned_rows == 0) return glrtx_sync(c);
    const size_t row = (size_t)c->width * 4;
    if (int rc = ensure(c, c->rgba8, row * (size_t)c->owned_rows)) return rc;
    if (int rc = launch((uchar4 *)c->rgba8.p)) return rc;
    if (int rc = glrtx_sync(c)) return rc;
    HIP_TRY(c, hipMemcpy2D(dst, dst_pitch, c->rgba8.p, row, row, (size_t)c->owned_rows, hipMemcpyDeviceToHost));
    return GLRTX_OK;
}

// Device time of `launches` (one call's worth, on the context's stream) by itself: `reps` of them back to back between one pair of events, after a pass that
// warms the device up.  A single launch between two events carries the command processor's latency on both sides, which says nothing about the kernel.
template <class Launches>
int burst_time(glrtx_ctx *c, int reps, float *ms_per_rep, Launches &&launches) {
    for (int pass = 0; pass < 2; pass++) {
        HIP_TRY(c, hipEventRecord(c->rs0, c->stream));
        for (int i = 0; i < reps; i++)
            if (int rc = launches()) return rc;
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->rs1, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->rs0, c->rs1));
    *ms_per_rep = ms / (float)reps;
    return GLRTX_OK;
}

// The refit plan of a packed scene (glrtx_ctx::Refit), uploaded next to it.  Everything in it is fixed by the topology: which vertices each leaf and light
// record reads, the reachable wire tree (parent, children, the forks without children), where each wire box lands in the packed layouts.
int refit_plan_upload(glrtx_ctx *c, const Packed &P, const float *tri, const float *light, size_t n_light, const float *bvh, size_t n_nodes, size_t n_vert,
                      const size_t bytes[5]) {
    const size_t n_wire = P.tree ? n_nodes : 0, n_leaf = P.leaf_wire.size();
    std::vector<int> parent(n_wire, -1), extra;
    std::vector<int2> kids(n_wire, make_int2(-1, -1));
    if (n_wire) {  // (pack_scene has checked the tree)
        std::vector<int> st{0};
        while (!st.empty()) {
            const int n = st.back();
            st.pop_back();
            const float *b = bvh + 9 * (size_t)n;
            if (!(b[8] < 0.0f)) continue;
            kids[n].x = b[6] >= 0.0f ? (int)b[6] : -1;
            kids[n].y = b[7] >= 0.0f ? (int)b[7] : -1;
            if (kids[n].x < 0 && kids[n].y < 0) extra.push_back(n);
            for (int ch : {kids[n].x, kids[n].y})
                if (ch >= 0) { parent[ch] = n; st.push_back(ch); }
        }
    }
    std::vector<int> ints;
    auto section = [&](size_t words) { while (ints.size() % 4) ints.push_back(0); const size_t at = ints.size(); ints.resize(at + words, -1); return at; };
    const size_t o_leaf = section(4 * n_leaf);
    for (size_t k = 0; k < n_leaf; k++) {
        for (int j = 0; j < 3; j++) ints[o_leaf + 4 * k + j] = (int)tri[4 * (size_t)P.leaf_tri[k] + j];
        ints[o_leaf + 4 * k + 3] = P.leaf_wire[k];
    }
    const size_t o_extra = section(extra.size());
    std::copy(extra.begin(), extra.end(), ints.begin() + o_extra);
    const size_t o_light = section(4 * n_light);
    for (size_t l = 0; l < n_light; l++)
        for (int j = 0; j < 3; j++) ints[o_light + 4 * l + j] = (int)light[4 * l + j];
    const size_t o_parent = section(n_wire);
    std::copy(parent.begin(), parent.end(), ints.begin() + o_parent);
    const size_t o_kids = section(2 * n_wire);
    std::memcpy(&ints[o_kids], kids.data(), n_wire * sizeof(int2));
    const size_t o_slot = section(2 * P.fork_slot.size());
    std::memcpy(&ints[o_slot], P.fork_slot.data(), P.fork_slot.size() * sizeof(int2));
    const size_t o_cpos = section(P.cpos_ref.size());
    for (size_t q = 0; q < P.cpos_ref.size(); q++) ints[o_cpos + q] = P.cpos_ref[q] >= 0 ? P.cpos_ref[q] : -1;
    const size_t o_vf = section(P.vine_fork.size());
    std::copy(P.vine_fork.begin(), P.vine_fork.end(), ints.begin() + o_vf);
    const size_t o_vl = section(P.vine_leaf.size());
    std::copy(P.vine_leaf.begin(), P.vine_leaf.end(), ints.begin() + o_vl);
    // keys: the wire boxes (the uploaded ones: a fork without children keeps its box), the arrival counters (0), eight read-back words
    std::vector<unsigned> keys(7 * n_wire + 8, 0u);
    for (size_t n = 0; n < n_wire; n++)
        for (int j = 0; j < 6; j++) {
            unsigned u; std::memcpy(&u, &bvh[9 * n + j], 4);
            keys[6 * n + j] = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        }
    glrtx_ctx::Refit &R = c->rf;
    if (int rc = dev_upload(c, R.ints, ints.data(), ints.size() * sizeof(int))) return rc;
    if (int rc = dev_upload(c, R.keys, keys.data(), keys.size() * sizeof(unsigned))) return rc;
    if (!R.slot_ev) HIP_TRY(c, hipEventCreateWithFlags(&R.slot_ev, hipEventDisableTiming));
    const int *I = (const int *)R.ints.p;
    unsigned *K = (unsigned *)R.keys.p;
    refit::Args &a = R.a;
    a = refit::Args{};
    a.leaf = (const int4 *)(I + o_leaf); a.n_leaf = (int)n_leaf;
    a.extra = I + o_extra; a.n_extra = (int)extra.size();
    a.light = (const int4 *)(I + o_light); a.n_light = (int)n_light;
    a.parent = I + o_parent; a.kids = (const int2 *)(I + o_kids);
    a.box = K; a.cnt = K + 6 * n_wire; a.out = K + 7 * n_wire;
    a.climb = P.n_vine > 0 ? 0 : 1;
    a.nodes = (uint4 *)c->forks.p; a.n_ids = (int)(P.tris.size() / 4);
    a.nrms = (uint4 *)c->nrms.p; a.lights = (uint4 *)c->lights.p;
    a.slot = (const int2 *)(I + o_slot); a.n_fork = (int)P.fork_slot.size();
    a.cpos = I + o_cpos; a.n_cpos = (int)P.cpos_ref.size(); a.cnodes = (uint4 *)c->cnodes.p;
    a.vine_fork = I + o_vf; a.vine_leaf = I + o_vl; a.n_vine = P.n_vine; a.vine_main = P.vine_main; a.vine = (uint4 *)c->vine.p;
    a.root_boxed = P.tree && P.root_boxed ? 1 : 0;
    R.n_vert = n_vert;
    for (int k = 0; k < 5; k++) R.bytes[k] = bytes[k];
    return GLRTX_OK;
}

#ifdef GLRTX_RAY_LOG
struct DbgLastLaunch { KernelArgs a; WfArgs w; int lds, grid; float4 *queues; int fetch; } g_dbg_last;  // what the last pt_render_wgwf launch was given (replay)
DevBuf g_dbg_log_rays, g_dbg_log_trips;
#endif

// Frames one launch may cover: bounded by a FIXED memory budget for what a launch needs PER FRAME -- one float4 plane per sample and owned pixel -- not by what happens
// to be free on the device, so that the launch shapes, and with them the timing, do not depend on what else runs there (path state does not count: it is addressed by
// workgroup and queue position, 0.8 GB whatever the frames in flight), and by the 31-bit path ids (frame * pixels + pixel).  GLRTX_FRAMES_BUDGET_MB overrides the default (tests).
// `slots`: the budget is shared by that many launches that may be in flight at once (fed launches: kFedSlots).
size_t frames_budget(const glrtx_ctx *c) {  // (this context's share of it)
    size_t budget = (size_t)kFramesBudgetGiB << 30;
    if (const char *v = std::getenv("GLRTX_FRAMES_BUDGET_MB")) budget = (size_t)std::max(1, std::atoi(v)) << 20;
    return budget / (size_t)std::max(c->budget_share, 1);
}
int frames_cap(const glrtx_ctx *c, const glrtx_params *p, int slots) {
    const size_t px = (size_t)((c->width + 7) / 8) * (size_t)((c->owned_rows + 7) / 8) * 64;
    const size_t per_frame = (size_t)std::max(p->n_samples, 1) * c->pitch_bytes * (size_t)std::max(c->owned_rows, 1);
    const size_t budget = frames_budget(c) / (size_t)std::max(slots, 1);
    const size_t id_cap = (((size_t)1 << 31) - 2) / std::max<size_t>(px, 1);  // path ids (frame * pixels + pixel) stay below 2^31
    return (int)std::max<size_t>(1, std::min<size_t>(id_cap, budget / std::max<size_t>(per_frame, 1)));
}

constexpr unsigned kFedSlots = 3;  // fed launches alternate between this many of the context's pipe slots (one renders, one drains into its accumulation pass, one is being fed)

// Nothing is appended to the open launch any more (glrtx_ctx::OpenFeed).  Host side only: the launch itself closes its feed when it runs dry.
void seal_feed(glrtx_ctx *c) {
    c->open.slot = nullptr;
    c->last_was_render = false;
}

// The bound texture set as the kernels take it (n_tex > 0)
static_assert(sizeof(TexDesc) == sizeof(glrtx_texture) && sizeof(glrtx_texture) == sizeof(glrt_detail::TexRecord), "one descriptor layout on the wire, the host and the device");
TexSet tex_set(const glrtx_ctx *c) {
    return TexSet{(const TexDesc *)c->texDesc.p, (const unsigned char *)c->texTexels.p, (const float2 *)c->texSt.p, (const int *)c->texBind.p, c->n_tex,
                  c->have_maps ? (const MapRec *)c->texMaps.p : nullptr};
}

bool same_camera(const glrtx_params &a, const glrtx_params &b) {
    return std::memcmp(a.c2w, b.c2w, sizeof a.c2w) == 0 && std::memcmp(a.s2c, b.s2c, sizeof a.s2c) == 0 && std::memcmp(&a.aperture, &b.aperture, 4) == 0 &&
           std::memcmp(&a.focal, &b.focal, 4) == 0 && a.n_samples == b.n_samples && a.max_depth == b.max_depth;
}

// The sample planes of frames [first, first + n) of the open launch: chunks of kFeedChunkFrames frames, allocated on demand -- also while the launch is running (an
// allocation does not wait for the device; nothing is ever freed here) -- and published through the feed block.
int feed_ensure_chunks(glrtx_ctx *c, glrtx_ctx::PipeSlot &sl, int first, int n, int cap, size_t frame_bytes) {
    for (int k = first / kFeedChunkFrames; k <= (first + n - 1) / kFeedChunkFrames; k++) {
        const int frames_in_chunk = std::min(kFeedChunkFrames, cap - k * kFeedChunkFrames);
        const size_t need = (size_t)std::max(frames_in_chunk, 1) * frame_bytes;
        if (!sl.chunks[k].p || sl.chunks[k].bytes < need) {
            if (sl.chunks[k].p) return fail(c, GLRTX_EDEVICE, "internal: plane chunk %d of a fed launch is too small (%zu < %zu bytes)", k, sl.chunks[k].bytes, need);
            HIP_TRY(c, hipMalloc(&sl.chunks[k].p, std::max<size_t>(need, 64)));
            sl.chunks[k].bytes = std::max<size_t>(need, 64);
        }
        sl.feed_h->chunks[k] = (float4 *)sl.chunks[k].p;
    }
    return GLRTX_OK;
}

// Append n frames to the open launch.  Returns 1 if the launch has taken them (nothing else to do), 0 if the caller must start a launch of its own (no open launch, another
// camera, the launch is full -- or it has closed its feed: the compare-and-swap on the published count fails).  Never an error: whatever goes wrong here, a launch can still be made.
int feed_append(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n) {
    glrtx_ctx::OpenFeed &o = c->open;
    if (!o.slot) return 0;
    if (!same_camera(o.p, *p) || o.frames + n > o.cap || o.vol != (c->ext_flags != 0)) { o.slot = nullptr; return 0; }
    if (feed_ensure_chunks(c, *o.slot, o.frames, n, o.cap, o.frame_bytes) != GLRTX_OK) { (void)hipGetLastError(); c->err.clear(); o.slot = nullptr; return 0; }
    FeedHost *fh = o.slot->feed_h;
    for (int i = 0; i < n; i++) fh->seeds[o.frames + i] = make_float2(seeds_xy[2 * i], seeds_xy[2 * i + 1]);
    unsigned expect = (unsigned)o.frames;  // (release: seeds and chunk pointers before the count that announces them)
    if (!__atomic_compare_exchange_n(&fh->frames_pub, &expect, (unsigned)(o.frames + n), false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)) { o.slot = nullptr; return 0; }
    o.frames += n;
    o.rec->frames = o.frames;
    c->st.frames_last = o.frames;
    c->st.feed_appended += (uint64_t)n;
    c->st.launches += (uint64_t)n;
    c->st.paths += (uint64_t)c->owned_rows * (uint64_t)c->width * (uint64_t)p->n_samples * (uint64_t)n;
    c->counters_stale = c->counters_stale || c->count_rays;
    return 1;
}

// ---- presentation (glrtx_ctx::Present)
bool presenting(const glrtx_ctx *c) { return c->pres.ring > 0; }

size_t present_image_bytes(const glrtx_ctx *c) { return (size_t)c->width * 4 * (size_t)c->owned_rows; }

// Before a render call of n frames changes anything: a free image for each of them (else GLRTX_EBUSY), device images of the current size, pinned ones too (a context's
// own; a group's are ensured by the group).  Growing the device ring waits for everything that may still use it.
int present_prepare(glrtx_ctx *c, int n) {
    if (!presenting(c) || n < 1) return GLRTX_OK;
    glrtx_ctx::Present &P = c->pres;
    if (n > P.ring) return fail(c, GLRTX_EINVAL, "presentation: a call of %d frames needs more images than the ring holds (%d)", n, P.ring);
    for (int k = 0; k < n; k++)
        if (P.img[(P.seq + k) % P.ring].state != glrtx_ctx::Present::Image::FREE) {
            P.st.busy_returns++;
            return fail(c, GLRTX_EBUSY, "presentation: no free ring image for frame %d of this call (release an acquired image first)", k + 1);
        }
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = present_image_bytes(c);
    if (P.dev.bytes < bytes * (size_t)P.ring) {
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        HIP_TRY(c, hipStreamSynchronize(P.copy));
        if (int rc = ensure(c, P.dev, bytes * (size_t)P.ring)) return rc;
    }
    if (!P.full)
        for (int k = 0; k < n; k++) {
            glrtx_ctx::Present::Image &im = P.img[(P.seq + k) % P.ring];
            if (im.host_bytes >= bytes && im.host) continue;  // (allocated up front by glrtx_present_enable: pinning memory waits for the device; only a resize lands here)
            if (im.host) HIP_TRY(c, hipHostFree(im.host));
            im.host = nullptr; im.host_bytes = 0;
            HIP_TRY(c, hipHostMalloc((void **)&im.host, std::max<size_t>(bytes, 64), hipHostMallocPortable));
            im.host_bytes = std::max<size_t>(bytes, 64);
        }
    return GLRTX_OK;
}

// The device image the next frame's pass writes.
uchar4 *present_dev_image(const glrtx_ctx *c, uint64_t seq) {
    return (uchar4 *)((char *)c->pres.dev.p + (size_t)(seq % (uint64_t)c->pres.ring) * present_image_bytes(c));
}

// Device image -> pinned image, on the copy stream.  A context: its owned rows as they are.  A group member: its 8-row stripes in place in the full image -- ONE strided
// copy for the whole stripes (a row of the copy is a stripe, contiguous on both sides; the destination steps by world stripes) and one more for a partial last stripe.
// Flipped, the device image holds the owned rows in reverse: the partial stripe (the image's top rows) first, then the whole stripes in descending order -- ascending
// destinations, so the strided copy runs forward as well.
int present_copy(glrtx_ctx *c, const char *src, uint8_t *dst, int &copies) {
    glrtx_ctx::Present &P = c->pres;
    const size_t rb = (size_t)c->width * 4;
    copies = 0;
    if (c->owned_rows == 0) return GLRTX_OK;
    if (!dst) return fail(c, GLRTX_EINVAL, "presentation: no host image (a group member renders through its group)");
    if (!P.full) {
        HIP_TRY(c, hipMemcpyAsync(dst, src, rb * (size_t)c->owned_rows, hipMemcpyDeviceToHost, P.copy));
        copies = 1;
        return GLRTX_OK;
    }
    const size_t sb = (size_t)c->stripe * rb;
    const int whole = c->owned_rows / c->stripe, tail = c->owned_rows % c->stripe;
    const size_t tail_at = (size_t)(whole * c->world + c->rank) * sb;  // the partial stripe's place (unflipped)
    if (!P.flip) {
        if (whole > 0) HIP_TRY(c, hipMemcpy2DAsync(dst + (size_t)c->rank * sb, (size_t)c->world * sb, src, sb, sb, (size_t)whole, hipMemcpyDeviceToHost, P.copy));
        if (tail > 0) HIP_TRY(c, hipMemcpyAsync(dst + tail_at, src + (size_t)whole * sb, (size_t)tail * rb, hipMemcpyDeviceToHost, P.copy));
    } else {
        if (tail > 0) HIP_TRY(c, hipMemcpyAsync(dst, src, (size_t)tail * rb, hipMemcpyDeviceToHost, P.copy));
        if (whole > 0) {
            const int s_hi = c->rank + (whole - 1) * c->world;  // the member's highest whole stripe: the first one in the flipped image
            const size_t at = (size_t)(c->height - (s_hi + 1) * c->stripe) * rb;
            HIP_TRY(c, hipMemcpy2DAsync(dst + at, (size_t)c->world * sb, src + (size_t)tail * rb, sb, sb, (size_t)whole, hipMemcpyDeviceToHost, P.copy));
        }
    }
    copies = (whole > 0) + (tail > 0);
    return GLRTX_OK;
}

// n frames have been given their images on the device by a pass ordered in front of the copy stream's last wait: number them, copy them out, record their events.
int present_issue(glrtx_ctx *c, int n) {
    glrtx_ctx::Present &P = c->pres;
    for (int k = 0; k < n; k++) {
        glrtx_ctx::Present::Image &im = P.img[P.seq % P.ring];
        int copies = 0;
        if (int rc = present_copy(c, (const char *)present_dev_image(c, P.seq), im.host, copies)) return rc;
        HIP_TRY(c, hipEventRecord(im.ev, P.copy));
        im.state = glrtx_ctx::Present::Image::PENDING;
        im.frame = ++P.frame;
        im.width = c->width;
        im.rows = P.full ? c->height : c->owned_rows;
        P.copies_last = copies;
        P.seq++;
        P.st.images++;
    }
    return GLRTX_OK;
}

// Around a presenting pass on the context's stream: timing, then the copy stream is ordered behind it and its n frames are issued.
int present_pass_begin(glrtx_ctx *c) {
    HIP_TRY(c, hipEventRecord(c->pres.t0, c->stream));
    return GLRTX_OK;
}
int present_pass_end(glrtx_ctx *c, int n) {
    glrtx_ctx::Present &P = c->pres;
    HIP_TRY(c, hipEventRecord(P.t1, c->stream));
    P.timed = true;
    HIP_TRY(c, hipEventRecord(P.pass_done, c->stream));
    HIP_TRY(c, hipStreamWaitEvent(P.copy, P.pass_done, 0));
    return present_issue(c, n);
}

// The image of a launch whose render kernel accumulated by itself (no planes): the resolve kernel into the frame's device image, behind the launch.
int present_resolve(glrtx_ctx *c) {
    if (c->owned_rows == 0) return present_issue(c, 1);
    if (int rc = present_pass_begin(c)) return rc;
    hipLaunchKernelGGL(resolve_kernel<kResolvePer>, resolve_grid(c->width, c->owned_rows), dim3(256), 0, c->stream, (const float4 *)c->accum,
                       (int)(c->pitch_bytes / sizeof(float4)), c->width, c->owned_rows, present_dev_image(c, c->pres.seq), c->width, c->pres.inv_gamma, c->pres.flip);
    HIP_TRY(c, hipGetLastError());
    return present_pass_end(c, 1);
}

// Presentation off: nothing is appended to an open launch (its pass might write images), every pass and copy has ended, the images not acquired are dropped.
int present_stop(glrtx_ctx *c) {
    glrtx_ctx::Present &P = c->pres;
    if (P.ring == 0) return GLRTX_OK;
    for (const auto &im : P.img)
        if (im.state == glrtx_ctx::Present::Image::HELD) return fail(c, GLRTX_EINVAL, "presentation: release the acquired images first");
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipStreamSynchronize(P.copy));
    P.st.dropped += P.seq - P.acq;
    for (auto &im : P.img) {
        if (im.ev) (void)hipEventDestroy(im.ev);
        if (im.host && !P.full) (void)hipHostFree(im.host);
    }
    P.img.clear();
    dev_free(P.dev);
    P.ring = 0;
    P.seq = P.acq = 0;
    return GLRTX_OK;
}

// Presentation on: images of their own (group members: host images borrowed from the group, set by it).
int present_start(glrtx_ctx *c, int ring, float gamma, int flip, bool full) {
    if (int rc = present_stop(c)) return rc;
    if (ring < 0 || ring > 1024) return fail(c, GLRTX_EINVAL, "glrtx_present_enable: ring_images %d (0 .. 1024)", ring);
    if (ring == 0) return GLRTX_OK;
    if (!(gamma > 0.f)) return fail(c, GLRTX_EINVAL, "glrtx_present_enable: gamma must be positive");
    glrtx_ctx::Present &P = c->pres;
    seal_feed(c);  // (a launch started before this call has a pass without images: nothing more goes into it)
    HIP_TRY(c, hipSetDevice(c->device));
    if (!P.copy) {
        HIP_TRY(c, hipStreamCreateWithFlags(&P.copy, hipStreamNonBlocking));
        HIP_TRY(c, hipEventCreateWithFlags(&P.pass_done, hipEventDisableTiming));
        HIP_TRY(c, hipEventCreate(&P.t0));
        HIP_TRY(c, hipEventCreate(&P.t1));
    }
    P.img.assign((size_t)ring, glrtx_ctx::Present::Image{});
    for (auto &im : P.img) HIP_TRY(c, hipEventCreateWithFlags(&im.ev, hipEventDisableTiming));
    P.ring = ring;
    P.inv_gamma = 1.0f / gamma;
    P.flip = flip ? 1 : 0;
    P.full = full;
    P.seq = P.acq = 0;
    P.timed = false;
    if (c->width > 0) {  // every image of the current size now: allocating pinned memory waits for the device, so it must not happen between two frames of a burst
        int rc = ensure(c, P.dev, present_image_bytes(c) * (size_t)ring);
        for (auto &im : P.img) {
            if (rc != GLRTX_OK || full) break;
            const hipError_t e = hipHostMalloc((void **)&im.host, std::max<size_t>(present_image_bytes(c), 64), hipHostMallocPortable);
            if (e != hipSuccess) rc = fail(c, GLRTX_ENOMEM, "glrtx_present_enable: pinned host memory: %s", hipGetErrorString(e));
            else im.host_bytes = std::max<size_t>(present_image_bytes(c), 64);
        }
        if (rc != GLRTX_OK) { (void)present_stop(c); return rc; }
    }
    return GLRTX_OK;
}

bool present_held(const glrtx_ctx *c) {
    for (const auto &im : c->pres.img)
        if (im.state == glrtx_ctx::Present::Image::HELD) return true;
    return false;
}

// ---- a render launch (variant 2).  What one launch is asked for.  The entry points make it and pass it through render_one into launch_wgwf: nothing about a launch travels through the context.
struct RenderReq {
    // Ordinary: glrtx_render / glrtx_render_frames.
    // Adaptive (glrtx_render_adaptive): the ADAPT kernel over the selection's active tiles -- plain, on the context's stream, always with sample planes, never fed.
    // Moments (glrtx_render_moments): the same shape -- plain, with sample planes, never fed -- on the ordinary kernel; the pass folds the planes into M as well.
    // Calibration (glrtx_hit_histogram): one plain single-frame launch on the context's stream that counts closest hits per leaf record into `hit_hist` while it shades
    //     into `scratch` instead of the accumulator: no pipe slot, no ray counting, no presentation step.
    // AdaptiveMoments (glrtx_render_adaptive_moments): Adaptive's launch on the selection made from M; the pass folds the active tiles' planes into M, not into H.
    // Cascades (glrtx_render_cascades): Moments' launch; the pass folds the planes into the cascade planes C instead of M.
    enum Kind { Ordinary, Adaptive, Moments, Calibration, AdaptiveMoments, Cascades } kind = Ordinary;
    bool adaptive() const { return kind == Adaptive || kind == AdaptiveMoments; }
    bool folds_moments() const { return kind == Moments || kind == AdaptiveMoments; }
    const float *seeds = nullptr;  // {x, y} per frame; a single frame's seed is the parameters' own
    int n_frames = 1;
    unsigned *hit_hist = nullptr; float4 *scratch = nullptr;  // Calibration
    bool calibration() const { return kind == Calibration; }
    bool count_rays(const glrtx_ctx *c) const { return c->count_rays && !calibration(); }
    bool presents(const glrtx_ctx *c) const { return presenting(c) && !calibration(); }
    float4 *accum(const glrtx_ctx *c) const { return calibration() ? scratch : c->accum; }
};

// ---- a launch's route (host/route_statement.h; DESIGN.md "A launch's route"): which kernel a call of `kind` runs on this context with these parameters, in
// which shading form, what the statistics say about it -- or why the call refuses.  Stated there, once; here the context's fields are handed over.  The two
// switches are read once a call: glrtx_set_*_wavefront's value, or GLRTX_VOLUME_WAVEFRONT / GLRTX_TEXTURE_WAVEFRONT = 0/1 in its place.
using glrt_detail::Route;
static_assert(glrt_detail::kWfDepthMax == kWfDepthMax && glrt_detail::kWfSampleMax == kWfSampleMax && glrt_detail::kWfVolSampleMax == kWfVolSampleMax,
              "the route statement's ranges are the path state's");
static_assert(glrt_detail::kRouteExtVolume == GLRTX_EXT_VOLUME && glrt_detail::kRouteFallbackDepth == GLRTX_FALLBACK_DEPTH &&
              glrt_detail::kRouteFallbackSamples == GLRTX_FALLBACK_SAMPLES && glrt_detail::kRouteFallbackExtensions == GLRTX_FALLBACK_EXTENSIONS, "the route statement's flag values");
static_assert((int)RenderReq::Ordinary == glrt_detail::kRouteOrdinary && (int)RenderReq::Adaptive == glrt_detail::kRouteAdaptive &&
              (int)RenderReq::Moments == glrt_detail::kRouteMoments && (int)RenderReq::Calibration == glrt_detail::kRouteCalibration &&
              (int)RenderReq::AdaptiveMoments == glrt_detail::kRouteAdaptiveMoments && (int)RenderReq::Cascades == glrt_detail::kRouteCascades, "the route statement's request kinds");
bool wavefront_switch(const char *name, bool set) {
    const char *v = std::getenv(name);
    return v ? std::atoi(v) != 0 : set;
}
Route route_of(const glrtx_ctx *c, const glrtx_params *p, RenderReq::Kind kind) {
    const glrt_detail::RouteState s{c->variant,  c->ext_flags, c->n_spheres, c->n_tex,    c->sc.n_vine, c->have_volume, c->have_maps,
                                    c->have_cut, c->have_emit, c->have_env,  wavefront_switch("GLRTX_VOLUME_WAVEFRONT", c->vol_wavefront),
                                    wavefront_switch("GLRTX_TEXTURE_WAVEFRONT", c->tex_wavefront), p->max_depth, p->n_samples};
    return glrt_detail::launch_route(s, (glrt_detail::RouteKind)kind);
}
bool on_wavefront(const Route &r) { return r.refusal.empty() && r.family == glrt_detail::kRouteWavefront; }
int route_refusal(glrtx_ctx *c, const Route &r, const char *fn) { return r.refusal.empty() ? GLRTX_OK : fail(c, GLRTX_EINVAL, "%s: %s", fn, r.refusal.c_str()); }

// The node fetch the wavefront kernel's traversal uses on this scene (vine: the list scan, fetch 0): 0 one record per lane, 1 pair-cooperative, 2 the two
// in alternate steps.  Picked by the size of the record array; GLRTX_PAIR_FETCH=0/1/2 overrides (read at every launch).  (See wgwf_kernel.)
int wgwf_fetch(const glrtx_ctx *c, bool vine) {
    int fetch = vine ? 0 : ((size_t)c->n_fork + (size_t)c->st.n_tri >= (size_t)kPairFetchMinRecords ? 1 : 0);
    if (const char *v = std::getenv("GLRTX_PAIR_FETCH")) fetch = vine ? 0 : std::max(0, std::min(2, std::atoi(v)));
    return fetch;
}

// The wavefront kernel's LDS without the compact layout's rank table: materials and lights | stacks | ctl | root box | camera block | seeds | light-test bits
int wgwf_lds_base(const glrtx_ctx *c) {
    return c->sc.lds_head_f4 * (int)sizeof(float4) + 2 * c->sc.stack_entries * kBlockThreads * (int)sizeof(int) + kWgCtlWords * (int)sizeof(unsigned) +
           2 * (int)sizeof(float4) + kCamFloatsPadded * (int)sizeof(float) + kLdsSeeds * (int)sizeof(float2) + kWgPathsMax / 8;
}

// Whether the wavefront kernel walks the compact node array (pack_compact: 48-byte records, three loads per step instead of four): it serves the
// one-record-per-lane fetch when its rank table fits in LDS beside everything else with GLRTX_WGWF_WAVES workgroups per CU still resident;
// GLRTX_COMPACT_NODES=0/1 overrides (1: as long as one workgroup fits).  The ray queries (glrtx_trace_rays) follow the same rule.
bool wgwf_compact(const glrtx_ctx *c, bool vine, int fetch) {
    const int lds_compact = wgwf_lds_base(c) + c->sc.n_crank * (int)sizeof(uint2);
    bool compact = !vine && fetch == 0 && c->sc.n_crank > 0 && (size_t)lds_compact * GLRTX_WGWF_WAVES <= (size_t)160 * 1024;
    if (const char *v = std::getenv("GLRTX_COMPACT_NODES")) compact = std::atoi(v) != 0 && !vine && fetch == 0 && c->sc.n_crank > 0 && lds_compact <= 160 * 1024;
    return compact;
}

// Variant 2: one persistent launch; every workgroup runs the wavefront trips of the pixels it takes from the frame's tile counter.
// n_frames > 1 ("frames in flight"): the launch covers n_frames consecutive frames that differ only in u_seed (seeds_xy);
// the per-sample planes are added to the accumulator in frame order afterwards (accumulate.hip.h), so the result is bit-identical to
// n_frames separate launches.  launch_wgwf is the steps below, in order; what they work out about the launch is gathered here.
using WgwfFn = void (*)(const KernelArgs, const WfArgs, unsigned *, float4 *, const int *, const unsigned *, const VolArgs, const TexSet);
struct WgwfLaunch {
    const glrtx_params *p;
    RenderReq req;
    const float *seeds_xy;  // n_frames seeds
    KernelArgs a;
    // sizes: 8x8 tiles per row, pixels of the whole tiles (path id = frame * total + pixel), one sample plane, one frame's planes
    int n_frames, n_planes, tiles8_x;
    size_t total, plane_f4, plane_bytes, frame_bytes;
    struct Form { bool busy, fed, piped; int fed_cap; } f;  // (wgwf_form)
    size_t ids;
    struct Kernel { WgwfFn fn; const char *name; bool vol, tex, maps, vine, compact, adapt; int fetch, lds, per_cu; size_t wg_slots; } k;  // (wgwf_kernel)
    glrtx_ctx::PipeSlot *slot;  // (wgwf_pipe_slot; null: plain)
    int pipe_busy, block_paths, grid;
    bool ctx_state;  // (wgwf_args) the buffers the kernel runs on, its stream, its arguments
    DevBuf *stateBuf, *queueBuf, *planeBuf;
    unsigned *workPtr;
    hipStream_t rstream;
    size_t state_entries, state_bytes;
    WfArgs w;
};

// ---- which form.  Three:
//   fed        -- on one of the context's pipe slots (own stream, state, queues, tile counter, plane chunks); the launch stays OPEN: later calls with the same camera
//                 append their frames to it while it runs (feed_append).  Every multi-frame launch on the context's own stream, and a single-frame launch that
//                 follows another one directly (a burst)
//   overlapped -- a single-frame launch on a pipe slot, the frame spread over all workgroup slots in one helping, slots handed over progressively (round 3): what a
//                 caller gets that renders, resolves and saves every frame -- the reference's loop, window.cpp:121-169 -- and any single frame on a caller's stream
//   plain      -- on the context's stream, nothing overlaps: multi-frame launches on a caller's stream (stream order is the caller's), GLRTX_NO_PIPELINE=1, and every
//                 launch that is not an ordinary one (RenderReq)
WgwfLaunch::Form wgwf_form(glrtx_ctx *c, const WgwfLaunch &L) {
    const glrtx_params *p = L.p;
    WgwfLaunch::Form f{};
    // (busy: the context's last render kernel -- a slot's, or one on the context's stream -- has not ended yet)
    f.busy = c->last_render_done && hipEventQuery(c->last_render_done) == hipErrorNotReady;
    (void)hipGetLastError();
    const bool burst = c->last_was_render && f.busy && same_camera(c->last_p, *p);
    const bool ordinary = L.req.kind == RenderReq::Ordinary;
    f.fed = ordinary && c->feed_ok && std::getenv("GLRTX_NO_FEED") == nullptr && c->pipeline && c->stream == c->own_stream && p->n_samples >= 1 && L.seeds_xy != nullptr &&
            (L.n_frames > 1 || burst);
    f.fed_cap = f.fed ? std::min(frames_cap(c, p, (int)kFedSlots), kFeedMaxFrames) : 0;
    if (const char *v = std::getenv("GLRTX_FEED_CAP")) f.fed_cap = std::max(1, std::min(f.fed_cap, std::atoi(v)));  // (tests: launches that fill up)
    if (f.fed && L.n_frames > f.fed_cap) f.fed = false;
    f.piped = f.fed || (ordinary && L.n_frames == 1 && c->pipeline && p->n_samples >= 1 && (size_t)p->n_samples * L.plane_bytes <= ((size_t)1 << 30));
    return f;
}

// ---- the kernel and how many of its workgroups fit the device.  The shading form -- plain, V, T or TM -- is the route's (route_of); the traversal that serves
// it is chosen here, from the tree and its size.  The plain form has four: ray counting on/off x (list scan of a vine (brute-force) tree | tree traversal
// with one record per lane | with the pair-cooperative node fetch | with the two in alternate steps).  The pair fetch trades 25 vector-ALU instructions per step for a
// third less time in the CU's vector-memory pipe (trav_asm.hip.h): it pays where a wave's lanes are spread over many records -- large trees, incoherent rays: config 5
// (100 k triangles) -9 % per frame -- and costs ~1 % where they share the top of a small tree (headline, 10 k triangles: the step is paced by instruction issue there),
// profiles/r04_ab_pair_fetch.txt.  Picked by the size of the record array; GLRTX_PAIR_FETCH=0/1 overrides.  All forms are bit-identical (same IEEE operations on the same record).
// On small trees the two forms in alternate steps (FETCH 2: the pipe is the busier unit in one step, the SIMDs in the next) beat both by 1.0 .. 1.3 % in round 4.
// Since the path state is read and written by queue position (WfArgs::state) the pipe has a fifth less to do and the plain form wins there: headline -0.7 %,
// config 2 -0.4 %, config 4 -1.0 % against the alternating one, the pure pair form +1.9 % (profiles/r05_state_by_position.txt).  The alternating form stays
// compiled in (GLRTX_PAIR_FETCH=2).  Random triangle soups prefer the pair form from 10 k triangles on (-2 %; 20 k: -4.5 %, 70 k: -7 %): what decides is how
// far apart a wave's rays are in the tree, which the record count only approximates.
// The compact node array (pack_compact) has its own four: wgwf_compact.
// The V form (kWgwfVolume: glrtx_set_volume_wavefront; routed here only with the volume alone) has one fetch form only: one record per lane on
// DevScene::nodes, as in the megakernels (no list scan, no pair fetch, no compact layout).
// The T and TM forms (kWgwfTextured, kWgwfMaps: glrtx_set_texture_wavefront; routed here only with a texture set alone) exist for the fetch forms the
// host picks for trees by default -- one record per lane, pair-cooperative, the compact array --: a forced GLRTX_PAIR_FETCH=2 is served as 0, a vine never gets here.
// Each of the twelve has its ADAPT twin (kWgwfAdaptive: glrtx_render_adaptive, glrtx_render_adaptive_moments): 48 instantiations, one table.
enum WgwfTrav { kTravVine, kTravFetch0, kTravFetch1, kTravFetch2, kTravCompact, kTravVolume, kTravTex0, kTravTex1, kTravTexCompact, kTravMaps0, kTravMaps1, kTravMapsCompact,
                kTravForms };
#define GLRTX_WGWF_ROW(VINE, FLAGS) {{pt_render_wgwf<false, VINE, FLAGS>, pt_render_wgwf<true, VINE, FLAGS>}, \
                                     {pt_render_wgwf<false, VINE, (FLAGS) | kWgwfAdaptive>, pt_render_wgwf<true, VINE, (FLAGS) | kWgwfAdaptive>}}
constexpr WgwfFn kWgwfKernels[kTravForms][2][2] = {  // [traversal][adaptive][count_rays]; the names of the shading forms: glrt_detail::kWgwfNames
    GLRTX_WGWF_ROW(true, 0), GLRTX_WGWF_ROW(false, 0), GLRTX_WGWF_ROW(false, 1), GLRTX_WGWF_ROW(false, 2), GLRTX_WGWF_ROW(false, kWgwfCompact), GLRTX_WGWF_ROW(false, kWgwfVolume),
    GLRTX_WGWF_ROW(false, kWgwfTextured), GLRTX_WGWF_ROW(false, kWgwfTextured | 1), GLRTX_WGWF_ROW(false, kWgwfTextured | kWgwfCompact),
    GLRTX_WGWF_ROW(false, kWgwfTextured | kWgwfMaps), GLRTX_WGWF_ROW(false, kWgwfTextured | kWgwfMaps | 1), GLRTX_WGWF_ROW(false, kWgwfTextured | kWgwfMaps | kWgwfCompact)};
#undef GLRTX_WGWF_ROW

int wgwf_kernel(glrtx_ctx *c, WgwfLaunch &L, const Route &route) {
    WgwfLaunch::Kernel &k = L.k;
    k.vol = route.vol; k.tex = route.tex; k.maps = route.maps; k.vine = route.vine;  // the shading form: the route's (a set beside the volume or on a vine never gets here)
    k.adapt = L.req.adaptive();
    k.fetch = k.vol ? 0 : wgwf_fetch(c, k.vine);
    if (k.tex && k.fetch == 2) k.fetch = 0;  // (the alternating fetch has no T form: served as one record per lane, and reported so)
    c->st.node_fetch_last = k.fetch;
    k.compact = !k.vol && wgwf_compact(c, k.vine, k.fetch);
    c->st.node_layout_last = k.compact ? 1 : 0;
    const int trav = k.tex ? (k.maps ? kTravMaps0 : kTravTex0) + (k.compact ? 2 : k.fetch)
                           : k.vol ? kTravVolume : k.compact ? kTravCompact : k.vine ? kTravVine : kTravFetch0 + k.fetch;
    k.fn = kWgwfKernels[trav][k.adapt][L.req.count_rays(c)];
    k.name = route.kernel;
    // (north_star's "primitives staged into LDS": materials, camera block, root box and the per-lane stacks are; the top tree levels were built, measured worth
    // nothing -- profiles/r02_lds_top.json -- and removed.)
    k.lds = wgwf_lds_base(c) + (k.compact ? c->sc.n_crank * (int)sizeof(uint2) : 0);  // | rank table
    if (k.lds > 160 * 1024) return fail(c, GLRTX_EDEVICE, "wgwf kernel needs %d B of LDS (> 160 KiB)", k.lds);
    if (k.lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void *)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds));
    k.per_cu = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&k.per_cu, k.fn, kBlockThreads, k.lds));
    // (launch_bounds' second argument is a minimum, not a cap: an instantiation with little LDS may be reported with more workgroups per CU than the buffers below are
    //  sized for -- ADVICE round 5)
    k.per_cu = std::max(1, std::min(k.per_cu, GLRTX_WGWF_WAVES));
    if (const char *v = std::getenv("GLRTX_WGS_PER_CU")) k.per_cu = std::max(1, std::min(k.per_cu, std::atoi(v)));  // occupancy experiments
    k.wg_slots = (size_t)c->n_cu * (size_t)k.per_cu;
    return GLRTX_OK;
}

// ---- the persistent megakernel (variant 1: render_one): its instantiation and its grid, then the launch.  The eighteen forms of pt_render_persistent that
// exist, each with and without ray counting: one table, in the order of glrt_detail::PersistForm -- the route picks the row and knows its name.
using glrt_detail::kPersistForms;
#define GLRTX_PERSIST_ROW(EXT, VOL, TEX, ENV, MAPS) \
    {(const void *)pt_render_persistent<false, EXT, VOL, TEX, ENV, MAPS>, (const void *)pt_render_persistent<true, EXT, VOL, TEX, ENV, MAPS>}
#define GLRTX_PERSIST_CUT_ROW(ENV, MAPS) \
    {(const void *)pt_render_persistent<false, true, false, true, ENV, MAPS, true>, (const void *)pt_render_persistent<true, true, false, true, ENV, MAPS, true>}
#define GLRTX_PERSIST_EMIT_ROW(ENV, MAPS) \
    {(const void *)pt_render_persistent<false, true, false, true, ENV, MAPS, false, Emit>, (const void *)pt_render_persistent<true, true, false, true, ENV, MAPS, false, Emit>}
// [form][count_rays]; the fourth argument is a VolArgs, in the kFormEnv* rows an EnvArgs, in the k*Cut rows a CutTail of either (include/glrtx.h "Cutouts"),
// in the k*Emit rows an EmitTail of either (include/glrtx.h "Emission maps")
const void *const kPersistent[kPersistForms][2] = {  // plain, ext, vol | tex, +vol, +maps, +vol +maps | env, +tex, +tex +maps | cut: tex, +maps, env +tex, +maps | emit: likewise
    GLRTX_PERSIST_ROW(false, false, false, false, false), GLRTX_PERSIST_ROW(true, false, false, false, false), GLRTX_PERSIST_ROW(true, true, false, false, false),
    GLRTX_PERSIST_ROW(true, false, true, false, false),   GLRTX_PERSIST_ROW(true, true, true, false, false),   GLRTX_PERSIST_ROW(true, false, true, false, true),
    GLRTX_PERSIST_ROW(true, true, true, false, true),     GLRTX_PERSIST_ROW(true, false, false, true, false),  GLRTX_PERSIST_ROW(true, false, true, true, false),
    GLRTX_PERSIST_ROW(true, false, true, true, true),
    GLRTX_PERSIST_CUT_ROW(false, false), GLRTX_PERSIST_CUT_ROW(false, true), GLRTX_PERSIST_CUT_ROW(true, false), GLRTX_PERSIST_CUT_ROW(true, true),
    GLRTX_PERSIST_EMIT_ROW(false, false), GLRTX_PERSIST_EMIT_ROW(false, true), GLRTX_PERSIST_EMIT_ROW(true, false), GLRTX_PERSIST_EMIT_ROW(true, true)};
#undef GLRTX_PERSIST_ROW
#undef GLRTX_PERSIST_EMIT_ROW
#undef GLRTX_PERSIST_CUT_ROW
struct PersistLaunch { const void *fn; int lds, grid; ExtArgs ex; };

// lds: the plain kernel's LDS bytes
int persist_kernel(glrtx_ctx *c, const Route &route, int lds, PersistLaunch &k) {
    k.fn = kPersistent[route.form][c->count_rays];
    k.ex = ExtArgs{};
    if (route.tex) k.ex.tex = tex_set(c);
    k.ex.spheres = (const float4 *)c->spheres.p; k.ex.sphere_mat = (const int *)c->sphereMat.p;
    k.ex.n_spheres = c->n_spheres; k.ex.flags = c->ext_flags;
    k.lds = lds + (route.ext ? c->n_spheres * (int)sizeof(float4) : 0);  // extension kernel: the spheres are staged behind the stacks
    if (k.lds > 160 * 1024) return fail(c, GLRTX_EDEVICE, "render kernel needs %d B of LDS (> 160 KiB)", k.lds);
    if (k.lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, k.lds));
    // grid = what is resident at once (occupancy x CUs), capped by the work available
    int per_cu = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k.fn, kBlockThreads, k.lds));
    if (per_cu < 1) per_cu = 1;
    const int tiles8 = ((c->width + 7) / 8) * ((c->owned_rows + 7) / 8);
    const int n_chunks = (tiles8 * 64 + kChunk - 1) / kChunk;
    const int waves_per_wg = kBlockThreads / 64;
    k.grid = std::max(1, std::min(per_cu * c->n_cu, (n_chunks + waves_per_wg - 1) / waves_per_wg));
    return GLRTX_OK;
}

int persist_launch(glrtx_ctx *c, const Route &route, const PersistLaunch &k, const KernelArgs &a, hipEvent_t ev0) {
    HIP_TRY(c, hipMemsetAsync(c->work.p, 0, sizeof(unsigned), c->stream));
    HIP_TRY(c, hipEventRecord(ev0, c->stream));
    c->last_kernel = route.kernel;
    unsigned *work = (unsigned *)c->work.p;
    const VolArgs va = route.vol ? c->vol : VolArgs{};  // the fourth argument: the volume's, or (kFormEnv*) the environment's
    EnvArgs ea = c->env;
    if (route.env) ea.p_env = c->sc.n_light == 0 ? 1.0f : c->env_cfg.light_pick;  // a scene without lights: the environment is the only light to pick
    // the CUT forms: the same fourth argument with the cutout tables appended behind it (pt_kernel.hip.h: CutTail)
    const CutSet cs{(const int *)c->cutTri.p, (const CutRec *)c->cutRec.p};
    const CutTail<VolArgs> va_cut{va, cs};
    const CutTail<EnvArgs> ea_cut{ea, cs};
    // the EMIT forms: likewise, with the emission table (pt_kernel.hip.h: EmitTail)
    const EmitSet es{(const int *)c->emitMat.p, (const float2 *)c->emitSt.p};
    const EmitTail<VolArgs> va_emit{va, es};
    const EmitTail<EnvArgs> ea_emit{ea, es};
    void *const tail = route.emit ? (route.env ? (void *)&ea_emit : (void *)&va_emit)
                       : route.cut ? (route.env ? (void *)&ea_cut : (void *)&va_cut) : (route.env ? (void *)&ea : (void *)&va);
    void *args[] = {(void *)&a, &work, (void *)&k.ex, tail};
    HIP_TRY(c, hipLaunchKernel(k.fn, dim3(k.grid), dim3(kBlockThreads), args, k.lds, c->stream));
    return GLRTX_OK;
}

// ---- the launch's shape.  plain / fed: every workgroup keeps up to kWgPathsMax paths alive, less when the launch is short (below; a fed launch is sized as if it were to take
// 16 frames: it may).  overlapped, issued while the context's last launch is still rendering: the frame in ONE helping per workgroup, spread over all the slots (the smallest power of two that holds
// work / resident paths: 2048 at 1080p; with 1024 the workgroups come back for a second helping, 1.31 instead of 1.24 ms per frame, with 4096 half of them get
// nothing, 1.67), every launch has the full grid and takes its tiles without guided self-scheduling, so its workgroups do not finish together -- one that finds the
// tile counter exhausted and its paths dead leaves, and a workgroup of the next launch (queued on another stream) takes the slot (profiles/r03_ab_pipeline.txt).
void wgwf_shape(const glrtx_ctx *c, const WgwfLaunch &L, bool overlapped, bool is_fed, int share, bool device_busy, int &block_paths, int &grid) {
    const int n_frames = L.n_frames, fed_cap = L.f.fed_cap, n_samples = L.p->n_samples;
    const size_t total = L.total;
    const int resident = std::max(1, L.k.per_cu / std::max(share, 1)) * c->n_cu;
    const size_t work = total * (size_t)(is_fed ? std::max(n_frames, std::min(16, fed_cap)) : n_frames);
    block_paths = kWgPathsMax;
    if (overlapped && device_busy) { block_paths = 256; while (block_paths < kWgPathsMax && (size_t)resident * block_paths < work) block_paths *= 2; }
    else {
        // A launch ends with a tail in which its last paths run out -- about one path item's lifetime, and an item is a pixel's n_samples samples in sequence
        // (their random numbers are one chain) -- and nothing overlaps that tail when the launch is alone on the device (plain, fed, or a single frame issued
        // to an idle device).  Fewer paths per workgroup mean more, shorter helpings and a shorter tail, but slower trips: the most paths that still give the
        // launch two helpings per workgroup (several frames of one sample per pixel) or four (more samples: longer items; a single frame: its tail is as long
        // as the rest of it).  Lone launches, profiles/r06_launch_shapes.txt: 1080p 1 spp, one frame 2.4 -> 1.67 ms (config 2: 2.1 -> 1.39, config 3: 17.0 -> 11.4,
        // config 5: 4.6 -> 3.1); 16 spp, one frame 39 -> 24 ms, four frames 19.4 -> 18.5; config 4 (4K, 16 spp), one frame 51 -> 39 ms.
        const size_t tenths = (n_samples > 1 || (n_frames == 1 && !is_fed)) ? 39 : 19;
        while (block_paths > 512 && work * 10 < tenths * (size_t)resident * block_paths) block_paths /= 2;
        while (block_paths > 256 && work < (size_t)resident * block_paths) block_paths /= 2;  // (small images: every workgroup of the grid has a full helping)
    }
    if (const char *v = std::getenv("GLRTX_BLOCK_PATHS")) { const int x = std::atoi(v); if (x >= 256 && x <= kWgPathsMax && (x & (x - 1)) == 0) block_paths = x; }
    grid = std::max(1, (int)std::min<size_t>((size_t)resident, (work + block_paths - 1) / block_paths));
}

// ---- a pipe slot (fed and overlapped launches).  A slot owns path state, per-workgroup queues and sample planes of its own (~0.8 GB at 1080p for an overlapped
// single frame, 1.4 GB + planes for a fed launch): the slots are charged to the same memory budget as the frames in flight (kFramesBudgetGiB, split between the members
// of a group that share this GPU), a slot whose buffers cannot be allocated is given up -- the launch then runs plain on the context's stream instead of failing -- and
// among the slots in use the next one whose previous launch has completed is taken (round robin only when none has), so that a launch never queues behind a busy slot
// while an idle one exists.  Leaves L.slot (null: the launch runs plain) and the launch's shape.
int wgwf_pipe_slot(glrtx_ctx *c, WgwfLaunch &L) {
    WgwfLaunch::Form &f = L.f;
    const int n_frames = L.n_frames;
    const size_t frame_bytes = L.frame_bytes;
    glrtx_ctx::PipeSlot *&slot = L.slot = nullptr;
    int &pipe_busy = L.pipe_busy = 0, &block_paths = L.block_paths = 0, &grid = L.grid = 0;
    if (f.piped) {
        const bool fed = f.fed, busy = f.busy;
        wgwf_shape(c, L, !fed, fed, 1, busy, block_paths, grid);
        // (an overlapped slot's path state holds either of a single frame's two shapes -- issued to an idle or to a busy device: growing it later would free memory, and
        //  freeing waits for the device)
        size_t slot_state_entries = (size_t)grid * block_paths;
        if (!fed) { int b2 = 0, g2 = 0; wgwf_shape(c, L, true, false, 1, !busy, b2, g2); slot_state_entries = std::max(slot_state_entries, (size_t)g2 * b2); }
        const size_t per_slot = (fed ? 0 : (size_t)kWfStatePlanes * slot_state_entries * sizeof(float4)) + (size_t)grid * kWgQueueF4 * sizeof(float4) + (fed ? 0 : frame_bytes);
        unsigned allowed = (unsigned)std::min<size_t>(c->pipe_slots, frames_budget(c) / std::max<size_t>(per_slot, 1));
        if (fed) allowed = std::min(allowed, kFedSlots);
        c->st.pipe_slots = (int32_t)allowed;
        if (allowed >= 1) {
            unsigned pick = c->pipe_next % allowed;
            for (unsigned k = 0; k < allowed; k++) {
                glrtx_ctx::PipeSlot &o = c->pipe[(c->pipe_next + k) % allowed];
                if (!o.used || hipEventQuery(o.acc_done) == hipSuccess) { pick = (c->pipe_next + k) % allowed; break; }
            }
            (void)hipGetLastError();
            c->pipe_next = pick + 1;
            slot = &c->pipe[pick];
            for (unsigned k = 0; k < kPipeSlots; k++)
                if (k != pick && c->pipe[k].used && hipEventQuery(c->pipe[k].render_done) == hipErrorNotReady) pipe_busy++;
            (void)hipGetLastError();
            if (c->pipe_share > 1 && pipe_busy > 0 && !fed) wgwf_shape(c, L, true, false, c->pipe_share, busy, block_paths, grid);  // (GLRTX_PIPE_SHARE: the round-3 form, A/B only)
            // the slot's buffers, before anything depends on them.  A fed launch's plane chunks hold a given number of bytes per frame: another size starts afresh
            // (the slot's last launch is waited for first: freeing memory waits for the device anyway)
            bool ok = true;
            // a fed launch writes the slot's feed block from the host: the slot's previous launch, which reads it, must have ended (with every fed slot busy the host
            // waits here: it is three launches ahead of the device)
            if (fed && slot->used) (void)hipEventSynchronize(slot->render_done);
            if (fed && slot->chunk_bytes != frame_bytes) {
                if (slot->used) (void)hipEventSynchronize(slot->acc_done);
                for (auto &ch : slot->chunks) dev_free(ch);
                std::memset(slot->feed_h->chunks, 0, sizeof slot->feed_h->chunks);
                slot->chunk_bytes = frame_bytes;
            }
            if (!fed) ok = ok && ensure(c, slot->state, (size_t)kWfStatePlanes * slot_state_entries * sizeof(float4)) == GLRTX_OK;
            ok = ok && ensure(c, slot->queues, (size_t)grid * kWgQueueF4 * sizeof(float4)) == GLRTX_OK;
            if (fed) ok = ok && ensure(c, slot->feed_d, sizeof(FeedDev)) == GLRTX_OK && feed_ensure_chunks(c, *slot, 0, n_frames, f.fed_cap, frame_bytes) == GLRTX_OK;
            else ok = ok && ensure(c, slot->planes, frame_bytes) == GLRTX_OK;
            if (!ok) {
                (void)hipGetLastError();
                c->err.clear();
                if (slot->used) (void)hipEventSynchronize(slot->acc_done);
                // memory is what ran out: this slot and the ones behind it give theirs back (they would never be picked again: pipe_slots shrinks to `pick`)
                for (unsigned k = pick; k < kPipeSlots; k++) {
                    glrtx_ctx::PipeSlot &o = c->pipe[k];
                    if (o.used) (void)hipEventSynchronize(o.acc_done);
                    dev_free(o.state); dev_free(o.planes); dev_free(o.queues); dev_free(o.feed_d);
                    for (auto &ch : o.chunks) dev_free(ch);
                    if (o.feed_h) std::memset(o.feed_h->chunks, 0, sizeof o.feed_h->chunks);
                    o.chunk_bytes = 0;
                    o.used = false;
                }
                (void)hipGetLastError();
                c->pipe_slots = pick;            // the slots in front of this one keep their buffers and stay in use
                if (pick == 0) c->pipeline = false;
                c->st.pipe_slots = (int32_t)pick;
                slot = nullptr;
                pipe_busy = 0;
            }
        }
        if (!slot) { f.piped = false; f.fed = false; }
    }
    if (!slot) {
        if (n_frames > frames_cap(c, L.p, 1)) return fail(c, GLRTX_ENOMEM, "glrtx_render_frames: %d frames exceed the frames-in-flight memory budget", n_frames);
        wgwf_shape(c, L, false, false, 1, f.busy, block_paths, grid);
    }
    if (slot) c->st.pipe_resident_max = std::max<int32_t>(c->st.pipe_resident_max, pipe_busy + 1);
    return GLRTX_OK;
}

// ---- the buffers the kernel runs on, and its arguments
int wgwf_args(glrtx_ctx *c, WgwfLaunch &L) {
    const glrtx_params *p = L.p;
    glrtx_ctx::PipeSlot *const slot = L.slot;
    const bool fed = L.f.fed, adapt = L.k.adapt, moments = L.req.kind == RenderReq::Moments || L.req.kind == RenderReq::Cascades;
    const int n_frames = L.n_frames, grid = L.grid;
    int rc;
    // A fed launch runs on its slot's stream and queues but on the CONTEXT's path state, like a plain launch: the same launch is 0.8 % faster there than on a slot's state
    // buffer (same-context A/B, two boxes, profiles/r06_ab_feed_cadence.txt -- where a 0.8-GB buffer lands physically decides what its stream of stores costs:
    // profiles/r04_context_regimes.txt).  Launches that share that buffer run one after the other (state_done in wgwf_issue): fed launches end all their workgroups together,
    // so there was nothing for them to overlap with anyway.
    L.ctx_state = !slot || fed;
    L.stateBuf = L.ctx_state ? &c->wfState : &slot->state;
    L.queueBuf = slot ? &slot->queues : &c->wfQ;
    L.planeBuf = slot ? &slot->planes : &c->wfPlanes;
    L.workPtr = (unsigned *)(slot ? slot->work.p : c->work.p);
    L.rstream = slot ? slot->stream : c->stream;  // the render kernel's stream
    // path state: two sets of six planes, an entry per workgroup of THIS launch and path-queue position (WfArgs::state): 0.8 GB for a full grid with kWgPathsMax paths
    // each, kilobytes for a small image (it used to be sized for the largest launch the device can hold, whatever the launch)
    L.state_entries = (size_t)grid * (size_t)L.block_paths;
    L.state_bytes = (size_t)kWfStatePlanes * L.state_entries * sizeof(float4);
    if ((rc = ensure(c, *L.stateBuf, L.state_bytes))) return rc;
    if ((rc = ensure(c, *L.queueBuf, (size_t)grid * kWgQueueF4 * sizeof(float4)))) return rc;  // per-workgroup queues
    WfArgs &w = L.w;
    std::memset(&w, 0, sizeof w);
    w.state = (float4 *)L.stateBuf->p;
    w.ids = L.state_entries;  // (the plane stride)
    c->st.wf_state_mib = (int32_t)((L.state_bytes + ((size_t)1 << 20) - 1) >> 20);
    w.total = (int)L.total;
    w.tiles8_x = L.tiles8_x;
    w.refill_min = kRefillMin;
    if (const char *v = std::getenv("GLRTX_REFILL_MIN")) w.refill_min = std::max(1, std::min(64, std::atoi(v)));
    w.n_frames = fed ? std::max(L.f.fed_cap, 2) : n_frames;  // (fed: the most frames the launch can take -- and > 1, so that path ids are split into frame and pixel)
    w.tiles_per_frame = (int)(L.total >> 6);
    if (fed) {
        FeedHost *fh = slot->feed_h;
        for (int i = 0; i < n_frames; i++) fh->seeds[i] = make_float2(L.seeds_xy[2 * i], L.seeds_xy[2 * i + 1]);
        __atomic_store_n(&fh->frames_pub, (unsigned)n_frames, __ATOMIC_RELEASE);
        w.feed_host = slot->feed_h_dev;
        w.feed_dev = (FeedDev *)slot->feed_d.p;
        w.feed_plane_f4 = L.plane_f4;
        w.feed_margin = 64 * 4 * grid;  // where guided self-scheduling starts to taper the helpings (gss_div x 64 tiles)
        if (const char *v = std::getenv("GLRTX_FEED_MARGIN")) w.feed_margin = std::max(0, std::atoi(v));
    } else {
        if (n_frames > 1) {
            if ((rc = ensure(c, c->wfSeeds, (size_t)n_frames * sizeof(float2)))) return rc;
            HIP_TRY(c, hipMemcpyAsync(c->wfSeeds.p, L.seeds_xy, (size_t)n_frames * sizeof(float2), hipMemcpyHostToDevice, c->stream));
            w.seeds = (const float2 *)c->wfSeeds.p;
            w.seeds_in_lds = n_frames <= kLdsSeeds ? 1 : 0;
        }
        if (n_frames > 1 || slot || adapt || moments) {
            if ((rc = ensure(c, *L.planeBuf, (size_t)std::max(L.n_planes, 1) * L.plane_f4 * sizeof(float4)))) return rc;
            w.planes = (float4 *)L.planeBuf->p;
        }
    }
    w.block_paths = L.block_paths;
    w.gss_div = (slot && !fed) ? 0 : 4 * grid;  // (overlapped single-frame launches: no guided self-scheduling, see wgwf_shape)
    if (const char *v = std::getenv("GLRTX_GSS_DIV")) w.gss_div = std::max(0, std::atoi(v));
    w.suspend_max = kSuspendMax;
    if (const char *v = std::getenv("GLRTX_SUSPEND_MAX")) w.suspend_max = std::max(0, std::min(64, std::atoi(v)));
    // trip guards (pt_render_wgwf): a path is alive for at most n_samples x (max_depth + 2) shaded trips; 64 times that (parked trips, the other paths' rounds) and a
    // constant are allowed between two tiles a workgroup is given
    w.trip_limit = (int)std::min<long long>(INT32_MAX, 64ll * std::max(p->n_samples, 1) * (p->max_depth + 2) + 64);
    // The V form: a bounce through a medium takes up to nine shaded trips instead of one -- the media hit that queues trial 1, then trials 1 .. 8, the last of which
    // queues the exit ray (the next bounce's path ray) -- and every such bounce ends the sample or advances the depth.  So a sample is alive for at most
    // 9 x (max_depth + 2) shaded trips, and the bound is nine times the plain one: 64 x n_samples x 9 x (max_depth + 2) + 64.
    if (L.k.vol) w.trip_limit = (int)std::min<long long>(INT32_MAX, 64ll * std::max(p->n_samples, 1) * 9 * (p->max_depth + 2) + 64);
    if (const char *v = std::getenv("GLRTX_TRIP_LIMIT")) w.trip_limit = std::max(1, std::atoi(v));
    w.err = c->guard_dev;
    return GLRTX_OK;
}

// ---- shape invariants of the hand-written kernel, checked on the host before every launch (an access past one of these
// buffers is a GPU memory fault, not an error code): every path id the launch can form indexes inside the state arrays;
// every workgroup of the grid has its own queue slice; a slice holds both halves of the double-buffered ray queue
// (2 rays per live path: the next ray and the shadow ray) and of the path-id queue; every (frame, sample) has its plane.
int wgwf_check(glrtx_ctx *c, const WgwfLaunch &L, const Route &route) {
    const glrtx_params *p = L.p;
    const glrtx_ctx::PipeSlot *const slot = L.slot;
    const WfArgs &w = L.w;
    const bool fed = L.f.fed, moments = L.req.folds_moments();
    const int n_frames = L.n_frames, grid = L.grid, block_paths = L.block_paths, fed_cap = L.f.fed_cap;
    const size_t state_entries = L.state_entries, total = L.total, max_id = L.ids - 1;
    const size_t max_sidx = (size_t)kWfSetPlanes * state_entries + (size_t)grid * block_paths - 1;  // the highest state index a ray record can carry (set 1)
    const size_t slice_f4 = 2 * (size_t)2 * 2 * block_paths /* ray records */ + (2 * (size_t)block_paths * sizeof(unsigned) + 15) / 16 /* path ids [2] */;
    static_assert(kWgSuspendAt + (size_t)kSuspendF4 * kBlockThreads == kWgQueueF4, "the suspend area closes a workgroup's slice");
    bool ok = slice_f4 <= kWgSuspendAt && max_id < (size_t)WF_INVALID && 2 * max_sidx + 1 < (size_t)WF_INVALID && (size_t)grid * block_paths <= state_entries &&
              (size_t)kWfStatePlanes * state_entries * sizeof(float4) < ((size_t)1 << 32) && (block_paths & (block_paths - 1)) == 0 && block_paths >= 256 &&
              block_paths <= kWgPathsMax && slice_f4 <= kWgQueueF4 && L.queueBuf->bytes >= (size_t)grid * kWgQueueF4 * sizeof(float4) &&
              L.stateBuf->bytes >= L.state_bytes && w.ids == state_entries && grid >= 1 && (size_t)grid <= L.k.wg_slots &&
              p->max_depth <= kWfDepthMax && p->n_samples <= kWfSampleMax && L.workPtr != nullptr;
    // the kernel that was picked serves the route's form (what may be bound beside a form is the route's business), and what that form reads is there
    ok = ok && route.family == glrt_detail::kRouteWavefront && L.k.vol == route.vol && L.k.tex == route.tex && L.k.maps == route.maps && L.k.vine == route.vine;
    if (route.vol) ok = ok && p->n_samples <= kWfVolSampleMax && c->vol.density != nullptr && c->vol.temperature != nullptr && !L.k.vine && L.k.fetch == 0 && !L.k.compact;
    if (route.tex) ok = ok && !L.k.vine && !route.vol && L.k.fetch != 2 && c->texDesc.p != nullptr && c->texTexels.p != nullptr && c->texSt.p != nullptr &&
                        c->texBind.p != nullptr && (!route.maps || c->texMaps.p != nullptr) && L.a.hit_hist == nullptr;
    if (!fed && n_frames > 1) ok = ok && c->wfSeeds.bytes >= (size_t)n_frames * sizeof(float2);
    if (w.planes) ok = ok && L.planeBuf->bytes >= (size_t)std::max(L.n_planes, 1) * L.plane_f4 * sizeof(float4);
    if (L.k.adapt) ok = ok && !fed && !slot && w.planes && c->ad_selected && c->ad_tiles == (int)(total >> 6) && c->adList.bytes >= (total >> 6) * sizeof(int) &&
                        c->adMask.bytes >= (total >> 6);
    const size_t acc_bytes = c->pitch_bytes * (size_t)c->owned_rows;
    if (L.req.kind == RenderReq::Adaptive) ok = ok && c->adHalf.current(accum_shape(c)) && c->adHalf.buf.bytes >= acc_bytes;
    if (moments) ok = ok && !fed && !slot && w.planes && c->mmM.current(accum_shape(c)) && c->mmM.buf.bytes >= acc_bytes;
    if (L.req.kind == RenderReq::Cascades) ok = ok && !fed && !slot && w.planes && c->rwC.current(accum_shape(c)) &&
                                                 c->rwC.buf.bytes >= (size_t)reweight::kCascades * acc_bytes;
    if (fed) ok = ok && n_frames >= 1 && n_frames <= fed_cap && fed_cap <= kFeedMaxFrames && slot->feed_d.bytes >= sizeof(FeedDev) && w.feed_host != nullptr &&
                  slot->chunks[(n_frames - 1) / kFeedChunkFrames].p != nullptr && slot->chunk_bytes == L.frame_bytes;
    if (!ok) return fail(c, GLRTX_EDEVICE, "internal: wgwf launch shapes inconsistent (ids %zu, max id %zu, grid %d of %zu slots (%d per CU), block_paths %d, frames %d, fed %d)", L.ids, max_id,
                         grid, L.k.wg_slots, L.k.per_cu, block_paths, n_frames, (int)fed);
    return GLRTX_OK;
}

// The accumulation pass of one (source, sink) pair on the context's stream (accumulate.hip.h).
template <class Src, class Sink>
void accumulate_launch(glrtx_ctx *c, const accumulate::Image &im, const Src &src, const Sink &sink) {
    hipLaunchKernelGGL(accumulate::entry(src, sink), dim3((im.width + 63) / 64, (im.rows + 3) / 4), dim3(256), 0, c->stream, im, src, sink);
}

// ---- issue: the render kernel on its stream, the accumulation pass (and the images) on the context's, the events that order and time them
int wgwf_issue(glrtx_ctx *c, const WgwfLaunch &L) {
    const glrtx_params *p = L.p;
    glrtx_ctx::PipeSlot *const slot = L.slot;
    const WfArgs &w = L.w;
    const bool fed = L.f.fed, adapt = L.k.adapt, vol = L.k.vol;
    const int n_frames = L.n_frames, n_planes = L.n_planes;
    const hipStream_t rstream = L.rstream;
    glrtx_ctx::LaunchRec *rec = nullptr;
    int rc;
    if ((rc = next_launch_rec(c, rec))) return rc;
    // a slot's render kernel overwrites the planes its previous plane-accumulation pass (two launches ago, on the context's stream) reads
    if (slot && slot->used) HIP_TRY(c, hipStreamWaitEvent(rstream, slot->acc_done, 0));
    // ... and a kernel on the context's path state starts behind the last one that used it (another stream's, possibly)
    if (L.ctx_state && c->state_used) HIP_TRY(c, hipStreamWaitEvent(rstream, c->state_done, 0));
    HIP_TRY(c, hipMemsetAsync(L.workPtr, 0, sizeof(unsigned), rstream));
    if (fed) {  // the device mirror starts with the frames published so far (kernel boundary: visible to every workgroup of the render kernel)
        hipLaunchKernelGGL(feed_prefill_kernel, dim3(1), dim3(64), 0, rstream, (FeedDev *)slot->feed_d.p, (const FeedHost *)slot->feed_h_dev, n_frames);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(rec->ev0, rstream));
    c->last_kernel = L.k.name;
    c->counters_stale = c->counters_stale || L.req.count_rays(c);
    const VolArgs va = vol ? c->vol : VolArgs{};
    const TexSet ts = L.k.tex ? tex_set(c) : TexSet{};
    hipLaunchKernelGGL(L.k.fn, dim3(L.grid), dim3(kBlockThreads), L.k.lds, rstream, L.a, w, L.workPtr, (float4 *)L.queueBuf->p, adapt ? (const int *)c->adList.p : nullptr,
                       adapt ? (const unsigned *)c->adCount.p : nullptr, va, ts);
    HIP_TRY(c, hipGetLastError());
#ifdef GLRTX_RAY_LOG
    g_dbg_last = {L.a, w, L.k.lds, L.grid, (float4 *)L.queueBuf->p, L.k.fetch};
#endif
    HIP_TRY(c, hipEventRecord(rec->evm, rstream));
    if (L.ctx_state) { HIP_TRY(c, hipEventRecord(c->state_done, rstream)); c->state_used = true; }
    if (slot) {  // the context's stream -- where the caller's own work, the resolve pass and the next accumulation are ordered -- takes over
        HIP_TRY(c, hipEventRecord(slot->render_done, rstream));
        HIP_TRY(c, hipStreamWaitEvent(c->stream, slot->render_done, 0));
        HIP_TRY(c, hipEventRecord(rec->eva, c->stream));  // (the interval evm..ev1 would include the wait for the passes queued before this one)
    }
    rec->has_eva = slot != nullptr;
    // presenting: the pass that adds the planes also resolves every frame into its device image (fed: however many frames the launch ends up with -- each was given an
    // image when it was appended); a launch without planes accumulated in the render kernel and is resolved behind it (below)
    const bool pres = L.req.presents(c);
    const bool pres_fused = pres && (fed || w.planes);
    if (pres_fused && (rc = present_pass_begin(c))) return rc;
    {
        // the source follows the form, the sink the request
        const accumulate::Image im{L.a.accum, L.a.pitch_f4, c->width, c->owned_rows};
        const accumulate::Planes flat{(const float4 *)L.planeBuf->p, n_frames, p->n_samples};
        const accumulate::Fed feed{fed ? (const FeedDev *)slot->feed_d.p : nullptr, p->n_samples};
        const glrtx_ctx::Present &P = c->pres;
        const accumulate::Present ring{(uchar4 *)P.dev.p, (size_t)c->width * (size_t)c->owned_rows, P.ring, pres ? (int)(P.seq % (uint64_t)P.ring) : 0, P.inv_gamma, P.flip};
        if (L.req.kind == RenderReq::AdaptiveMoments) {
            if (n_planes > 0) accumulate_launch(c, im, flat, accumulate::MomentsMasked{(float4 *)c->mmM.buf.p, (const unsigned char *)c->adMask.p, L.tiles8_x});
        } else if (adapt) accumulate_launch(c, im, flat, accumulate::Half{(float4 *)c->adHalf.buf.p, (const unsigned char *)c->adMask.p, L.tiles8_x});
        else if (L.req.kind == RenderReq::Moments) { if (n_planes > 0) accumulate_launch(c, im, flat, accumulate::Moments{(float4 *)c->mmM.buf.p}); }
        else if (L.req.kind == RenderReq::Cascades) {
            if (n_planes > 0) accumulate_launch(c, im, flat, accumulate::Cascades{(float4 *)c->rwC.buf.p, (size_t)L.a.pitch_f4 * (size_t)c->owned_rows, c->rw_start});
        }
        else if (fed && pres) accumulate_launch(c, im, feed, ring);
        else if (fed) accumulate_launch(c, im, feed, accumulate::None{});
        else if (w.planes && pres) accumulate_launch(c, im, flat, ring);
        else if (w.planes && n_planes > 0) accumulate_launch(c, im, flat, accumulate::None{});
        HIP_TRY(c, hipGetLastError());
    }
    if (pres_fused && (rc = present_pass_end(c, n_frames))) return rc;
    if (slot) { HIP_TRY(c, hipEventRecord(slot->acc_done, c->stream)); slot->used = true; }
    HIP_TRY(c, hipEventRecord(rec->ev1, c->stream));
    rec->kernel = c->last_kernel; rec->frames = n_frames;
    c->ring_head++;
    c->st.frames_last = n_frames;
    c->st.paths += (uint64_t)c->owned_rows * (uint64_t)c->width * (uint64_t)p->n_samples * (uint64_t)n_frames;
    // what the next call may build on
    c->last_render_done = slot ? slot->render_done : c->state_done;  // (a plain launch runs on the context's path state: ctx_state)
    if (fed) {
        c->open.slot = slot; c->open.p = *p; c->open.frames = n_frames; c->open.cap = L.f.fed_cap; c->open.rec = rec; c->open.frame_bytes = L.frame_bytes; c->open.vol = vol;
        c->st.feed_launches++;
    } else c->open.slot = nullptr;
    if (pres && !pres_fused) return present_resolve(c);
    return GLRTX_OK;
}

int launch_wgwf(glrtx_ctx *c, const KernelArgs &a, const glrtx_params *p, const RenderReq &req, const Route &route) {
    WgwfLaunch L{};
    L.p = p; L.req = req; L.a = a; L.n_frames = req.n_frames;
    L.seeds_xy = req.n_frames == 1 ? p->seed : req.seeds;
    L.tiles8_x = (c->width + 7) / 8;
    L.total = (size_t)L.tiles8_x * ((c->owned_rows + 7) / 8) * 64;
    if (L.total * 2 >= (size_t)INT32_MAX) return fail(c, GLRTX_EINVAL, "image too large for the wgwf variant");
    L.plane_f4 = (size_t)a.pitch_f4 * (size_t)c->owned_rows;
    L.plane_bytes = L.plane_f4 * sizeof(float4);
    L.frame_bytes = (size_t)std::max(p->n_samples, 1) * L.plane_bytes;
    L.n_planes = L.n_frames * p->n_samples;
    L.f = wgwf_form(c, L);
    L.ids = L.total * (size_t)(L.f.fed ? L.f.fed_cap : L.n_frames);  // path id = frame * total + pixel
    if (L.ids + 1 >= (size_t)UINT32_MAX) return fail(c, GLRTX_EINVAL, "glrtx_render_frames: %d frames of %zu pixels exceed the 32-bit ray id space", L.n_frames, L.total);
    if (int rc = wgwf_kernel(c, L, route)) return rc;
    if (int rc = wgwf_pipe_slot(c, L)) return rc;
    if (int rc = wgwf_args(c, L)) return rc;
    if (int rc = wgwf_check(c, L, route)) return rc;
    return wgwf_issue(c, L);
}


// ---- denoising (glrtx_render_features, glrtx_denoise)
void denoise_release(glrtx_ctx *c) {
    c->ftN.drop(); dev_free(c->ftA); dev_free(c->ftCounter); dev_free(c->dnP[0]); dev_free(c->dnP[1]); c->dnD.drop();
    dev_free(c->ftN_spare); dev_free(c->ftA_spare); dev_free(c->accum_spare); dev_free(c->rpCount);  // (glrtx_reproject's spares have the old shape too)
    c->rp_have = false;
    dev_free(c->ftG); dev_free(c->ftG_spare);
    c->mt_g_have = false;
    for (DevBuf &v : c->dnV) dev_free(v);
}

// The two filters' configurations as one: glrtx_denoise_cfg and glrtx_denoise_var_cfg differ in the name of the colour term's sigma.
struct FilterCfg { int iterations; float sigma_c, sigma_normal, sigma_depth; int demodulate; };
FilterCfg filter_cfg(const glrtx_denoise_cfg &k) { return {k.iterations, k.sigma_color, k.sigma_normal, k.sigma_depth, k.demodulate}; }
FilterCfg filter_cfg(const glrtx_denoise_var_cfg &k) { return {k.iterations, k.sigma_lum, k.sigma_normal, k.sigma_depth, k.demodulate}; }

template <class Cfg>
int denoise_cfg_check(glrtx_ctx *c, const Cfg *cfg, const char *fn, FilterCfg &k) {
    if (!cfg) return fail(c, GLRTX_EINVAL, "%s: NULL cfg", fn);
    k = filter_cfg(*cfg);
    if (k.iterations < 1 || k.iterations > 6) return fail(c, GLRTX_EINVAL, "%s: iterations %d outside 1..6", fn, k.iterations);
    const float sg[3] = {k.sigma_c, k.sigma_normal, k.sigma_depth};
    for (float v : sg)
        if (!(v > 0.0f) || std::isinf(v)) return fail(c, GLRTX_EINVAL, "%s: sigma %g is not a positive finite number", fn, (double)v);
    return GLRTX_OK;
}

// The filter's passes on `stream`: accum (pitch_f4) + the two feature planes -> D, through the ping-pong images p0 / p1 (all but accum packed rows of `width`).
// With `moments` (pitch_f4) and the variance planes v[0] (V0), v[1], v[2] (packed floats) the variance pass runs first and the iterations are the
// variance-guided ones; without them (both null) they are the plain ones.
int denoise_passes(glrtx_ctx *c, hipStream_t stream, const float4 *accum, const float4 *moments, int pitch_f4, const float4 *guide, const float4 *albedo, float4 *p0,
                   float4 *p1, float4 *D, float *const *v, int width, int rows, const FilterCfg &k) {
    const dim3 grid((unsigned)(((width + denoise::kTileDn - 1) / denoise::kTileDn) * ((rows + denoise::kTileDn - 1) / denoise::kTileDn)));
    const int demod = k.demodulate ? 1 : 0;
    const bool var = moments != nullptr;
    if (var) {
        variance::Args va;
        va.accum = accum; va.moments = moments; va.guide = guide; va.albedo = albedo; va.v0 = v[0];
        va.pitch_f4 = pitch_f4; va.width = width; va.rows = rows;
        va.sigma_normal = k.sigma_normal; va.sigma_depth = k.sigma_depth; va.demodulate = demod;
        hipLaunchKernelGGL(variance::variance_estimate, grid, dim3(256), 0, stream, va);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(denoise::denoise_prep, grid, dim3(256), 0, stream, accum, pitch_f4, albedo, p0, width, rows, demod);
    HIP_TRY(c, hipGetLastError());
    using Kernel = void (*)(const denoise::Args);
    static const Kernel kernels[2][3][2] = {  // [variance-guided][iteration 0, 1, 2 and later: S = 1, 2, 0][last]
        {{denoise::denoise_atrous<1, false>, denoise::denoise_atrous<1, true>},
         {denoise::denoise_atrous<2, false>, denoise::denoise_atrous<2, true>},
         {denoise::denoise_atrous<0, false>, denoise::denoise_atrous<0, true>}},
        {{denoise::denoise_atrous_var<1, false>, denoise::denoise_atrous_var<1, true>},
         {denoise::denoise_atrous_var<2, false>, denoise::denoise_atrous_var<2, true>},
         {denoise::denoise_atrous_var<0, false>, denoise::denoise_atrous_var<0, true>}}};
    float4 *img[2] = {p0, p1};
    for (int it = 0; it < k.iterations; it++) {
        const bool last = it == k.iterations - 1;
        denoise::Args a{};
        a.src = img[it & 1]; a.guide = guide; a.albedo = albedo; a.dst = last ? D : img[(it + 1) & 1];
        a.width = width; a.rows = rows; a.spacing = 1 << it;
        if (var) {
            a.vsrc = it == 0 ? v[0] : v[1 + ((it - 1) & 1)]; a.vdst = v[1 + (it & 1)];
            a.sigma_c = k.sigma_c;
        } else {
            uint32_t pw = (uint32_t)(127 - 2 * it) << 23;  // 4^-it
            float scale;
            std::memcpy(&scale, &pw, 4);
            float sc = k.sigma_c * scale;
            uint32_t scb;
            std::memcpy(&scb, &sc, 4);
            if ((scb & 0x7F800000u) == 0u) sc = 0.0f;  // (a denormal: the device would read it as zero)
            a.sigma_c = sc;
        }
        a.sigma_normal = k.sigma_normal; a.sigma_depth = k.sigma_depth;
        a.demodulate = demod;
        hipLaunchKernelGGL(kernels[var][std::min(it, 2)][last], grid, dim3(256), 0, stream, a);
        HIP_TRY(c, hipGetLastError());
    }
    return GLRTX_OK;
}

// The debug entry points' device buffers: a handful of allocations, freed on scope exit, and the first HIP error of the sequence -- every step after it is
// skipped, and result() reports it.
struct DebugScratch {
    std::vector<void *> bufs;
    hipError_t e = hipSuccess;
    ~DebugScratch() {
        for (void *q : bufs) (void)hipFree(q);
    }
    bool ok() const { return e == hipSuccess; }
    template <class T = float4>
    T *alloc(size_t bytes, const void *upload = nullptr) {
        void *q = nullptr;
        if (ok() && (e = hipMalloc(&q, bytes)) == hipSuccess) bufs.push_back(q);
        if (ok() && upload) e = hipMemcpy(q, upload, bytes, hipMemcpyHostToDevice);
        return (T *)q;
    }
    void sync() {
        if (ok()) e = hipDeviceSynchronize();
    }
    void download(void *to, const void *from, size_t bytes) {
        if (ok() && to) e = hipMemcpy(to, from, bytes, hipMemcpyDeviceToHost);
    }
    int result(int rc, const char *fn) const { return ok() ? rc : fail(nullptr, GLRTX_EDEVICE, "%s: %s", fn, hipGetErrorString(e)); }
};


// ---- reprojection (glrtx_reproject, glrtx_reproject_motion): the launches
// What the two kernels share (reproject::Common): the old view (accumulator of pitch_f4, planes N0 / A0), the new view's x1 (N1, or G1 for the motion kernel) and A1 -> `out` (pitch_f4); with mom /
// mom_out the moments plane rides the same taps.  `counts`: reproject::kCountBytes.
reproject::Common reproject_common(const glrt_detail::ReprojectSetup &st, const float4 *acc, const float4 *n0, const float4 *a0, const float4 *x1, const float4 *a1, float4 *out,
                                   int pitch_f4, int width, int rows, void *counts, const float4 *mom, float4 *mom_out) {
    reproject::Common a{};
    std::memcpy(a.W, st.W, sizeof a.W);
    std::memcpy(a.S, st.S, sizeof a.S);
    a.opx = st.o_prev[0]; a.opy = st.o_prev[1]; a.opz = st.o_prev[2];
    a.acc = acc; a.n0 = n0; a.a0 = a0; a.x1 = x1; a.a1 = a1; a.out = out;
    a.pitch_f4 = pitch_f4; a.width = width; a.rows = rows;
    a.tiles_x = (width + 7) / 8;
    a.n_tiles = a.tiles_x * ((rows + 7) / 8);
    a.max_history = st.max_history; a.depth_tol = st.depth_tolerance; a.normal_tol = st.normal_tolerance;
    a.counts = (unsigned long long *)counts;
    a.mom = mom; a.mom_out = mom_out;
    return a;
}

// Either kernel on `stream`, its counters zeroed first.
template <class A>
int reproject_launch(glrtx_ctx *c, hipStream_t stream, void (*kernel)(const A), const A &a) {
    HIP_TRY(c, hipMemsetAsync(a.c.counts, 0, reproject::kCountBytes, stream));
    hipLaunchKernelGGL(kernel, dim3((unsigned)((a.c.n_tiles + 3) / 4)), dim3(256), 0, stream, a);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}

// The static kernel (common.x1: N1): the new view's camera.
int reproject_pass(glrtx_ctx *c, hipStream_t stream, const reproject::Common &common, const float *c2w_cur, const float *s2c_cur, int stripe) {
    reproject::Args a{};
    a.c = common;
    std::memcpy(a.cam.cam, c2w_cur, 16 * sizeof(float));
    std::memcpy(a.cam.cam + 16, s2c_cur, 16 * sizeof(float));
    a.cam.width = common.width; a.cam.height = common.rows;
    a.cam.owned_rows = common.rows; a.cam.rank = 0; a.cam.world = 1; a.cam.stripe = stripe;
    return reproject_launch(c, stream, reproject::reproject_kernel, a);
}

// The motion-aware kernel (reproject_motion.hip.h; common.x1: G1): the previous geometry (prev_pos / prev_nrm: motion::Args').
int reproject_motion_pass(glrtx_ctx *c, hipStream_t stream, const reproject::Common &common, const float4 *prev_pos, const float4 *prev_nrm, int n_tri) {
    motion::Args a{};
    a.c = common; a.prev_pos = prev_pos; a.prev_nrm = prev_nrm; a.n_tri = n_tri;
    return reproject_launch(c, stream, motion::reproject_motion_kernel, a);
}


// ---- adaptive sampling (glrtx_render_adaptive)
// Everything glrtx_render_adaptive refuses, checked before anything changes.  The megakernels have no tile list and the present ring no adaptive form.
int adapt_check(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg) {
    const char *fn = "glrtx_render_adaptive";
    if (!p || !cfg) return fail(c, GLRTX_EINVAL, "%s: NULL params or cfg", fn);
    if (cfg->min_samples < 2) return fail(c, GLRTX_EINVAL, "%s: min_samples %d < 2 (the half buffer needs two samples)", fn, cfg->min_samples);
    if (n_frames < 0 || (n_frames > 0 && !seeds_xy)) return fail(c, GLRTX_EINVAL, "%s: bad seeds/n_frames", fn);
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (p->n_samples < 0 || p->max_depth < 0) return fail(c, GLRTX_EINVAL, "%s: negative n_samples/max_depth", fn);
    if (c->pres.ring > 0) return fail(c, GLRTX_EINVAL, "%s: presentation is enabled (the present ring has no adaptive form)", fn);
    return route_refusal(c, route_of(c, p, RenderReq::Adaptive), fn);  // what only the wavefront kernel can do: it has the tile list
}

// The selection, on the context's stream behind everything issued before: mask, ascending list and count of the active tiles.  from_moments
// (glrtx_render_adaptive_moments): from M, which the caller has made sure of, by adaptive_moments::select_kernel; H is neither read nor allocated.
int adapt_select(glrtx_ctx *c, const glrtx_adaptive *cfg, bool from_moments) {
    const int tiles8_x = (c->width + 7) / 8, tiles8_y = (c->owned_rows + 7) / 8, n_tiles = tiles8_x * tiles8_y;
    if (!from_moments && c->owned_rows > 0 && !c->adHalf.current(accum_shape(c)))
        if (int rc = plane_zero(c, c->adHalf)) return rc;  // (first adaptive use, or the accumulator's pitch or rows have changed)
    int rc;
    if ((rc = ensure(c, c->adMask, (size_t)n_tiles)) || (rc = ensure(c, c->adList, (size_t)n_tiles * sizeof(int))) || (rc = ensure(c, c->adCount, sizeof(unsigned))))
        return rc;
    c->ad_tiles = n_tiles; c->ad_tiles_x = tiles8_x;
    c->ad_selected = true;
    if (n_tiles == 0) { HIP_TRY(c, hipMemsetAsync(c->adCount.p, 0, sizeof(unsigned), c->stream)); return GLRTX_OK; }
    const int pitch_f4 = (int)(c->pitch_bytes / sizeof(float4));
    if (from_moments)
        hipLaunchKernelGGL(adaptive_moments::select_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, c->stream, (const float4 *)c->mmM.buf.p, pitch_f4, c->width,
                           c->owned_rows, tiles8_x, n_tiles, cfg->threshold, cfg->min_samples, (unsigned char *)c->adMask.p, (float *)nullptr);
    else
        hipLaunchKernelGGL(adaptive_select_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, c->stream, (const float4 *)c->accum, (const float4 *)c->adHalf.buf.p, pitch_f4, c->width,
                           c->owned_rows, tiles8_x, n_tiles, cfg->threshold, cfg->min_samples, (unsigned char *)c->adMask.p, (float *)nullptr);
    HIP_TRY(c, hipGetLastError());
    hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(kAdaptCompactThreads), 0, c->stream, (const unsigned char *)c->adMask.p, n_tiles, (int *)c->adList.p,
                       (unsigned *)c->adCount.p);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}

// ---- variance guidance (glrtx_track_moments, glrtx_render_moments, glrtx_denoise_variance)
// Everything a render call that folds its planes into a side plane refuses (glrtx_render_moments, glrtx_render_cascades), checked before anything changes:
// glrtx_render_adaptive's list, the volume and the plane's tracking being off (`tracked`; `untracked` says so).
int side_plane_check(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, const char *fn, bool tracked, const char *untracked) {
    if (!p) return fail(c, GLRTX_EINVAL, "%s: NULL params", fn);
    if (!tracked) return fail(c, GLRTX_EINVAL, "%s: %s", fn, untracked);
    if (n_frames < 0 || (n_frames > 0 && !seeds_xy)) return fail(c, GLRTX_EINVAL, "%s: bad seeds/n_frames", fn);
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (p->n_samples < 0 || p->max_depth < 0) return fail(c, GLRTX_EINVAL, "%s: negative n_samples/max_depth", fn);
    if (c->pres.ring > 0) return fail(c, GLRTX_EINVAL, "%s: presentation is enabled (the present ring's passes fold neither moments nor cascades)", fn);
    return route_refusal(c, route_of(c, p, RenderReq::Moments), fn);  // what only the wavefront kernel can do: it writes the sample planes (one list for the three calls)
}

int moments_check(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, const char *fn = "glrtx_render_moments") {
    return side_plane_check(c, p, seeds_xy, n_frames, fn, c->mm_on, "moments are not tracked (glrtx_track_moments)");
}

// Everything glrtx_render_adaptive_moments refuses, checked before anything changes: glrtx_render_adaptive's list and glrtx_render_moments's (which holds all of the
// former's but the configuration, and the volume forms besides).
int adapt_moments_check(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg) {
    const char *fn = "glrtx_render_adaptive_moments";
    if (!p || !cfg) return fail(c, GLRTX_EINVAL, "%s: NULL params or cfg", fn);
    if (cfg->min_samples < 2) return fail(c, GLRTX_EINVAL, "%s: min_samples %d < 2 (one sample has no variance)", fn, cfg->min_samples);
    return moments_check(c, p, seeds_xy, n_frames, fn);
}

// ---- firefly re-weighting (glrtx_track_cascades, glrtx_render_cascades, glrtx_reweight)
bool cascade_start_ok(float s) { return s >= 0x1p-20f && s <= 0x1p20f; }  // (a NaN fails both)

int reweight_cfg_check(glrtx_ctx *c, const glrtx_reweight_cfg *k, const char *fn) {
    if (!k) return fail(c, GLRTX_EINVAL, "%s: NULL cfg", fn);
    if (!(k->kappa > 0.0f) || std::isinf(k->kappa)) return fail(c, GLRTX_EINVAL, "%s: kappa %g is not a positive finite number", fn, (double)k->kappa);
    return GLRTX_OK;
}

// The resolve on `stream`: the six planes (pitch_f4, `plane` float4 apart) -> D (packed rows of `width`).
int reweight_pass(glrtx_ctx *c, hipStream_t stream, const float4 *C, size_t plane, int pitch_f4, int width, int rows, float4 *D, const glrtx_reweight_cfg &k) {
    const reweight::Args a{C, plane, D, pitch_f4, width, rows, k.kappa};
    hipLaunchKernelGGL(reweight::reweight_kernel, reweight::reweight_grid(width, rows), dim3(256), 0, stream, a);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}

// ---- tone mapping (glrtx_exposure_measure, glrtx_tonemap, glrtx_resolve_tonemapped_rgba8)
static_assert(sizeof(tonemap::Exposure) == tonemap::kExposureOut + sizeof(glrtx_exposure), "tonemap::Exposure ends with glrtx_exposure's image");

bool tm_positive(float v) { return v > 0.0f && !std::isinf(v); }

// Everything a call that takes a glrtx_tonemap_cfg refuses about the cfg itself, checked before anything changes.
int tonemap_cfg_check(glrtx_ctx *c, const glrtx_tonemap_cfg *k, const char *fn) {
    if (!k) return fail(c, GLRTX_EINVAL, "%s: NULL cfg", fn);
    if (k->op < 0 || k->op > 2) return fail(c, GLRTX_EINVAL, "%s: op %d outside 0..2", fn, k->op);
    if (k->source < 0 || k->source > 1) return fail(c, GLRTX_EINVAL, "%s: source %d outside 0..1", fn, k->source);
    if (!tm_positive(k->exposure)) return fail(c, GLRTX_EINVAL, "%s: exposure %g is not a positive finite number", fn, (double)k->exposure);
    if (!tm_positive(k->key)) return fail(c, GLRTX_EINVAL, "%s: key %g is not a positive finite number", fn, (double)k->key);
    if (!tm_positive(k->white) || !std::isnormal(k->white * k->white))
        return fail(c, GLRTX_EINVAL, "%s: white %g is not a positive finite number with a normal square", fn, (double)k->white);
    if (!tm_positive(k->gamma)) return fail(c, GLRTX_EINVAL, "%s: gamma %g is not a positive finite number", fn, (double)k->gamma);
    if (!(k->adapt > 0.0f && k->adapt <= 1.0f)) return fail(c, GLRTX_EINVAL, "%s: adapt %g outside (0, 1]", fn, (double)k->adapt);
    if (k->low_permille < 0 || k->low_permille >= k->high_permille || k->high_permille > 1000)
        return fail(c, GLRTX_EINVAL, "%s: histogram window %d..%d is not 0 <= low < high <= 1000", fn, k->low_permille, k->high_permille);
    return GLRTX_OK;
}
tonemap::Curve tonemap_curve(const glrtx_tonemap_cfg &k) { return {k.op, k.auto_exposure ? 1 : 0, k.exposure, k.white}; }

// The context's exposure block, zeroed when it is first allocated (no E, an empty working histogram).
int exposure_ensure(glrtx_ctx *c) {
    if (c->tmExp.p) return GLRTX_OK;
    if (int rc = ensure(c, c->tmExp, sizeof(tonemap::Exposure))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->tmExp.p, 0, sizeof(tonemap::Exposure), c->stream));
    return GLRTX_OK;
}

// The HDR image a tone-mapping or bloom cfg names: 0 the accumulator, 1 the image D -- of the current shape, or the call is refused.
int hdr_source(glrtx_ctx *c, int source, const char *fn, const float4 *&src, int &pitch_f4) {
    if (source == 1) {
        if (!c->dnD.current(packed_shape(c)))
            return fail(c, GLRTX_EINVAL, "%s: source = 1 without a denoised image of the current shape (call glrtx_denoise or glrtx_denoise_variance first)", fn);
        src = (const float4 *)c->dnD.buf.p; pitch_f4 = c->width;
    } else {
        src = c->accum; pitch_f4 = (int)(c->pitch_bytes / sizeof(float4));
    }
    return GLRTX_OK;
}

// The context checks every tone-mapping call shares, and the source the cfg names.
int tonemap_source(glrtx_ctx *c, const glrtx_tonemap_cfg *k, const char *fn, const float4 *&src, int &pitch_f4) {
    if (int rc = tonemap_cfg_check(c, k, fn)) return rc;
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    return hdr_source(c, k->source, fn, src, pitch_f4);
}

// What the two tone-mapping calls that read B share: the cfg with its source unread, and B of the current shape.
int tonemap_bloomed_cfg(glrtx_ctx *c, const glrtx_tonemap_cfg *cfg, const char *fn, glrtx_tonemap_cfg &k) {
    if (!cfg) return fail(c, GLRTX_EINVAL, "%s: NULL cfg", fn);
    k = *cfg;
    k.source = 0;  // (not read: the source is B)
    if (int rc = tonemap_cfg_check(c, &k, fn)) return rc;
    if (!c->blB.current(packed_shape(c))) return fail(c, GLRTX_EINVAL, "%s: no bloomed plane (call glrtx_bloom first)", fn);
    return GLRTX_OK;
}

// One measurement on `stream`: the histogram into st->work, then the reduce.
int exposure_passes(glrtx_ctx *c, hipStream_t stream, const float4 *src, int pitch_f4, int width, int rows, tonemap::Exposure *st, const glrtx_tonemap_cfg &k) {
    if (rows > 0) {
        hipLaunchKernelGGL(tonemap::exposure_histogram, tonemap::histogram_grid(width, rows), dim3(256), 0, stream, src, pitch_f4, width, rows, st);
        HIP_TRY(c, hipGetLastError());
    }
    const tonemap::ReduceArgs ra{st, k.key, k.adapt, k.low_permille, k.high_permille};
    hipLaunchKernelGGL(tonemap::exposure_reduce, dim3(1), dim3(256), 0, stream, ra);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}
int tonemap_plane_pass(glrtx_ctx *c, hipStream_t stream, const float4 *src, int pitch_f4, int width, int rows, float4 *T, const tonemap::Exposure *st,
                       const glrtx_tonemap_cfg &k) {
    hipLaunchKernelGGL(tonemap::tonemap_plane, dim3((unsigned)((width + 63) / 64), (unsigned)((rows + 3) / 4)), dim3(256), 0, stream, src, pitch_f4, width, rows, T,
                       tonemap_curve(k), st);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}
int tonemap_resolve_pass(glrtx_ctx *c, hipStream_t stream, const float4 *src, int pitch_f4, int width, int rows, uchar4 *out, const tonemap::Exposure *st,
                         const glrtx_tonemap_cfg &k) {
    hipLaunchKernelGGL(tonemap::tonemap_resolve<kResolvePer>, resolve_grid(width, rows), dim3(256), 0, stream, src, pitch_f4, width, rows, out, width, 1.0f / k.gamma,
                       k.flip_y ? 1 : 0, tonemap_curve(k), st);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}

// ---- bloom (glrtx_bloom, glrtx_debug_bloom)
// The sizes of the levels 0 .. levels and where D_k (k >= 1) starts in the packed pyramid, in float4.
struct BloomLevels {
    int n, w[9], h[9];
    size_t at[10];  // at[k]: D_k's first texel; at[n + 1]: the pyramid's size
};
BloomLevels bloom_levels(int width, int rows, int levels) {
    BloomLevels L{};
    L.n = levels; L.w[0] = width; L.h[0] = rows;
    L.at[0] = L.at[1] = 0;
    for (int k = 1; k <= levels; k++) {
        L.w[k] = (L.w[k - 1] + 1) >> 1; L.h[k] = (L.h[k - 1] + 1) >> 1;
        L.at[k + 1] = L.at[k] + (size_t)L.w[k] * (size_t)L.h[k];
    }
    return L;
}

// Everything a call that takes a glrtx_bloom_cfg refuses about the cfg itself, checked before anything changes.
int bloom_cfg_check(glrtx_ctx *c, const glrtx_bloom_cfg *k, const char *fn) {
    if (!k) return fail(c, GLRTX_EINVAL, "%s: NULL cfg", fn);
    if (k->source < 0 || k->source > 1) return fail(c, GLRTX_EINVAL, "%s: source %d outside 0..1", fn, k->source);
    if (!(k->threshold >= 0.0f) || std::isinf(k->threshold)) return fail(c, GLRTX_EINVAL, "%s: threshold %g is not a finite number >= 0", fn, (double)k->threshold);
    if (!(k->strength >= 0.0f && k->strength <= 1.0e4f)) return fail(c, GLRTX_EINVAL, "%s: strength %g outside [0, 1e4]", fn, (double)k->strength);
    if (k->levels < 1 || k->levels > 8) return fail(c, GLRTX_EINVAL, "%s: levels %d outside 1..8", fn, k->levels);
    return GLRTX_OK;
}

// The context checks every call that takes a glrtx_bloom_cfg shares, and the source the cfg names.
int bloom_source(glrtx_ctx *c, const glrtx_bloom_cfg *k, const char *fn, const float4 *&src, int &pitch_f4) {
    if (int rc = bloom_cfg_check(c, k, fn)) return rc;
    if (!c->accum || c->width < 1 || c->owned_rows < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (c->world > 1) return fail(c, GLRTX_EINVAL, "%s: the context is partitioned (rank %d of %d): the glow would stop at every stripe's seam", fn, c->rank, c->world);
    return hdr_source(c, k->source, fn, src, pitch_f4);
}

// The down chain on `stream`: the source through the bright pass to D_1, then D_1 .. D_levels into the packed pyramid.
int bloom_down_passes(glrtx_ctx *c, hipStream_t stream, const float4 *src, int pitch_f4, const BloomLevels &L, float4 *pyr, const glrtx_bloom_cfg &k) {
    hipLaunchKernelGGL(bloom::bloom_down<true>, bloom::down_grid(L.w[1], L.h[1]), dim3(256), 0, stream, src, pitch_f4, L.w[0], L.h[0], pyr + L.at[1], L.w[1], L.h[1],
                       k.threshold);
    HIP_TRY(c, hipGetLastError());
    for (int j = 1; j < L.n; j++) {
        hipLaunchKernelGGL(bloom::bloom_down<false>, bloom::down_grid(L.w[j + 1], L.h[j + 1]), dim3(256), 0, stream, (const float4 *)(pyr + L.at[j]), L.w[j], L.w[j],
                           L.h[j], pyr + L.at[j + 1], L.w[j + 1], L.h[j + 1], 0.0f);
        HIP_TRY(c, hipGetLastError());
    }
    return GLRTX_OK;
}
// The up chain: U_k over D_k for k = levels - 1 .. 1, then B from U_1 and the source.
int bloom_up_passes(glrtx_ctx *c, hipStream_t stream, const float4 *src, int pitch_f4, const BloomLevels &L, float4 *pyr, float4 *B, const glrtx_bloom_cfg &k) {
    for (int j = L.n - 1; j >= 1; j--) {
        hipLaunchKernelGGL(bloom::bloom_up<false>, bloom::up_grid(L.w[j], L.h[j]), dim3(256), 0, stream, (const float4 *)(pyr + L.at[j + 1]), L.w[j + 1], L.h[j + 1],
                           pyr + L.at[j], L.w[j], L.h[j], (const float4 *)nullptr, 0, (float4 *)nullptr, 0.0f, 0.0f);
        HIP_TRY(c, hipGetLastError());
    }
    hipLaunchKernelGGL(bloom::bloom_up<true>, bloom::up_grid(L.w[0], L.h[0]), dim3(256), 0, stream, (const float4 *)(pyr + L.at[1]), L.w[1], L.h[1], (float4 *)nullptr,
                       L.w[0], L.h[0], src, pitch_f4, B, k.strength, 1.0f / (float)k.levels);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}
// B's and the pyramid's allocations (the pyramid always at its eight-level size: a shape has one); B is about to be written
int bloom_ensure(glrtx_ctx *c) {
    if (int rc = ensure(c, c->blPyr, bloom_levels(c->width, c->owned_rows, 8).at[9] * sizeof(float4))) return rc;
    return plane_packed(c, c->blB);
}

}  // namespace

extern "C" {

int glrtx_abi_version(void) { return GLRTX_ABI_VERSION; }

const char *glrtx_last_error(const glrtx_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int glrtx_create(glrtx_ctx **out, int device_id) {
    if (!out) return fail(nullptr, GLRTX_EINVAL, "glrtx_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n == 0)
        return fail(nullptr, GLRTX_EDEVICE, "no HIP device available (%s)", e == hipSuccess ? "count 0" : hipGetErrorString(e));
    if (device_id < 0) {
        if (hipGetDevice(&device_id) != hipSuccess) device_id = 0;
    }
    if (device_id >= n) return fail(nullptr, GLRTX_EINVAL, "device %d out of range (%d devices)", device_id, n);
    hipDeviceProp_t prop;
    if ((e = hipGetDeviceProperties(&prop, device_id)) != hipSuccess)
        return fail(nullptr, GLRTX_EDEVICE, "hipGetDeviceProperties: %s", hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, GLRTX_EDEVICE, "device %d is %s; this library is built for gfx950 only", device_id, prop.gcnArchName);
    glrtx_ctx *c = new (std::nothrow) glrtx_ctx;
    if (!c) return fail(nullptr, GLRTX_ENOMEM, "out of host memory");
    c->device = device_id;
    if ((e = hipSetDevice(device_id)) != hipSuccess || (e = hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking)) != hipSuccess ||
        (e = hipEventCreate(&c->tm0)) != hipSuccess || (e = hipEventCreate(&c->tm1)) != hipSuccess ||
        (e = hipEventCreate(&c->rs0)) != hipSuccess || (e = hipEventCreate(&c->rs1)) != hipSuccess ||
        (e = hipMalloc(&c->counter.p, 2 * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(c->counter.p, 0, 2 * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMalloc(&c->work.p, 64)) != hipSuccess ||
        (e = hipEventCreateWithFlags(&c->state_done, hipEventDisableTiming)) != hipSuccess ||
        (e = hipHostMalloc((void **)&c->guard_host, 64, hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
        (e = hipHostGetDevicePointer((void **)&c->guard_dev, c->guard_host, 0)) != hipSuccess) {
        fail(nullptr, GLRTX_EDEVICE, "context setup failed: %s", hipGetErrorString(e));
        glrtx_destroy(c);
        return GLRTX_EDEVICE;
    }
    for (auto &r : c->ring)
        if ((e = hipEventCreate(&r.ev0)) != hipSuccess || (e = hipEventCreate(&r.evm)) != hipSuccess || (e = hipEventCreate(&r.eva)) != hipSuccess ||
            (e = hipEventCreate(&r.ev1)) != hipSuccess) {
            fail(nullptr, GLRTX_EDEVICE, "context setup failed: %s", hipGetErrorString(e));
            glrtx_destroy(c);
            return GLRTX_EDEVICE;
        }
    std::memset(c->guard_host, 0, 64);
    c->stream = c->own_stream;
    // The slots' streams are created at a priority of their own (GLRTX_PIPE_PRIORITY: high (default) | normal | low).  The runtime maps the streams of a process onto a
    // few hardware queues PER PRIORITY LEVEL, and streams that share a queue run one after the other: at the default priority the slots share those queues with
    // whatever streams the host application creates, and two caller streams kept busy with small kernels took one launch per frame from 1.25 to 2.7 ms
    // (tests/test_gpu_parity.py::test_overlapped_launches_next_to_a_callers_own_streams).  At a priority of their own the slots are mapped among themselves.
    // NOTE for embedders: at "high" the library's render kernels are scheduled ahead of the host application's own normal-priority work on this GPU.
    int prio_least = 0, prio_greatest = 0, prio = 0;
    if (hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest) != hipSuccess) { (void)hipGetLastError(); prio_least = prio_greatest = 0; }
    {
        const char *v = std::getenv("GLRTX_PIPE_PRIORITY");
        const std::string m = v ? v : "high";
        prio = m == "low" ? prio_least : (m == "normal" ? 0 : prio_greatest);
        prio = std::max(std::min(prio, prio_least), prio_greatest);  // numerically: greatest <= prio <= least
    }
    for (auto &sl : c->pipe)
        if ((e = hipStreamCreateWithPriority(&sl.stream, hipStreamNonBlocking, prio)) != hipSuccess || (e = hipEventCreateWithFlags(&sl.render_done, hipEventDisableTiming)) != hipSuccess ||
            (e = hipEventCreateWithFlags(&sl.acc_done, hipEventDisableTiming)) != hipSuccess || (e = hipMalloc(&sl.work.p, 64)) != hipSuccess) {
            fail(nullptr, GLRTX_EDEVICE, "context setup failed: %s", hipGetErrorString(e));
            glrtx_destroy(c);
            return GLRTX_EDEVICE;
        }
    for (auto &sl : c->pipe) {
        if (hipHostMalloc((void **)&sl.feed_h, sizeof(FeedHost), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
            hipHostGetDevicePointer((void **)&sl.feed_h_dev, sl.feed_h, 0) != hipSuccess) {
            (void)hipGetLastError();
            c->feed_ok = false;  // no host-coherent memory: launches are never fed (they still overlap as in round 5)
            break;
        }
        std::memset(sl.feed_h, 0, sizeof(FeedHost));
    }
    c->pipeline = std::getenv("GLRTX_NO_PIPELINE") == nullptr;
    if (const char *v = std::getenv("GLRTX_PIPE_SHARE")) c->pipe_share = std::max(1, std::min(4, std::atoi(v)));
    if (const char *v = std::getenv("GLRTX_PIPE_SLOTS")) c->pipe_slots = (unsigned)std::max(1, std::min((int)kPipeSlots, std::atoi(v)));
    c->n_cu = prop.multiProcessorCount;
    if (const char *v = std::getenv("GLRTX_VARIANT")) { const int x = std::atoi(v); if (x >= 0 && x <= 2) c->variant = x; }
    if (const char *v = std::getenv("GLRTX_SHADOW_LIMIT")) c->sc.shadow_limited = std::atoi(v) != 0 ? 1 : 0;  // default 0: the reference's own search (pt_kernel.hip.h: shadow_limit)
    *out = c;
    return GLRTX_OK;
}

void glrtx_destroy(glrtx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->own_stream) (void)hipStreamSynchronize(c->own_stream);
    {
        glrtx_ctx::Present &P = c->pres;
        if (P.copy) { (void)hipStreamSynchronize(P.copy); (void)hipStreamDestroy(P.copy); }
        for (auto &im : P.img) {
            if (im.ev) (void)hipEventDestroy(im.ev);
            if (im.host && !P.full) (void)hipHostFree(im.host);
        }
        dev_free(P.dev);
        if (P.pass_done) (void)hipEventDestroy(P.pass_done);
        if (P.t0) (void)hipEventDestroy(P.t0);
        if (P.t1) (void)hipEventDestroy(P.t1);
    }
    for (auto &sl : c->pipe) {
        if (sl.stream) { (void)hipStreamSynchronize(sl.stream); (void)hipStreamDestroy(sl.stream); }
        if (sl.render_done) (void)hipEventDestroy(sl.render_done);
        if (sl.acc_done) (void)hipEventDestroy(sl.acc_done);
        dev_free(sl.state); dev_free(sl.queues); dev_free(sl.planes); dev_free(sl.work); dev_free(sl.feed_d);
        for (auto &ch : sl.chunks) dev_free(ch);
        if (sl.feed_h) (void)hipHostFree(sl.feed_h);
    }
    dev_free(c->texDesc); dev_free(c->texTexels); dev_free(c->texSt); dev_free(c->texBind); dev_free(c->texMaps); dev_free(c->cutRec); dev_free(c->cutTri);
    dev_free(c->emitMat); dev_free(c->emitSt);
    for (DevBuf *b : {&c->envTexels, &c->envRowQ, &c->envRowAlias, &c->envColQ, &c->envColAlias, &c->envCellP}) dev_free(*b);
    dev_free(c->spheres); dev_free(c->sphereMat); dev_free(c->volDensity); dev_free(c->volTemp); dev_free(c->forks); dev_free(c->cnodes); dev_free(c->cranks); dev_free(c->nrms); dev_free(c->mats); dev_free(c->lights); dev_free(c->vine);
    dev_free(c->accum_own); dev_free(c->counter); dev_free(c->rgba8); dev_free(c->work);
    c->adHalf.drop(); dev_free(c->adMask); dev_free(c->adList); dev_free(c->adCount);
    c->mmM.drop(); dev_free(c->mmM_spare);
    c->rwC.drop();
    dev_free(c->tmExp); c->tmT.drop();
    c->blB.drop(); dev_free(c->blPyr);
    denoise_release(c);
    dev_free(c->mtPos); dev_free(c->mtNrm);
    dev_free(c->wfState); dev_free(c->wfQ); dev_free(c->wfSeeds); dev_free(c->wfPlanes);
    dev_free(c->bvhVert); dev_free(c->bvhTri); dev_free(c->bvhNodes);
    dev_free(c->rf.ints); dev_free(c->rf.keys); dev_free(c->rf.vert);
    dev_free(c->sk.rest); dev_free(c->sk.rig); dev_free(c->sk.pose); dev_free(c->sk.dq); dev_free(c->sk.morph);
    dev_free(c->sk.srow); dev_free(c->sk.sent); dev_free(c->sk.swt);
    normals_drop(c);
    dev_free(c->qwire); dev_free(c->qcounter); dev_free(c->qrays); dev_free(c->qhits);
    if (c->rf.slot_ev) (void)hipEventDestroy(c->rf.slot_ev);
    if (c->bvhWs.p) { (void)hipFree(c->bvhWs.p); c->bvhWs.p = nullptr; c->bvhWs.bytes = 0; }
    for (auto &r : c->ring) {
        if (r.ev0) (void)hipEventDestroy(r.ev0);
        if (r.evm) (void)hipEventDestroy(r.evm);
        if (r.eva) (void)hipEventDestroy(r.eva);
        if (r.ev1) (void)hipEventDestroy(r.ev1);
    }
    if (c->tm0) (void)hipEventDestroy(c->tm0);
    if (c->tm1) (void)hipEventDestroy(c->tm1);
    if (c->rs0) (void)hipEventDestroy(c->rs0);
    if (c->rs1) (void)hipEventDestroy(c->rs1);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    if (c->guard_host) (void)hipHostFree(c->guard_host);
    if (c->state_done) (void)hipEventDestroy(c->state_done);
    delete c;
}

int glrtx_upload_scene(glrtx_ctx *c, const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat,
                       size_t n_mat, const float *light, size_t n_light, const float *bvh, size_t n_nodes) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    Packed P;
    if (int prc = pack_scene(c, nullptr, P, vert, n_vert, tri, n_tri, mat, n_mat, light, n_light, bvh, n_nodes)) return prc;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<float4> &forks = P.forks, &tris = P.tris, &nrms = P.nrms, &mats = P.mats, &lights = P.lights;
    const int root_ref = P.root_ref, stack_need = P.stack_need;

    int rc;
    // one node array: the leaf records in reverse order of their ids (id k at record index ~k; id 0, directly in front of fork 0, is the
    // all-zero record an absent child refers to: never hit), then the forks (DevScene::forks points at fork 0)
    const size_t tri_f4 = tris.size(), n_ids = tris.size() / 4;
    if ((tri_f4 + forks.size()) * sizeof(float4) >= ((size_t)1 << 32)) return fail(c, GLRTX_EINVAL, "glrtx_upload_scene: node array exceeds 4 GiB");
    std::vector<float4> nodes(tri_f4 + forks.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t id = 0; id < n_ids; id++) std::memcpy(&nodes[4 * (n_ids - 1 - id)], &tris[4 * id], 4 * sizeof(float4));
    std::memcpy(nodes.data() + tri_f4, forks.data(), forks.size() * sizeof(float4));
    if ((rc = dev_upload(c, c->forks, nodes.data(), nodes.size() * sizeof(float4)))) return rc;
    if ((rc = dev_upload(c, c->cnodes, P.cnodes.data(), P.cnodes.size() * sizeof(float4)))) return rc;
    if ((rc = dev_upload(c, c->cranks, P.cranks.data(), P.cranks.size() * sizeof(uint2)))) return rc;
    if ((rc = dev_upload(c, c->nrms, nrms.data(), nrms.size() * sizeof(float4)))) return rc;
    if ((rc = dev_upload(c, c->mats, mats.data(), mats.size() * sizeof(float4)))) return rc;
    if ((rc = dev_upload(c, c->lights, lights.data(), lights.size() * sizeof(float4)))) return rc;
    if (!P.vine.empty() && (rc = dev_upload(c, c->vine, P.vine.data(), P.vine.size() * sizeof(float4)))) return rc;
    c->have_scene = false;  // (until the plan is in place too)
    {
        std::vector<int> wire(P.leaf_tri.size() + 1, -1);
        for (size_t k = 0; k < P.leaf_tri.size(); k++) wire[k + 1] = P.leaf_tri[k];
        if ((rc = dev_upload(c, c->qwire, wire.data(), wire.size() * sizeof(int)))) return rc;
    }
    const size_t scene_bytes[5] = {nodes.size() * sizeof(float4), P.cnodes.size() * sizeof(float4), nrms.size() * sizeof(float4), lights.size() * sizeof(float4),
                                   P.vine.size() * sizeof(float4)};
    if ((rc = refit_plan_upload(c, P, tri, light, n_light, bvh, n_nodes, n_vert, scene_bytes))) return rc;

    DevScene &sc = c->sc;
    sc.forks = (const float4 *)c->forks.p + tri_f4;
    sc.nodes0 = (const float4 *)c->forks.p;
    sc.node_bias = (unsigned)(tri_f4 * sizeof(float4));
    sc.cnodes = (const float4 *)c->cnodes.p;
    sc.cranks = (const uint2 *)c->cranks.p;
    sc.n_crank = (int)P.cranks.size();
    sc.nrms = (const float4 *)c->nrms.p;
    sc.mats = (const float4 *)c->mats.p;
    sc.lights = (const float4 *)c->lights.p;
    sc.root_ref = root_ref;
    sc.root_boxed = P.root_boxed;
    sc.root_lo = P.root_lo; sc.root_hi = P.root_hi;
    sc.n_light = (int)n_light;
    sc.n_mat = (int)n_mat;
    sc.n_fork = (int)(forks.size() / 4);
    sc.stack_entries = stack_need;
    sc.mats_in_lds = (n_mat > 0 && n_mat <= (size_t)kMaxLdsMaterials) ? 1 : 0;
    sc.lights_in_lds = (n_light > 0 && n_light <= (size_t)kMaxLdsLights && std::getenv("GLRTX_NO_LDS_LIGHTS") == nullptr) ? 1 : 0;
    sc.lds_head_f4 = (sc.mats_in_lds ? 3 * (int)n_mat : 0) + (sc.lights_in_lds ? 6 * (int)n_light : 0);
    sc.vine = P.vine.empty() ? nullptr : (const float4 *)c->vine.p;
    sc.n_vine = P.n_vine;
    sc.vine_main = P.vine_main;
    sc.vine_uniform = P.vine_uniform;
    if (std::getenv("GLRTX_NO_VINE_SCAN")) sc.n_vine = 0;  // A/B: force the generic tree traversal
    c->n_tri = (int)n_tri; c->n_fork = (int)(forks.size() / 4); c->n_mat = (int)n_mat; c->n_light = (int)n_light;
    c->have_scene = true;
    c->leaf_tri.swap(P.leaf_tri);
    c->n_spheres = 0;  // spheres reference this scene's materials: upload them again after a new scene
    c->n_tex = 0;      // ... and so does a texture set's binding (glrtx_upload_textures)
    c->have_maps = false;  // ... and the material maps bound on top of it (glrtx_bind_material_maps)
    c->have_cut = false;   // ... and the cutout records (glrtx_bind_cutouts)
    c->have_emit = false;  // ... and the emission maps (glrtx_bind_emission_maps)
    c->scene_light_st.assign(6 * n_light, 0.0f);  // the corners' (s, t) of every light: words 6 and 7 of its three wire vertices, in wire order
    for (size_t l = 0; l < n_light; l++)
        for (int j = 0; j < 3; j++) {
            const float *v = vert + 15 * (size_t)light[4 * l + j];
            c->scene_light_st[6 * l + 2 * j] = v[6]; c->scene_light_st[6 * l + 2 * j + 1] = v[7];
        }
    c->scene_mat.assign(c->leaf_tri.size() + 1, -1);  // the material of every device triangle: word 3 of a wire triangle
    for (size_t k = 0; k < c->leaf_tri.size(); k++) c->scene_mat[k + 1] = (int32_t)tri[4 * (size_t)c->leaf_tri[k] + 3];
    c->scene_st.assign(6 * (c->leaf_tri.size() + 1), 0.0f);  // the corners' (s, t) of every device triangle: words 6 and 7 of a wire vertex
    for (size_t k = 0; k < c->leaf_tri.size(); k++)
        for (int j = 0; j < 3; j++) {
            const float *v = vert + 15 * (size_t)tri[4 * (size_t)c->leaf_tri[k] + j];
            c->scene_st[6 * (k + 1) + 2 * j] = v[6]; c->scene_st[6 * (k + 1) + 2 * j + 1] = v[7];
        }
    dev_free(c->mtPos); dev_free(c->mtNrm);  // (glrtx_track_motion: the previous geometry was another scene's; the stream is idle)
    c->mt_geom = glrtx_ctx::kMtNone;
    dev_free(c->sk.rest); dev_free(c->sk.rig); dev_free(c->sk.pose);  // (glrtx_upload_rig: the rig was another scene's)
    dev_free(c->sk.dq);
    morph_drop(c);
    c->sk.n_bones = 0;
    normals_drop(c);  // (glrtx_upload_normal_topology, glrtx_set_pose_normals: the topology was another scene's)
    c->st.stack_entries = stack_need;
    c->st.lds_bytes = lds_bytes_for(sc);
    c->st.n_tri = c->n_tri; c->st.n_fork = c->n_fork; c->st.n_mat = c->n_mat; c->st.n_light = c->n_light;
    return GLRTX_OK;
}

namespace {

// The refit (refit.hip.h) from device vertices on the context's stream, behind every launch that may still read the scene; blocks until it has run and
// the root box and vine_uniform -- kernel arguments -- are read back.  Launches issued after it are therefore ordered after it, on any stream.
int refit_run(glrtx_ctx *c, const void *dev_vert) {
    glrtx_ctx::Refit &R = c->rf;
    for (auto &sl : c->pipe)
        if (sl.stream && sl.used) {
            HIP_TRY(c, hipEventRecord(R.slot_ev, sl.stream));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, R.slot_ev, 0));
        }
    refit::Args a = R.a;
    a.vert = (const unsigned *)dev_vert;
    const int n1 = std::max(1, a.n_leaf + a.n_extra + a.n_light);
    hipLaunchKernelGGL(refit::k_refit_leaves, dim3((n1 + refit::kBlock - 1) / refit::kBlock), dim3(refit::kBlock), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    if (a.n_vine > 0) {
        hipLaunchKernelGGL(refit::k_refit_vine, dim3(1), dim3(refit::kVineBlock), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
    }
    const int n3 = 2 * a.n_fork + a.n_cpos + a.n_vine + 1;
    hipLaunchKernelGGL(refit::k_refit_scatter, dim3((n3 + refit::kBlock - 1) / refit::kBlock), dim3(refit::kBlock), 0, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    unsigned out[8];
    HIP_TRY(c, hipMemcpyAsync(out, a.out, sizeof out, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    float f[6];
    std::memcpy(f, out, sizeof f);
    c->sc.root_lo = make_float4(f[0], f[1], f[2], 0.f);
    c->sc.root_hi = make_float4(f[3], f[4], f[5], 0.f);
    c->sc.vine_uniform = a.n_vine > 0 && out[6] != 0u ? 1 : 0;
    return GLRTX_OK;
}

// glrtx_track_motion: the scene's leaf records as they stand become the previous geometry (motion::snapshot_kernel), on the context's stream.  Only reads the
// scene, so it needs no wait for the pipe slots; the refit that follows on the same stream is ordered behind it.
int motion_snapshot(glrtx_ctx *c) {
    const size_t bytes = (size_t)std::max(c->n_tri, 1) * 3 * sizeof(float4);
    for (DevBuf *b : {&c->mtPos, &c->mtNrm})
        if (b->bytes < bytes) {  // (triangles no leaf names are never looked up: G holds leaves' triangles only; zeroed all the same)
            if (int rc = ensure(c, *b, bytes)) return rc;
            HIP_TRY(c, hipMemsetAsync(b->p, 0, b->bytes, c->stream));
        }
    const refit::Args &r = c->rf.a;
    motion::SnapArgs a;
    a.nodes = r.nodes; a.nrms = r.nrms;
    a.wire = (const int *)c->qwire.p;
    a.n_ids = r.n_ids; a.n_leaf = r.n_leaf; a.n_tri = c->n_tri;
    a.prev_pos = (uint4 *)c->mtPos.p; a.prev_nrm = (uint4 *)c->mtNrm.p;
    if (a.n_leaf > 0) {
        hipLaunchKernelGGL(motion::snapshot_kernel, dim3((unsigned)((a.n_leaf + 255) / 256)), dim3(256), 0, c->stream, a);
        HIP_TRY(c, hipGetLastError());
    }
    c->mt_geom = glrtx_ctx::kMtSaved;
    return GLRTX_OK;
}

int update_check(glrtx_ctx *c, const void *vert, size_t n_vert, const char *fn) {
    if (!c) return GLRTX_EINVAL;
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (!vert) return fail(c, GLRTX_EINVAL, "%s: NULL vertices", fn);
    if (n_vert != c->rf.n_vert) return fail(c, GLRTX_EINVAL, "%s: %zu vertices, the scene was uploaded with %zu", fn, n_vert, c->rf.n_vert);
    return GLRTX_OK;
}

// ---- rebuilding normals (glrtx_upload_normal_topology, glrtx_update_positions, glrtx_set_pose_normals, glrtx_debug_rebuild_normals; normals.hip.h)
static_assert(normals::kChunk == GLRTX_NORMAL_CHUNK && glrt_detail::kNormalChunk == GLRTX_NORMAL_CHUNK &&
                  glrt_detail::kNormalsWeldPositions == GLRTX_NORMALS_WELD_POSITIONS,
              "normals.hip.h, host/normal_topology.h and glrtx.h disagree");

// The rebuild in place on a.vert: face vectors, class sums, the members' normal words
void normals_launch(const normals::Args &a, hipStream_t stream) {
    const auto grid = [](unsigned n) { return dim3((n + normals::kBlock - 1) / normals::kBlock); };
    if (a.n_vert == 0) return;
    if (a.n_tri > 0) hipLaunchKernelGGL(normals::face_kernel, grid(a.n_tri), dim3(normals::kBlock), 0, stream, a);
    hipLaunchKernelGGL(normals::class_kernel, grid(a.n_classes), dim3(normals::kBlock), 0, stream, a);
    hipLaunchKernelGGL(normals::vertex_kernel, grid(a.n_vert), dim3(normals::kBlock), 0, stream, a);
}

// The context's rebuild on its vertex buffer (which the caller has just written on the stream)
void normals_run(glrtx_ctx *c) {
    normals::Args a = c->nm.a;
    a.vert = (unsigned *)c->rf.vert.p;
    normals_launch(a, c->stream);
}

// The index of a checked mesh as the kernels read it: 16-byte triangle records {i0, i1, i2, flip as a sign mask}, and the face lists as 32-bit rows.  Returns
// false when the lists hold 2^32 entries or more.
bool normals_index(const float *tri, size_t n_tri, const uint32_t *cls, const uint8_t *flip, size_t n_vert, std::vector<uint4> &rec, std::vector<unsigned> &row,
                   std::vector<uint32_t> &face) {
    std::vector<uint64_t> row64;
    glrt_detail::normal_face_lists(tri, n_tri, cls, n_vert, row64, face);
    if (row64.back() >= ((uint64_t)1 << 32)) return false;
    row.assign(row64.begin(), row64.end());
    rec.resize(n_tri);
    for (size_t t = 0; t < n_tri; t++)
        rec[t] = make_uint4((unsigned)tri[4 * t], (unsigned)tri[4 * t + 1], (unsigned)tri[4 * t + 2], flip[t] ? 0x80000000u : 0u);
    return true;
}

int normals_fault(glrtx_ctx *c, const glrt_detail::NormalFault &f, size_t n_vert, const char *fn) {
    char why[256];
    glrt_detail::normal_fault_message(f, n_vert, why, sizeof why);
    return fail(c, GLRTX_EINVAL, "%s: %s", fn, why);
}

// ---- a geometry move (DESIGN.md "A geometry move"): the call's checks, move_begin, the new vertices written on the context's stream, move_commit
// Nothing more goes into an open launch; with own_buffer the context's vertex buffer is there to be written (a caller's device vertices need none).
// (static, as the other new helpers below: an unnamed namespace inside this file's extern "C" block does not keep a name out of the dynamic symbol table)
static int move_begin(glrtx_ctx *c, bool own_buffer) {
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return own_buffer ? ensure(c, c->rf.vert, c->rf.n_vert * normals::kVertexWords * sizeof(float)) : GLRTX_OK;
}

// The vertices at dev_vert become the scene's: the rebuild in the context's buffer if asked for, the previous geometry kept if this is the first move since the
// last feature pass (glrtx_track_motion), then the refit
static int move_commit(glrtx_ctx *c, const void *dev_vert, bool rebuild_normals) {
    if (rebuild_normals) normals_run(c);
    HIP_TRY(c, hipGetLastError());
    if (c->mt_on && c->mt_geom == glrtx_ctx::kMtCurrent)
        if (int rc = motion_snapshot(c)) return rc;
    return refit_run(c, dev_vert);
}

// glrtx_update_positions / _device between begin and commit: the records from `dev_pos` and the topology's rest copy
int positions_run(glrtx_ctx *c, const void *dev_pos) {
    const size_t n_vert = c->rf.n_vert;
    if (n_vert > 0)
        hipLaunchKernelGGL(normals::positions_kernel, dim3((unsigned)((n_vert + normals::kBlock - 1) / normals::kBlock)), dim3(normals::kBlock), 0, c->stream,
                           (const unsigned *)c->nm.rest.p, (const unsigned *)dev_pos, (unsigned *)c->rf.vert.p, (unsigned)n_vert);
    return move_commit(c, c->rf.vert.p, true);
}

int positions_check(glrtx_ctx *c, const void *pos, size_t n_vert, const char *fn) {
    if (int rc = update_check(c, pos, n_vert, fn)) return rc;
    if (!c->nm.have) return fail(c, GLRTX_EINVAL, "%s: no normal topology uploaded (glrtx_upload_normal_topology)", fn);
    return GLRTX_OK;
}

}  // namespace

int glrtx_upload_normal_topology(glrtx_ctx *c, const float *rest_vert, size_t n_vert, const float *tri, size_t n_tri, unsigned flags) {
    const char *fn = "glrtx_upload_normal_topology";
    if (int rc = update_check(c, rest_vert, n_vert, fn)) return rc;
    if (flags & ~GLRTX_NORMALS_WELD_POSITIONS) return fail(c, GLRTX_EINVAL, "%s: unknown flag bits 0x%x", fn, flags & ~GLRTX_NORMALS_WELD_POSITIONS);
    if (!tri) return fail(c, GLRTX_EINVAL, "%s: NULL triangles", fn);
    glrt_detail::NormalFault f;
    if (!glrt_detail::normal_mesh_check(tri, n_tri, n_vert, f)) return normals_fault(c, f, n_vert, fn);
    std::vector<uint32_t> cls(n_vert), face;
    std::vector<uint8_t> flip(n_tri);
    const size_t n_classes = glrt_detail::normal_weld(rest_vert, n_vert, flags, cls.data());
    glrt_detail::normal_flips(rest_vert, tri, n_tri, flip.data());
    std::vector<uint4> rec;
    std::vector<unsigned> row;
    if (!normals_index(tri, n_tri, cls.data(), flip.data(), n_vert, rec, row, face)) return fail(c, GLRTX_EINVAL, "%s: the face lists hold 2^32 entries or more", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (as glrtx_upload_rig: the frees are ordered behind anything on the stream)
    const bool pose_on = c->nm.have && c->nm.pose_on;  // (a topology that replaces one keeps the switch)
    c->nm.have = c->nm.pose_on = false;  // (until every buffer is in place)
    glrtx_ctx::Normals &N = c->nm;
    if (int rc = dev_upload(c, N.rest, rest_vert, n_vert * normals::kVertexWords * sizeof(float))) return rc;
    if (int rc = dev_upload(c, N.tri, rec.data(), rec.size() * sizeof(uint4))) return rc;
    if (int rc = dev_upload(c, N.cls, cls.data(), cls.size() * sizeof(uint32_t))) return rc;
    if (int rc = dev_upload(c, N.row, row.data(), row.size() * sizeof(unsigned))) return rc;
    if (int rc = dev_upload(c, N.face, face.data(), face.size() * sizeof(uint32_t))) return rc;
    if (int rc = ensure(c, N.fvec, n_tri * sizeof(float4))) return rc;
    if (int rc = ensure(c, N.cnrm, n_classes * sizeof(float4))) return rc;
    N.a = normals::Args{(const uint4 *)N.tri.p, (const unsigned *)N.cls.p, (const unsigned *)N.row.p, (const unsigned *)N.face.p, nullptr, (float4 *)N.fvec.p,
                        (float4 *)N.cnrm.p, (unsigned)n_vert, (unsigned)n_tri, (unsigned)n_classes};
    N.have = true;
    N.pose_on = pose_on;
    return GLRTX_OK;
}

int glrtx_update_positions(glrtx_ctx *c, const float *pos, size_t n_vert) {
    if (int rc = positions_check(c, pos, n_vert, "glrtx_update_positions")) return rc;
    if (int rc = move_begin(c, true)) return rc;
    if (int rc = ensure(c, c->nm.pos, n_vert * 3 * sizeof(float))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->nm.pos.p, pos, n_vert * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return positions_run(c, c->nm.pos.p);
}

int glrtx_update_positions_device(glrtx_ctx *c, const void *dev_pos, size_t n_vert) {
    if (int rc = positions_check(c, dev_pos, n_vert, "glrtx_update_positions_device")) return rc;
    if (int rc = move_begin(c, true)) return rc;
    return positions_run(c, dev_pos);
}

int glrtx_set_pose_normals(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    if (enable && (!c->have_scene || !c->nm.have))
        return fail(c, GLRTX_EINVAL, "glrtx_set_pose_normals: no normal topology uploaded (glrtx_upload_normal_topology)");
    c->nm.pose_on = enable != 0;
    return GLRTX_OK;
}

int glrtx_debug_rebuild_normals(const float *vert_in, size_t n_vert, const float *tri, size_t n_tri, const uint32_t *class_of_vertex, const uint8_t *flip,
                                float *vert_out) {
    const char *fn = "glrtx_debug_rebuild_normals";
    if ((n_vert > 0 && (!vert_in || !class_of_vertex || !vert_out)) || (n_tri > 0 && !flip)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    glrt_detail::NormalFault f;
    if (!glrt_detail::normal_mesh_check(tri, n_tri, n_vert, f) || !glrt_detail::normal_class_check(class_of_vertex, n_vert, f))
        return normals_fault(nullptr, f, n_vert, fn);
    if (n_vert == 0) return GLRTX_OK;
    std::vector<uint4> rec;
    std::vector<unsigned> row;
    std::vector<uint32_t> face;
    if (!normals_index(tri, n_tri, class_of_vertex, flip, n_vert, rec, row, face)) return fail(nullptr, GLRTX_EINVAL, "%s: the face lists hold 2^32 entries or more", fn);
    const size_t bytes = n_vert * normals::kVertexWords * sizeof(float);
    DebugScratch s;
    normals::Args a{};
    a.tri = s.alloc<uint4>(std::max<size_t>(rec.size(), 1) * sizeof(uint4), rec.empty() ? nullptr : rec.data());
    a.cls = s.alloc<unsigned>(n_vert * sizeof(unsigned), class_of_vertex);
    a.row = s.alloc<unsigned>(row.size() * sizeof(unsigned), row.data());
    a.face = s.alloc<unsigned>(std::max<size_t>(face.size(), 1) * sizeof(unsigned), face.empty() ? nullptr : face.data());
    a.vert = s.alloc<unsigned>(bytes, vert_in);
    a.fvec = s.alloc<float4>(std::max<size_t>(n_tri, 1) * sizeof(float4));
    a.cnrm = s.alloc<float4>((row.size() - 1) * sizeof(float4));
    a.n_vert = (unsigned)n_vert; a.n_tri = (unsigned)n_tri; a.n_classes = (unsigned)(row.size() - 1);
    if (s.ok()) {
        normals_launch(a, 0);
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(vert_out, a.vert, bytes);
    return s.result(GLRTX_OK, fn);
}

// Device time of the rebuild by itself, as glrtx_debug_skin_burst: the three passes on the context's vertex buffer, whose normal words then hold the rebuilt
// normals of the positions that are there (after a glrtx_update_positions or a pose under glrtx_set_pose_normals: exactly what they hold already).
int glrtx_debug_normals_burst(glrtx_ctx *c, int reps, float *ms_per_launch) {
    const char *fn = "glrtx_debug_normals_burst";
    if (!c || !ms_per_launch || reps < 1) return GLRTX_EINVAL;
    if (!c->have_scene || !c->nm.have || c->rf.vert.bytes < c->rf.n_vert * normals::kVertexWords * sizeof(float))
        return fail(c, GLRTX_EINVAL, "%s: no normal topology uploaded, or no vertices in the vertex buffer yet", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return burst_time(c, reps, ms_per_launch, [&] { normals_run(c); return GLRTX_OK; });
}

int glrtx_update_vertices(glrtx_ctx *c, const float *vert, size_t n_vert) {
    if (int rc = update_check(c, vert, n_vert, "glrtx_update_vertices")) return rc;
    if (int rc = move_begin(c, true)) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->rf.vert.p, vert, n_vert * 15 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return move_commit(c, c->rf.vert.p, false);
}

int glrtx_update_vertices_device(glrtx_ctx *c, const void *dev_vert, size_t n_vert) {
    if (int rc = update_check(c, dev_vert, n_vert, "glrtx_update_vertices_device")) return rc;
    if (int rc = move_begin(c, false)) return rc;  // (the caller's buffer is read where it is: the context's stays unallocated)
    return move_commit(c, dev_vert, false);
}

namespace {

// ---- posing (glrtx_upload_rig, glrtx_pose, glrtx_debug_skin; skin.hip.h)
bool all_finite(const float *v, size_t n) {
    for (size_t k = 0; k < n; k++)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// What the rig calls refuse alike; weights are the context call's to check (the debug hook takes any).
int rig_check(glrtx_ctx *c, const void *rest, size_t n_vert, const int32_t *bones4, const float *weights4, int n_bones, const char *fn) {
    if (n_bones < 1 || n_bones > GLRT_MAX_BONES) return fail(c, GLRTX_EINVAL, "%s: %d bones (1 .. %d)", fn, n_bones, GLRT_MAX_BONES);
    if (n_vert >= ((size_t)1 << 31)) return fail(c, GLRTX_EINVAL, "%s: %zu vertices (at most 2^31 - 1)", fn, n_vert);
    if (n_vert > 0 && (!rest || !bones4 || !weights4)) return fail(c, GLRTX_EINVAL, "%s: NULL buffer", fn);
    for (size_t k = 0; k < 4 * n_vert; k++)
        if (bones4[k] < 0 || bones4[k] >= n_bones) return fail(c, GLRTX_EINVAL, "%s: vertex %zu names bone %d of %d", fn, k / 4, (int)bones4[k], n_bones);
    return GLRTX_OK;
}

// The kernel's rig records: {b0, b1, b2, b3} {w0, w1, w2, w3} a vertex, 32 bytes
void rig_records(std::vector<uint4> &r, size_t n_vert, const int32_t *bones4, const float *weights4) {
    r.resize(2 * n_vert);
    for (size_t i = 0; i < n_vert; i++) {
        std::memcpy(&r[2 * i], bones4 + 4 * i, sizeof(uint4));
        std::memcpy(&r[2 * i + 1], weights4 + 4 * i, sizeof(uint4));
    }
}

}  // namespace

int glrtx_upload_rig(glrtx_ctx *c, const float *rest_vert, size_t n_vert, const int32_t *bones4, const float *weights4, int n_bones) {
    const char *fn = "glrtx_upload_rig";
    if (int rc = update_check(c, rest_vert, n_vert, fn)) return rc;
    if (int rc = rig_check(c, rest_vert, n_vert, bones4, weights4, n_bones, fn)) return rc;
    if (!all_finite(weights4, 4 * n_vert)) return fail(c, GLRTX_EINVAL, "%s: a weight is not finite", fn);
    std::vector<uint4> rig;
    rig_records(rig, n_vert, bones4, weights4);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a glrtx_pose's kernel has run: glrtx_pose blocks; this orders the frees behind anything else on the stream)
    c->sk.n_bones = 0;  // (until all three buffers are in place)
    morph_drop(c);  // the morph targets were the previous rig's (glrtx_upload_morph_targets, glrtx_upload_morph_targets_sparse)
    if (int rc = dev_upload(c, c->sk.rest, rest_vert, n_vert * skin::kVertexWords * sizeof(float))) return rc;
    if (int rc = dev_upload(c, c->sk.rig, rig.data(), rig.size() * sizeof(uint4))) return rc;
    if (int rc = ensure(c, c->sk.pose, (size_t)n_bones * 12 * sizeof(float))) return rc;
    c->sk.n_bones = n_bones;
    return GLRTX_OK;
}

namespace {

// ---- deforming (glrtx_upload_morph_targets, glrtx_pose_morph, glrtx_pose_dualquat, glrtx_debug_deform; skin.hip.h: deform_kernel)
static_assert(skin::kMaxTargets == GLRTX_MAX_MORPH_TARGETS, "skin.hip.h and glrtx.h disagree");

// The kernel's list of active targets: those whose weight is not a zero after the flush, in ascending index
void morph_list(skin::Morph &m, const float *weights, int n_targets) {
    m.n_active = 0;
    for (int k = 0; k < n_targets; k++)
        if (!glrt_detail::tiny(weights[k])) {
            m.index[m.n_active] = (unsigned)k;
            m.weight[m.n_active++] = weights[k];
        }
}

// What the pose calls and the debug hook refuse alike about the morph weights
int morph_check(glrtx_ctx *c, const float *morph_weights, int n_targets, const char *fn, int cap = GLRTX_MAX_MORPH_TARGETS) {
    if (n_targets < 0 || n_targets > cap) return fail(c, GLRTX_EINVAL, "%s: %d morph targets (0 .. %d)", fn, n_targets, cap);
    if (n_targets > 0 && !morph_weights) return fail(c, GLRTX_EINVAL, "%s: NULL morph weights", fn);
    if (!all_finite(morph_weights, (size_t)n_targets)) return fail(c, GLRTX_EINVAL, "%s: a morph weight is not finite", fn);
    return GLRTX_OK;
}

// ---- sparse targets (glrtx_upload_morph_targets_sparse, glrtx_debug_deform_sparse; skin.hip.h: deform_sparse_kernel)
static_assert(skin::kMaxSparseTargets == GLRTX_MAX_SPARSE_MORPH_TARGETS && glrt_detail::kMaxSparseTargets == GLRTX_MAX_SPARSE_MORPH_TARGETS,
              "skin.hip.h, host/morph_sparse.h and glrtx.h disagree");

// What the upload, the debug hook and the CPU statement refuse alike about a set in its wire form (host/morph_sparse.h)
int sparse_check(glrtx_ctx *c, const uint64_t *offsets, const uint32_t *vertex, const float *deltas, int n_targets, size_t n_vert, const char *fn) {
    glrt_detail::SparseFault f;
    if (glrt_detail::morph_sparse_check(offsets, vertex, deltas, n_targets, n_vert, f)) return GLRTX_OK;
    char why[256];
    glrt_detail::morph_sparse_message(f, n_targets, why, sizeof why);
    return fail(c, GLRTX_EINVAL, "%s: %s", fn, why);
}

// The vertex-major inverted index of a checked set: row[n_vert + 1], and the entries in row order.  A stable counting sort over the target-major input: the
// targets are walked in ascending index, so the entries of a row come out ascending by target.
void sparse_index(const uint64_t *offsets, const uint32_t *vertex, const float *deltas, int n_targets, size_t n_vert, std::vector<unsigned> &row,
                  std::vector<float4> &entry) {
    const size_t nnz = n_targets > 0 ? (size_t)offsets[n_targets] : 0;
    row.assign(n_vert + 1, 0u);
    for (size_t e = 0; e < nnz; e++) row[(size_t)vertex[e] + 1]++;
    for (size_t i = 0; i < n_vert; i++) row[i + 1] += row[i];
    entry.resize(2 * nnz);
    std::vector<unsigned> at(row.begin(), row.end() - 1);
    for (int k = 0; k < n_targets; k++)
        for (uint64_t e = offsets[k]; e < offsets[k + 1]; e++) {
            const float *d = deltas + 6 * e;
            float4 *q = entry.data() + 2 * (size_t)at[vertex[e]]++;
            q[0] = make_float4(__builtin_bit_cast(float, (unsigned)k), d[0], d[1], d[2]);
            q[1] = make_float4(d[3], d[4], d[5], 0.0f);
        }
}

// The pose's weight table: the weight of an active target, exact +0 of an inactive one.  Returns the number of active targets.
int sparse_weights(std::vector<float> &tab, const float *weights, int n_targets) {
    tab.assign((size_t)n_targets, 0.0f);
    int n_active = 0;
    for (int k = 0; k < n_targets; k++)
        if (!glrt_detail::tiny(weights[k])) {
            tab[(size_t)k] = weights[k];
            n_active++;
        }
    return n_active;
}

using PoseLaunch = glrtx_ctx::PoseLaunch;

static void pose_launch(const PoseLaunch &L, hipStream_t stream) {
    if (L.kernel == PoseLaunch::kNone || L.skin.n_vert == 0) return;
    const dim3 grid((unsigned)((L.skin.n_vert + skin::kBlock - 1) / skin::kBlock)), block(skin::kBlock);
    if (L.kernel == PoseLaunch::kSkin) hipLaunchKernelGGL(skin::skin_kernel, grid, block, 0, stream, L.skin);
    else if (L.kernel == PoseLaunch::kDeform && L.mode) hipLaunchKernelGGL(skin::deform_kernel<true>, grid, block, 0, stream, L.deform);
    else if (L.kernel == PoseLaunch::kDeform) hipLaunchKernelGGL(skin::deform_kernel<false>, grid, block, 0, stream, L.deform);
    else if (L.mode) hipLaunchKernelGGL(skin::deform_sparse_kernel<true>, grid, block, 0, stream, L.sparse);
    else hipLaunchKernelGGL(skin::deform_sparse_kernel<false>, grid, block, 0, stream, L.sparse);
}

// What the pose calls refuse alike; the bone count and the pose data each refuses in its own words
static int pose_check(glrtx_ctx *c, const char *fn) {
    if (!c) return GLRTX_EINVAL;
    if (!c->have_scene || c->sk.n_bones == 0) return fail(c, GLRTX_EINVAL, "%s: no rig uploaded (glrtx_upload_rig)", fn);
    return GLRTX_OK;
}

// A pose call behind its checks, as a geometry move: the pose data (mode 0: 12 floats a bone, mode 1: 8) into its buffer, the kernel into the context's vertex
// buffer.  kSkin is glrtx_pose; kDeform asks for the deform kernels, the dense or the sparse one as the rig's set and the weights decide.
static int pose_move(glrtx_ctx *c, PoseLaunch::Kernel kernel, int mode, const float *bone_data, const float *morph_weights, int n_targets) {
    if (int rc = move_begin(c, true)) return rc;
    glrtx_ctx::Rig &K = c->sk;
    const size_t pose_bytes = (size_t)K.n_bones * (mode ? 8 : 12) * sizeof(float);
    DevBuf &pose = mode ? K.dq : K.pose;
    if (int rc = ensure(c, pose, pose_bytes)) return rc;
    HIP_TRY(c, hipMemcpyAsync(pose.p, bone_data, pose_bytes, hipMemcpyHostToDevice, c->stream));
    // A sparse set with an active weight and an entry goes through deform_sparse_kernel; without either there is nothing to add, and deform_kernel with no
    // active target reads no delta at all: Posing's bits
    if (kernel == PoseLaunch::kDeform && K.sparse && K.nnz > 0 && sparse_weights(K.wtab, morph_weights, n_targets) > 0) kernel = PoseLaunch::kSparse;
    PoseLaunch L(kernel, mode, K.rest.p, K.rig.p, pose.p, c->rf.vert.p, c->rf.n_vert);
    if (kernel == PoseLaunch::kSparse) {
        if (int rc = ensure(c, K.swt, (size_t)n_targets * sizeof(float))) return rc;
        HIP_TRY(c, hipMemcpyAsync(K.swt.p, K.wtab.data(), (size_t)n_targets * sizeof(float), hipMemcpyHostToDevice, c->stream));
        L.sparse.row = (const unsigned *)K.srow.p; L.sparse.entry = (const float4 *)K.sent.p; L.sparse.weight = (const float *)K.swt.p;
        L.sparse.n_targets = n_targets;
    } else if (kernel == PoseLaunch::kDeform) {
        L.deform.deltas = (const float2 *)K.morph.p;
        if (!K.sparse) morph_list(L.deform.morph, morph_weights, n_targets);
    }
    pose_launch(L, c->stream);
    if (kernel != PoseLaunch::kSkin) K.last = L;  // (a glrtx_pose leaves the record: glrtx_debug_deform_burst goes on replaying the last deform launch)
    return move_commit(c, c->rf.vert.p, c->nm.pose_on);  // (glrtx_set_pose_normals: the rebuild between the kernel and the refit)
}

// glrtx_pose_morph (mode 0: n_bones x 12 floats) and glrtx_pose_dualquat (mode 1: n_bones x 8 floats)
int deform_pose(glrtx_ctx *c, const float *bone_data, int n_bones, const float *morph_weights, int n_targets, int mode, const char *fn) {
    if (int rc = pose_check(c, fn)) return rc;
    if (n_bones != c->sk.n_bones) return fail(c, GLRTX_EINVAL, "%s: %d bones, the rig has %d", fn, n_bones, c->sk.n_bones);
    if (n_targets != c->sk.n_targets) return fail(c, GLRTX_EINVAL, "%s: %d morph weights, the rig has %d targets", fn, n_targets, c->sk.n_targets);
    if (!bone_data) return fail(c, GLRTX_EINVAL, "%s: NULL pose", fn);
    if (int rc = morph_check(c, morph_weights, n_targets, fn, c->sk.sparse ? GLRTX_MAX_SPARSE_MORPH_TARGETS : GLRTX_MAX_MORPH_TARGETS)) return rc;
    if (!all_finite(bone_data, (size_t)n_bones * (mode ? 8 : 12))) return fail(c, GLRTX_EINVAL, "%s: a pose entry is not finite", fn);
    return pose_move(c, PoseLaunch::kDeform, mode, bone_data, morph_weights, n_targets);
}

// What the three pose hooks share: the rest vertices, the rig records, the pose data and the output in scratch, as one launch L; a hook adds its own
// buffers to both, then run(): the launch on the null stream, the result read back
struct PoseScratch : DebugScratch {
    size_t bytes;
    PoseLaunch L;
    PoseScratch(PoseLaunch::Kernel kernel, int mode, const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data,
                int n_bones)
        : bytes(n_vert * skin::kVertexWords * sizeof(float)) {
        std::vector<uint4> rig;
        rig_records(rig, n_vert, bones4, weights4);
        const unsigned *R = alloc<unsigned>(bytes, rest);
        const uint4 *G = alloc<uint4>(rig.size() * sizeof(uint4), rig.data());
        const float4 *P = alloc<float4>((size_t)n_bones * (mode ? 8 : 12) * sizeof(float), bone_data);
        L = PoseLaunch(kernel, mode, R, G, P, alloc<unsigned>(bytes), n_vert);
    }
    int run(float *vert_out, const char *fn) {
        if (ok()) {
            pose_launch(L, 0);
            e = hipGetLastError();
        }
        sync();
        download(vert_out, L.skin.out, bytes);
        return result(GLRTX_OK, fn);
    }
};

}  // namespace

int glrtx_upload_morph_targets(glrtx_ctx *c, const float *deltas, int n_targets, size_t n_vert) {
    const char *fn = "glrtx_upload_morph_targets";
    if (!c) return GLRTX_EINVAL;
    if (!c->have_scene || c->sk.n_bones == 0) return fail(c, GLRTX_EINVAL, "%s: no rig uploaded (glrtx_upload_rig)", fn);
    if (n_vert != c->rf.n_vert) return fail(c, GLRTX_EINVAL, "%s: %zu vertices, the rig has %zu", fn, n_vert, c->rf.n_vert);
    if (n_targets < 0 || n_targets > GLRTX_MAX_MORPH_TARGETS) return fail(c, GLRTX_EINVAL, "%s: %d morph targets (0 .. %d)", fn, n_targets, GLRTX_MAX_MORPH_TARGETS);
    if (n_targets > 0 && n_vert > 0 && !deltas) return fail(c, GLRTX_EINVAL, "%s: NULL deltas", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (as glrtx_upload_rig: the free is ordered behind anything on the stream)
    morph_drop(c);  // (either kind of set: an upload replaces whatever the rig holds)
    if (n_targets == 0) return GLRTX_OK;
    if (int rc = dev_upload(c, c->sk.morph, deltas, (size_t)n_targets * n_vert * skin::kDeltaWords * sizeof(float))) return rc;
    c->sk.n_targets = n_targets;
    return GLRTX_OK;
}

int glrtx_upload_morph_targets_sparse(glrtx_ctx *c, const uint64_t *offsets, const uint32_t *vertex, const float *deltas, int n_targets, size_t n_vert) {
    const char *fn = "glrtx_upload_morph_targets_sparse";
    if (!c) return GLRTX_EINVAL;
    if (!c->have_scene || c->sk.n_bones == 0) return fail(c, GLRTX_EINVAL, "%s: no rig uploaded (glrtx_upload_rig)", fn);
    if (n_vert != c->rf.n_vert) return fail(c, GLRTX_EINVAL, "%s: %zu vertices, the rig has %zu", fn, n_vert, c->rf.n_vert);
    if (int rc = sparse_check(c, offsets, vertex, deltas, n_targets, n_vert, fn)) return rc;
    std::vector<unsigned> row;
    std::vector<float4> entry;
    if (n_targets > 0) sparse_index(offsets, vertex, deltas, n_targets, n_vert, row, entry);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (as glrtx_upload_rig: the frees are ordered behind anything on the stream)
    morph_drop(c);
    if (n_targets == 0) return GLRTX_OK;
    if (int rc = dev_upload(c, c->sk.srow, row.data(), row.size() * sizeof(unsigned))) return rc;
    if (int rc = dev_upload(c, c->sk.sent, entry.data(), entry.size() * sizeof(float4))) return rc;
    c->sk.n_targets = n_targets;
    c->sk.sparse = true;
    c->sk.nnz = entry.size() / 2;
    return GLRTX_OK;
}

int glrtx_pose(glrtx_ctx *c, const float *matrices, int n_bones) {
    const char *fn = "glrtx_pose";
    if (int rc = pose_check(c, fn)) return rc;
    if (n_bones != c->sk.n_bones) return fail(c, GLRTX_EINVAL, "%s: %d matrices, the rig has %d bones", fn, n_bones, c->sk.n_bones);
    if (!matrices) return fail(c, GLRTX_EINVAL, "%s: NULL matrices", fn);
    if (!all_finite(matrices, (size_t)n_bones * 12)) return fail(c, GLRTX_EINVAL, "%s: a matrix entry is not finite", fn);
    return pose_move(c, PoseLaunch::kSkin, 0, matrices, nullptr, 0);
}

int glrtx_pose_morph(glrtx_ctx *c, const float *matrices, int n_bones, const float *morph_weights, int n_targets) {
    return deform_pose(c, matrices, n_bones, morph_weights, n_targets, 0, "glrtx_pose_morph");
}

int glrtx_pose_dualquat(glrtx_ctx *c, const float *dualquats, int n_bones, const float *morph_weights, int n_targets) {
    return deform_pose(c, dualquats, n_bones, morph_weights, n_targets, 1, "glrtx_pose_dualquat");
}

int glrtx_debug_skin(const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *matrices, int n_bones, float *vert_out) {
    const char *fn = "glrtx_debug_skin";
    if (int rc = rig_check(nullptr, rest, n_vert, bones4, weights4, n_bones, fn)) return rc;
    if (!matrices || (n_vert > 0 && !vert_out)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n_vert == 0) return GLRTX_OK;
    return PoseScratch(PoseLaunch::kSkin, 0, rest, n_vert, bones4, weights4, matrices, n_bones).run(vert_out, fn);
}

int glrtx_debug_deform(const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                       const float *deltas, const float *morph_weights, int n_targets, float *vert_out) {
    const char *fn = "glrtx_debug_deform";
    if (int rc = rig_check(nullptr, rest, n_vert, bones4, weights4, n_bones, fn)) return rc;
    if (mode != 0 && mode != 1) return fail(nullptr, GLRTX_EINVAL, "%s: mode %d (0: matrices, 1: dual quaternions)", fn, mode);
    if (int rc = morph_check(nullptr, morph_weights, n_targets, fn)) return rc;
    if (!bone_data || (n_vert > 0 && (!vert_out || (n_targets > 0 && !deltas)))) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n_vert == 0) return GLRTX_OK;
    PoseScratch s(PoseLaunch::kDeform, mode, rest, n_vert, bones4, weights4, bone_data, n_bones);
    if (n_targets > 0) s.L.deform.deltas = s.alloc<float2>((size_t)n_targets * n_vert * skin::kDeltaWords * sizeof(float), deltas);
    morph_list(s.L.deform.morph, morph_weights, n_targets);
    return s.run(vert_out, fn);
}

int glrtx_debug_deform_sparse(const float *rest, size_t n_vert, const int32_t *bones4, const float *weights4, const float *bone_data, int n_bones, int mode,
                              const uint64_t *offsets, const uint32_t *vertex, const float *deltas, const float *morph_weights, int n_targets, float *vert_out) {
    const char *fn = "glrtx_debug_deform_sparse";
    if (int rc = rig_check(nullptr, rest, n_vert, bones4, weights4, n_bones, fn)) return rc;
    if (mode != 0 && mode != 1) return fail(nullptr, GLRTX_EINVAL, "%s: mode %d (0: matrices, 1: dual quaternions)", fn, mode);
    if (int rc = sparse_check(nullptr, offsets, vertex, deltas, n_targets, n_vert, fn)) return rc;
    if (int rc = morph_check(nullptr, morph_weights, n_targets, fn, GLRTX_MAX_SPARSE_MORPH_TARGETS)) return rc;
    if (!bone_data || (n_vert > 0 && !vert_out)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n_vert == 0) return GLRTX_OK;
    std::vector<unsigned> row;
    std::vector<float4> entry;
    std::vector<float> tab;
    sparse_index(offsets, vertex, deltas, n_targets, n_vert, row, entry);
    sparse_weights(tab, morph_weights, n_targets);
    PoseScratch s(PoseLaunch::kSparse, mode, rest, n_vert, bones4, weights4, bone_data, n_bones);
    skin::SparseArgs &a = s.L.sparse;
    a.row = s.alloc<unsigned>(row.size() * sizeof(unsigned), row.data());
    a.entry = s.alloc<float4>(std::max<size_t>(entry.size(), 2) * sizeof(float4), entry.empty() ? nullptr : entry.data());  // (the hook always runs the sparse kernel)
    a.weight = s.alloc<float>(std::max<size_t>(tab.size(), 1) * sizeof(float), tab.empty() ? nullptr : tab.data());
    a.n_targets = n_targets;
    return s.run(vert_out, fn);
}

// Device time of the skinning kernel by itself, as glrtx_debug_reweight_burst measures its pass: the rig with the matrices of the last glrtx_pose, into the
// context's vertex buffer -- which holds exactly that already, so nothing changes.
int glrtx_debug_skin_burst(glrtx_ctx *c, int reps, float *ms_per_launch) {
    const char *fn = "glrtx_debug_skin_burst";
    if (!c || !ms_per_launch || reps < 1) return GLRTX_EINVAL;
    const size_t n_vert = c->rf.n_vert;
    if (!c->have_scene || c->sk.n_bones == 0 || c->rf.vert.bytes < n_vert * skin::kVertexWords * sizeof(float))
        return fail(c, GLRTX_EINVAL, "%s: no rig uploaded, or no glrtx_pose yet", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    const PoseLaunch L(PoseLaunch::kSkin, 0, c->sk.rest.p, c->sk.rig.p, c->sk.pose.p, c->rf.vert.p, n_vert);
    return burst_time(c, reps, ms_per_launch, [&] { pose_launch(L, c->stream); return GLRTX_OK; });
}

// Device time of the deform kernel by itself, as glrtx_debug_skin_burst: the last glrtx_pose_morph / glrtx_pose_dualquat launch again (whichever kernel it
// ran), into the context's vertex buffer -- which holds exactly that already, unless another call has written it since.
int glrtx_debug_deform_burst(glrtx_ctx *c, int reps, float *ms_per_launch) {
    const char *fn = "glrtx_debug_deform_burst";
    if (!c || !ms_per_launch || reps < 1) return GLRTX_EINVAL;
    if (!c->have_scene || c->sk.n_bones == 0 || c->sk.last.kernel == PoseLaunch::kNone)
        return fail(c, GLRTX_EINVAL, "%s: no rig uploaded, or no glrtx_pose_morph / glrtx_pose_dualquat yet", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return burst_time(c, reps, ms_per_launch, [&] { pose_launch(c->sk.last, c->stream); return GLRTX_OK; });
}

namespace {

int trace_check(glrtx_ctx *c, const void *rays, size_t n, const void *hits, int flags, const char *fn) {
    if (!c) return GLRTX_EINVAL;
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (flags != GLRTX_TRACE_CLOSEST && flags != GLRTX_TRACE_ANY) return fail(c, GLRTX_EINVAL, "%s: unknown flags %d", fn, flags);
    if (n >= ((size_t)1 << 31)) return fail(c, GLRTX_EINVAL, "%s: %zu rays (at most 2^31 - 1)", fn, n);
    if (n > 0 && (!rays || !hits)) return fail(c, GLRTX_EINVAL, "%s: NULL buffer", fn);
    return GLRTX_OK;
}

// One query launch on the context's stream (query.hip.h): the tree kernel with the node layout the wavefront kernel would walk, or the list scan on a vine.
// A persistent grid: as many workgroups as are resident on the device at once, fewer when the batch has fewer rays.
int trace_launch(glrtx_ctx *c, const void *rays, void *hits, size_t n, int flags) {
    const bool vine = c->sc.n_vine > 0, any = flags == GLRTX_TRACE_ANY;
    const int fetch = wgwf_fetch(c, vine);
    const int lds_stack = 2 * c->sc.stack_entries * kBlockThreads * (int)sizeof(int), lds_ranks = c->sc.n_crank * (int)sizeof(uint2);
    // the compact records where the wavefront kernel would walk them; GLRTX_COMPACT_NODES=0/1 (read at every call) forces either layout -- the query has no
    // pair-cooperative fetch, so 1 holds whatever the size of the tree, as long as the rank table fits in LDS
    bool compact = wgwf_compact(c, vine, fetch);
    if (const char *v = std::getenv("GLRTX_COMPACT_NODES")) compact = std::atoi(v) != 0 && !vine && c->sc.n_crank > 0;
    compact = compact && lds_stack + lds_ranks <= 160 * 1024;
    c->st.node_layout_last = compact ? 1 : 0;  // (as the render path records it: the tests read which kernel a query ran)
    using Kernel = void (*)(const query::Args);
    const Kernel kernel = vine ? (any ? (Kernel)query::trace_vine<true> : (Kernel)query::trace_vine<false>)
                        : compact ? (any ? (Kernel)query::trace_tree<true, true> : (Kernel)query::trace_tree<false, true>)
                                  : (any ? (Kernel)query::trace_tree<true, false> : (Kernel)query::trace_tree<false, false>);
    const int lds = vine ? 0 : lds_stack + (compact ? lds_ranks : 0);
    if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    int per_cu = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlockThreads, lds));
    per_cu = std::max(per_cu, 1);
    const size_t needed = (n + kBlockThreads - 1) / kBlockThreads;
    const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)per_cu * (size_t)c->n_cu, needed));
    if (int rc = ensure(c, c->qcounter, sizeof(unsigned))) return rc;
    HIP_TRY(c, hipMemsetAsync(c->qcounter.p, 0, sizeof(unsigned), c->stream));
    query::Args a;
    a.sc = c->sc;
    a.rays = (const float4 *)rays;
    a.hits = (float4 *)hits;
    a.wire = (const int *)c->qwire.p;
    a.counter = (unsigned *)c->qcounter.p;
    a.n = (unsigned)n;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), lds, c->stream, a);
    HIP_TRY(c, hipGetLastError());
    return GLRTX_OK;
}

}  // namespace

int glrtx_trace_rays(glrtx_ctx *c, const float *rays, size_t n, float *hits_out, int flags) {
    if (int rc = trace_check(c, rays, n, hits_out, flags, "glrtx_trace_rays")) return rc;
    if (n == 0) return GLRTX_OK;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure(c, c->qrays, n * 8 * sizeof(float))) return rc;
    if (int rc = ensure(c, c->qhits, n * 4 * sizeof(float))) return rc;
    HIP_TRY(c, hipMemcpyAsync(c->qrays.p, rays, n * 8 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (int rc = trace_launch(c, c->qrays.p, c->qhits.p, n, flags)) return rc;
    HIP_TRY(c, hipMemcpyAsync(hits_out, c->qhits.p, n * 4 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return GLRTX_OK;
}

int glrtx_trace_rays_device(glrtx_ctx *c, const void *dev_rays, size_t n, void *dev_hits, int flags) {
    if (int rc = trace_check(c, dev_rays, n, dev_hits, flags, "glrtx_trace_rays_device")) return rc;
    if (n == 0) return GLRTX_OK;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return trace_launch(c, dev_rays, dev_hits, n, flags);
}

int glrtx_debug_read_scene(glrtx_ctx *c, int which, void *dst, size_t capacity_bytes, size_t *bytes_out) {
    if (!c) return GLRTX_EINVAL;
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "glrtx_debug_read_scene: no scene uploaded");
    if (which < 0 || which > GLRTX_SCENE_ROOT) return fail(c, GLRTX_EINVAL, "glrtx_debug_read_scene: no buffer %d", which);
    const void *src[5] = {c->forks.p, c->cnodes.p, c->nrms.p, c->lights.p, c->vine.p};
    int32_t root[12];
    size_t n = which == GLRTX_SCENE_ROOT ? sizeof root : c->rf.bytes[which];
    if (bytes_out) *bytes_out = n;
    if (!dst) return GLRTX_OK;
    if (capacity_bytes < n) return fail(c, GLRTX_EINVAL, "glrtx_debug_read_scene: %zu bytes, room for %zu", n, capacity_bytes);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (which == GLRTX_SCENE_ROOT) {
        std::memcpy(&root[0], &c->sc.root_lo, 16);
        std::memcpy(&root[4], &c->sc.root_hi, 16);
        root[8] = c->sc.root_boxed; root[9] = c->sc.vine_uniform; root[10] = c->sc.root_ref; root[11] = c->rf.a.n_vine;
        std::memcpy(dst, root, sizeof root);
    } else if (n) {
        HIP_TRY(c, hipMemcpy(dst, src[which], n, hipMemcpyDeviceToHost));
    }
    return GLRTX_OK;
}

// Host-only validation of a wire-format scene (no device needed): the same checks and repacking
// glrtx_upload_scene performs.  Outputs may be NULL.
int glrtx_check_scene(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat,
                      const float *light, size_t n_light, const float *bvh, size_t n_nodes, int *n_fork_out,
                      int *stack_entries_out) {
    Packed P;
    if (int rc = pack_scene(nullptr, &g_create_error, P, vert, n_vert, tri, n_tri, mat, n_mat, light, n_light, bvh, n_nodes)) return rc;
    if (n_fork_out) *n_fork_out = (int)(P.forks.size() / 4);
    if (stack_entries_out) *stack_entries_out = P.stack_need;
    return GLRTX_OK;
}

// Host-only: the fork records as the device will see them (16 floats each: {minL, refL} {maxL, refR} {minR, -} {maxR, -}; refs as
// int bit patterns: a ref < 0 is the record ~id of a leaf, ids from 1 in traversal order, ref -1 = id 0 the never-hit record an absent child refers to;
// leaf pairs have no fork record -- include/glrtx.h), for tests that replay
// trav_step's push / pop rules on the packed tree and compare the deepest stack they reach with stack_entries.
int glrtx_debug_pack_forks(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat, const float *light,
                           size_t n_light, const float *bvh, size_t n_nodes, float *forks_out, size_t capacity_forks, int *n_fork_out,
                           int *root_ref_out, int *stack_entries_out) {
    Packed P;
    if (int rc = pack_scene(nullptr, &g_create_error, P, vert, n_vert, tri, n_tri, mat, n_mat, light, n_light, bvh, n_nodes)) return rc;
    const size_t nf = P.forks.size() / 4;
    if (n_fork_out) *n_fork_out = (int)nf;
    if (root_ref_out) *root_ref_out = P.root_ref;
    if (stack_entries_out) *stack_entries_out = P.stack_need;
    if (forks_out) {
        if (capacity_forks < nf) return pfail(nullptr, &g_create_error, GLRTX_EINVAL, "glrtx_debug_pack_forks: %zu forks, room for %zu", nf, capacity_forks);
        std::memcpy(forks_out, P.forks.data(), nf * 16 * sizeof(float));
    }
    return GLRTX_OK;
}

// Host-only: the compact node array, its rank table and the 64-byte leaf records (include/glrtx.h), for tests that walk both layouts.
int glrtx_debug_pack_compact(const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat, const float *light,
                             size_t n_light, const float *bvh, size_t n_nodes, float *records_out, size_t capacity_positions, int *n_positions_out,
                             uint32_t *ranks_out, size_t capacity_words, float *leaves_out, size_t capacity_ids, int *n_ids_out) {
    Packed P;
    if (int rc = pack_scene(nullptr, &g_create_error, P, vert, n_vert, tri, n_tri, mat, n_mat, light, n_light, bvh, n_nodes)) return rc;
    const size_t np = P.cnodes.size() / 3, nw = 2 * P.cranks.size(), ni = P.tris.size() / 4;
    if (n_positions_out) *n_positions_out = (int)np;
    if (n_ids_out) *n_ids_out = (int)ni;
    if ((records_out && capacity_positions < np) || (ranks_out && capacity_words < nw) || (leaves_out && capacity_ids < ni))
        return pfail(nullptr, &g_create_error, GLRTX_EINVAL, "glrtx_debug_pack_compact: %zu positions, %zu rank words, %zu leaf ids: an output is too small", np, nw, ni);
    if (records_out) std::memcpy(records_out, P.cnodes.data(), np * 12 * sizeof(float));
    if (ranks_out) std::memcpy(ranks_out, P.cranks.data(), nw * sizeof(uint32_t));
    if (leaves_out) std::memcpy(leaves_out, P.tris.data(), ni * 16 * sizeof(float));
    return GLRTX_OK;
}

int glrtx_build_lbvh(glrtx_ctx *c, const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out, int *max_depth_out,
                     float *build_ms_out) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!vert || !tri || !nodes_out || n_tri == 0 || n_vert == 0) return fail(c, GLRTX_EINVAL, "glrtx_build_lbvh: empty input");
    if (2 * n_tri - 1 > ((size_t)1 << 24) || n_vert > (size_t)INT32_MAX / 16)
        return fail(c, GLRTX_EINVAL, "glrtx_build_lbvh: %zu triangles: node indices must fit a float (2^24)", n_tri);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_nodes = 2 * n_tri - 1;
    int rc;
    if ((rc = dev_upload(c, c->bvhVert, vert, n_vert * 15 * sizeof(float)))) return rc;
    if ((rc = dev_upload(c, c->bvhTri, tri, n_tri * 4 * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->bvhNodes, n_nodes * 9 * sizeof(float)))) return rc;
    int depth = 0, bad = 0;
    HIP_TRY(c, hipEventRecord(c->tm0, c->stream));
    HIP_TRY(c, lbvh::build(c->stream, (const float *)c->bvhVert.p, (unsigned)n_vert, (const float *)c->bvhTri.p, (unsigned)n_tri,
                           (float *)c->bvhNodes.p, c->bvhWs, &depth, &bad));
    HIP_TRY(c, hipEventRecord(c->tm1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->tm1));
    if (bad) return fail(c, GLRTX_ESCENE, "glrtx_build_lbvh: a triangle references a vertex out of range");
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->tm0, c->tm1));
    HIP_TRY(c, hipMemcpy(nodes_out, c->bvhNodes.p, n_nodes * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (max_depth_out) *max_depth_out = depth;
    if (build_ms_out) *build_ms_out = ms;
    return depth < 63 ? GLRTX_OK : fail(c, GLRTX_EDEPTH, "glrtx_build_lbvh: tree depth %d exceeds the 64-entry traversal stack", depth);
}

int glrtx_build_bvh_sah(glrtx_ctx *c, const float *vert, size_t n_vert, const float *tri, size_t n_tri, float *nodes_out, int *max_depth_out,
                     float *build_ms_out) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!vert || !tri || !nodes_out || n_tri == 0 || n_vert == 0) return fail(c, GLRTX_EINVAL, "glrtx_build_bvh_sah: empty input");
    if (2 * n_tri - 1 > ((size_t)1 << 24) || n_vert > (size_t)INT32_MAX / 16)
        return fail(c, GLRTX_EINVAL, "glrtx_build_bvh_sah: %zu triangles: node indices must fit a float (2^24)", n_tri);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t n_nodes = 2 * n_tri - 1;
    int rc;
    if ((rc = dev_upload(c, c->bvhVert, vert, n_vert * 15 * sizeof(float)))) return rc;
    if ((rc = dev_upload(c, c->bvhTri, tri, n_tri * 4 * sizeof(float)))) return rc;
    if ((rc = ensure(c, c->bvhNodes, n_nodes * 9 * sizeof(float)))) return rc;
    int depth = 0, bad = 0;
    HIP_TRY(c, hipEventRecord(c->tm0, c->stream));
    HIP_TRY(c, sahl::build(c->stream, (const float *)c->bvhVert.p, (unsigned)n_vert, (const float *)c->bvhTri.p, (unsigned)n_tri,
                           (float *)c->bvhNodes.p, c->bvhWs, &depth, &bad, nullptr));
    HIP_TRY(c, hipEventRecord(c->tm1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->tm1));
    if (bad) return fail(c, GLRTX_ESCENE, "glrtx_build_bvh_sah: a triangle references a vertex out of range");
    float ms = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&ms, c->tm0, c->tm1));
    HIP_TRY(c, hipMemcpy(nodes_out, c->bvhNodes.p, n_nodes * 9 * sizeof(float), hipMemcpyDeviceToHost));
    if (max_depth_out) *max_depth_out = depth;
    if (build_ms_out) *build_ms_out = ms;
    return depth < 63 ? GLRTX_OK : fail(c, GLRTX_EDEPTH, "glrtx_build_bvh_sah: tree depth %d exceeds the 64-entry traversal stack", depth);
}

int glrtx_upload_spheres(glrtx_ctx *c, const float *spheres, size_t n_spheres) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (n_spheres && !spheres) return fail(c, GLRTX_EINVAL, "glrtx_upload_spheres: NULL buffer with non-zero count");
    if (n_spheres > (size_t)kMaxSpheres) return fail(c, GLRTX_EINVAL, "glrtx_upload_spheres: at most %d spheres (they are tested one by one)", kMaxSpheres);
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "glrtx_upload_spheres: upload the scene (materials) first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    std::vector<float4> sp(n_spheres);
    std::vector<int> mt(n_spheres);
    for (size_t k = 0; k < n_spheres; k++) {
        const float *r = spheres + 5 * k;
        if (!(r[3] > 0.0f)) return fail(c, GLRTX_ESCENE, "sphere %zu: radius %g is not positive", k, r[3]);
        if (!(r[4] >= 0.0f) || (size_t)r[4] >= (size_t)c->n_mat) return fail(c, GLRTX_ESCENE, "sphere %zu: material %g out of range", k, r[4]);
        sp[k] = make_float4(r[0], r[1], r[2], r[3]);
        mt[k] = (int)r[4];
    }
    int rc;
    if ((rc = dev_upload(c, c->spheres, sp.data(), n_spheres * sizeof(float4)))) return rc;
    if ((rc = dev_upload(c, c->sphereMat, mt.data(), n_spheres * sizeof(int)))) return rc;
    c->n_spheres = (int)n_spheres;
    return GLRTX_OK;
}

int glrtx_upload_textures(glrtx_ctx *c, const glrtx_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *material_texture,
                          size_t n_mat) {
    const char *fn = "glrtx_upload_textures";
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (n_tex == 0) {  // unbind: the next launch is routed as before (the buffers stay until the context goes)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->n_tex = 0;
        c->have_maps = false;
        c->have_cut = false;
        c->have_emit = false;
        return GLRTX_OK;
    }
    if (n_mat != (size_t)c->n_mat) return fail(c, GLRTX_EINVAL, "%s: %zu bindings, the scene has %d materials", fn, n_mat, c->n_mat);
    if (!material_texture) return fail(c, GLRTX_EINVAL, "%s: NULL material_texture", fn);
    const std::string bad = glrt_detail::texture_set_error(reinterpret_cast<const glrt_detail::TexRecord *>(tex), n_tex, texels, texel_bytes);
    if (!bad.empty()) return fail(c, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (also behind every launch that reads the materials or a set bound before)
    std::vector<float4> m0(3 * n_mat);
    HIP_TRY(c, hipMemcpy(m0.data(), c->mats.p, m0.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < n_mat; m++) {
        const int32_t k = material_texture[m];
        if (k < -1 || (k >= 0 && (size_t)k >= n_tex)) return fail(c, GLRTX_EINVAL, "%s: material %zu is bound to texture %d of %zu", fn, m, k, n_tex);
        int type;
        std::memcpy(&type, &m0[3 * m].w, 4);
        if (k >= 0 && type != 2) return fail(c, GLRTX_EINVAL, "%s: material %zu is bound to texture %d and is not diffuse (type %d)", fn, m, k, type);
    }
    // used bytes of the blob only: the last texel of the texture that reaches furthest
    size_t used = 0;
    for (size_t k = 0; k < n_tex; k++)
        used = std::max(used, (size_t)tex[k].offset + (size_t)tex[k].width * (size_t)tex[k].height * glrt_detail::tex_texel_bytes(tex[k].format));
    // fresh buffers first, the context's own replaced only once all four are filled: a failure leaves the bound set as it was
    DevBuf d, t, st, b;
    int rc;
    if ((rc = dev_upload(c, d, tex, n_tex * sizeof(glrtx_texture))) || (rc = dev_upload(c, t, texels, used)) ||
        (rc = dev_upload(c, st, c->scene_st.data(), c->scene_st.size() * sizeof(float))) || (rc = dev_upload(c, b, material_texture, n_mat * sizeof(int32_t)))) {
        dev_free(d); dev_free(t); dev_free(st); dev_free(b);
        return rc;
    }
    dev_free(c->texDesc); dev_free(c->texTexels); dev_free(c->texSt); dev_free(c->texBind);
    c->have_maps = false;  // (glrtx_bind_material_maps: a new set invalidates the indices)
    c->have_cut = false;   // (glrtx_bind_cutouts: likewise)
    c->have_emit = false;  // (glrtx_bind_emission_maps: likewise)
    c->tex_format.resize(n_tex);
    for (size_t k = 0; k < n_tex; k++) c->tex_format[k] = tex[k].format;
    c->texDesc = d; c->texTexels = t; c->texSt = st; c->texBind = b;
    c->n_tex = (int)n_tex;
    return GLRTX_OK;
}

int glrtx_debug_texture_lookup(const glrtx_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const float *st, size_t n,
                               float *rgb_out) {
    const char *fn = "glrtx_debug_texture_lookup";
    if (n_tex == 0 || (n && (!which || !st || !rgb_out))) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer or no texture", fn);
    if (n > (size_t)INT32_MAX / 4) return fail(nullptr, GLRTX_EINVAL, "%s: too many lookups", fn);
    const std::string bad = glrt_detail::texture_set_error(reinterpret_cast<const glrt_detail::TexRecord *>(tex), n_tex, texels, texel_bytes);
    if (!bad.empty()) return fail(nullptr, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    for (size_t i = 0; i < n; i++)
        if (which[i] < 0 || (size_t)which[i] >= n_tex) return fail(nullptr, GLRTX_EINVAL, "%s: lookup %zu names texture %d of %zu", fn, i, which[i], n_tex);
    if (n == 0) return GLRTX_OK;
    DebugScratch s;
    TexSet ts{};
    ts.desc = s.alloc<TexDesc>(n_tex * sizeof(glrtx_texture), tex);
    ts.texels = s.alloc<unsigned char>(texel_bytes, texels);
    ts.n_tex = (int)n_tex;
    const int *d_which = s.alloc<int>(n * sizeof(int), which);
    const float *d_st = s.alloc<float>(2 * n * sizeof(float), st);
    float *d_out = s.alloc<float>(3 * n * sizeof(float));
    if (s.ok()) {
        hipLaunchKernelGGL(tex_lookup_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ts, d_which, d_st, (unsigned)n, d_out);
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(rgb_out, d_out, 3 * n * sizeof(float));
    return s.result(GLRTX_OK, fn);
}

// ---- material maps (include/glrtx.h "Material maps"; maps.hip.h)
static_assert(sizeof(glrtx_material_map) == sizeof(MapRec) && sizeof(MapRec) == 16, "one map record on the wire and the device");
static_assert(GLRTX_MAP_ALPHA_MIN == MAP_ALPHA_MIN && GLRTX_MAP_RECORD_FLOATS == kMapRecordFloats, "material map constants");

int glrtx_bind_material_maps(glrtx_ctx *c, const glrtx_material_map *maps, size_t n_mat) {
    const char *fn = "glrtx_bind_material_maps";
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!maps || n_mat == 0) {  // unbind: the next launch runs the textured kernels as before (the buffer stays until the context goes)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->have_maps = false;
        return GLRTX_OK;
    }
    if (!c->have_scene || c->n_tex == 0) return fail(c, GLRTX_EINVAL, "%s: no texture set is bound (call glrtx_upload_textures first)", fn);
    if (n_mat != (size_t)c->n_mat) return fail(c, GLRTX_EINVAL, "%s: %zu records, the scene has %d materials", fn, n_mat, c->n_mat);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (also behind every launch that reads the materials or the maps bound before)
    std::vector<float4> m0(3 * n_mat);
    HIP_TRY(c, hipMemcpy(m0.data(), c->mats.p, m0.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < n_mat; m++) {
        const glrtx_material_map &r = maps[m];
        int type;
        std::memcpy(&type, &m0[3 * m].w, 4);
        for (int which = 0; which < 2; which++) {
            const int32_t k = which ? r.roughness : r.normal;
            const char *what = which ? "roughness" : "normal";
            if (k < -1 || k >= c->n_tex) return fail(c, GLRTX_EINVAL, "%s: material %zu: %s map %d of %d textures", fn, m, what, k, c->n_tex);
            if (k >= 0 && c->tex_format[(size_t)k] == GLRTX_TEX_RGBA8_SRGB)
                return fail(c, GLRTX_EINVAL, "%s: material %zu: %s map %d has format GLRTX_TEX_RGBA8_SRGB (a map holds vectors, not colours)", fn, m, what, k);
        }
        if (r.normal >= 0 && type != 2 && type != 3)
            return fail(c, GLRTX_EINVAL, "%s: material %zu has a normal map and is neither diffuse nor conductor (type %d)", fn, m, type);
        if (r.roughness >= 0 && type != 3) return fail(c, GLRTX_EINVAL, "%s: material %zu has a roughness map and is not a conductor (type %d)", fn, m, type);
        if (!std::isfinite(r.normal_scale)) return fail(c, GLRTX_EINVAL, "%s: material %zu: normal_scale is not finite", fn, m);
        if (r.reserved != 0) return fail(c, GLRTX_EINVAL, "%s: material %zu: reserved is %d, not 0", fn, m, r.reserved);
    }
    DevBuf b;  // a fresh buffer first: a failure leaves the bound maps as they were
    if (int rc = dev_upload(c, b, maps, n_mat * sizeof(glrtx_material_map))) { dev_free(b); return rc; }
    dev_free(c->texMaps);
    c->texMaps = b;
    c->have_maps = true;
    return GLRTX_OK;
}

int glrtx_debug_map_normal(const float *records, size_t n, float scale, float *normal_out) {
    const char *fn = "glrtx_debug_map_normal";
    if (n && (!records || !normal_out)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n > (size_t)INT32_MAX / kMapRecordFloats) return fail(nullptr, GLRTX_EINVAL, "%s: too many records", fn);
    if (n == 0) return GLRTX_OK;
    DebugScratch s;
    const float *d_rec = s.alloc<float>(kMapRecordFloats * n * sizeof(float), records);
    float *d_out = s.alloc<float>(3 * n * sizeof(float));
    if (s.ok()) {
        hipLaunchKernelGGL(map_normal_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, d_rec, (unsigned)n, scale, d_out);
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(normal_out, d_out, 3 * n * sizeof(float));
    return s.result(GLRTX_OK, fn);
}

// ---- cutouts (include/glrtx.h "Cutouts"; texture.hip.h: cut_accepts, pt_kernel.hip.h: trav_step<.., CUT>)
static_assert(sizeof(glrtx_cutout) == sizeof(CutRec) && sizeof(CutRec) == 16, "one cutout record on the wire and the device");

int glrtx_bind_cutouts(glrtx_ctx *c, const glrtx_cutout *cut, size_t n_mat) {
    const char *fn = "glrtx_bind_cutouts";
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!cut || n_mat == 0) {  // unbind: the next launch is routed as before (the buffers stay until the context goes)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->have_cut = false;
        return GLRTX_OK;
    }
    if (!c->have_scene || c->n_tex == 0) return fail(c, GLRTX_EINVAL, "%s: no texture set is bound (call glrtx_upload_textures first)", fn);
    if (n_mat != (size_t)c->n_mat) return fail(c, GLRTX_EINVAL, "%s: %zu records, the scene has %d materials", fn, n_mat, c->n_mat);
    if (c->sc.n_vine > 0) return fail(c, GLRTX_EINVAL, "%s: the tree is a vine (the list scan has no cutout form)", fn);
    if (c->have_emit) return fail(c, GLRTX_EINVAL, "%s: emission maps are bound (glrtx_bind_emission_maps: the two do not combine yet; unbind them first)", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (also behind every launch that reads the materials or the records bound before)
    std::vector<float4> m0(3 * n_mat);
    HIP_TRY(c, hipMemcpy(m0.data(), c->mats.p, m0.size() * sizeof(float4), hipMemcpyDeviceToHost));
    for (size_t m = 0; m < n_mat; m++) {
        const glrtx_cutout &r = cut[m];
        int type;
        std::memcpy(&type, &m0[3 * m].w, 4);
        if (r.texture < -1 || r.texture >= c->n_tex) return fail(c, GLRTX_EINVAL, "%s: material %zu: cutout texture %d of %d textures", fn, m, r.texture, c->n_tex);
        if (r.channel < 0 || r.channel > 3) return fail(c, GLRTX_EINVAL, "%s: material %zu: channel %d is not 0 .. 3", fn, m, r.channel);
        if (!std::isfinite(r.cutoff)) return fail(c, GLRTX_EINVAL, "%s: material %zu: cutoff is not finite", fn, m);
        if (r.texture >= 0 && type != 2 && type != 3)
            return fail(c, GLRTX_EINVAL, "%s: material %zu has a cutout and is neither diffuse nor conductor (type %d)", fn, m, type);
        if (r.reserved != 0) return fail(c, GLRTX_EINVAL, "%s: material %zu: reserved is %d, not 0", fn, m, r.reserved);
    }
    // tri_cut: the record index of every device triangle, -1 where its material is not cut (record 0: the never-hit triangle)
    std::vector<int32_t> tri_cut(c->scene_mat.size(), -1);
    for (size_t t = 1; t < tri_cut.size(); t++) {
        const int32_t m = c->scene_mat[t];
        if (m >= 0 && (size_t)m < n_mat && cut[m].texture >= 0) tri_cut[t] = m;
    }
    DevBuf b, tc;  // fresh buffers first: a failure leaves the bound records as they were
    int rc;
    if ((rc = dev_upload(c, b, cut, n_mat * sizeof(glrtx_cutout))) || (rc = dev_upload(c, tc, tri_cut.data(), tri_cut.size() * sizeof(int32_t)))) {
        dev_free(b); dev_free(tc);
        return rc;
    }
    dev_free(c->cutRec); dev_free(c->cutTri);
    c->cutRec = b; c->cutTri = tc;
    c->have_cut = true;
    return GLRTX_OK;
}

const char *glrtx_debug_last_kernel(const glrtx_ctx *c) { return c ? c->last_kernel : ""; }

// ---- emission maps (include/glrtx.h "Emission maps"; texture.hip.h: EmitSet, pt_kernel.hip.h: shade_core<.., EMIT>)
int glrtx_bind_emission_maps(glrtx_ctx *c, const int32_t *material_emission, size_t n_mat) {
    const char *fn = "glrtx_bind_emission_maps";
    if (!c) return fail(nullptr, GLRTX_EINVAL, "%s: NULL context", fn);
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!material_emission || n_mat == 0) {  // unbind: the next launch is routed as before (the buffers stay until the context goes)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->have_emit = false;
        return GLRTX_OK;
    }
    std::vector<float4> m0(3 * (size_t)std::max(c->n_mat, 0));
    if (c->have_scene && !m0.empty()) {
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));  // (also behind every launch that reads the materials or the table bound before)
        HIP_TRY(c, hipMemcpy(m0.data(), c->mats.p, m0.size() * sizeof(float4), hipMemcpyDeviceToHost));
    }
    const std::string bad = glrt_detail::emission_bind_error(c->have_scene, (size_t)c->n_mat, (size_t)c->n_tex, c->have_cut, material_emission, n_mat, [&](size_t m) {
        int type;
        std::memcpy(&type, &m0[3 * m].w, 4);
        return type;
    });
    if (!bad.empty()) return fail(c, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    DevBuf b, st;  // fresh buffers first: a failure leaves the bound table as it was
    int rc;
    const float no_light[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (a scene without lights: the table is never read, the buffer is not empty)
    const bool lights = !c->scene_light_st.empty();
    if ((rc = dev_upload(c, b, material_emission, n_mat * sizeof(int32_t))) ||
        (rc = dev_upload(c, st, lights ? c->scene_light_st.data() : no_light, (lights ? c->scene_light_st.size() : 6) * sizeof(float)))) {
        dev_free(b); dev_free(st);
        return rc;
    }
    dev_free(c->emitMat); dev_free(c->emitSt);
    c->emitMat = b; c->emitSt = st;
    c->have_emit = true;
    return GLRTX_OK;
}

int glrtx_debug_light_emission(glrtx_ctx *c, const int32_t *lid, const float *u, size_t n, float *out) {
    const char *fn = "glrtx_debug_light_emission";
    if (!c) return fail(nullptr, GLRTX_EINVAL, "%s: NULL context", fn);
    if (!c->have_scene || c->n_tex == 0 || !c->have_emit) return fail(c, GLRTX_EINVAL, "%s: no emission maps are bound (glrtx_bind_emission_maps)", fn);
    if (n && (!lid || !u || !out)) return fail(c, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n > (size_t)INT32_MAX / 8) return fail(c, GLRTX_EINVAL, "%s: too many samples", fn);
    for (size_t i = 0; i < n; i++)
        if (lid[i] < 0 || lid[i] >= c->n_light) return fail(c, GLRTX_EINVAL, "%s: sample %zu names light %d of %d", fn, i, lid[i], c->n_light);
    if (n == 0) return GLRTX_OK;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    DebugScratch s;
    const int *d_lid = s.alloc<int>(n * sizeof(int), lid);
    const float *d_u = s.alloc<float>(2 * n * sizeof(float), u);
    float *d_out = s.alloc<float>(5 * n * sizeof(float));
    if (s.ok()) {
        const EmitSet es{(const int *)c->emitMat.p, (const float2 *)c->emitSt.p};
        hipLaunchKernelGGL(emit_light_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, tex_set(c), es, (const float4 *)c->lights.p, (const float4 *)c->mats.p,
                           d_lid, d_u, (unsigned)n, d_out);
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(out, d_out, 5 * n * sizeof(float));
    return s.result(GLRTX_OK, fn);
}

int glrtx_debug_texture_channel(const glrtx_texture *tex, size_t n_tex, const void *texels, size_t texel_bytes, const int32_t *which, const int32_t *channel,
                                const float *st, size_t n, float *value_out) {
    const char *fn = "glrtx_debug_texture_channel";
    if (n_tex == 0 || (n && (!which || !channel || !st || !value_out))) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer or no texture", fn);
    if (n > (size_t)INT32_MAX / 4) return fail(nullptr, GLRTX_EINVAL, "%s: too many lookups", fn);
    const std::string bad = glrt_detail::texture_set_error(reinterpret_cast<const glrt_detail::TexRecord *>(tex), n_tex, texels, texel_bytes);
    if (!bad.empty()) return fail(nullptr, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    for (size_t i = 0; i < n; i++) {
        if (which[i] < 0 || (size_t)which[i] >= n_tex) return fail(nullptr, GLRTX_EINVAL, "%s: lookup %zu names texture %d of %zu", fn, i, which[i], n_tex);
        if (channel[i] < 0 || channel[i] > 3) return fail(nullptr, GLRTX_EINVAL, "%s: lookup %zu names channel %d, not 0 .. 3", fn, i, channel[i]);
    }
    if (n == 0) return GLRTX_OK;
    DebugScratch s;
    TexSet ts{};
    ts.desc = s.alloc<TexDesc>(n_tex * sizeof(glrtx_texture), tex);
    ts.texels = s.alloc<unsigned char>(texel_bytes, texels);
    ts.n_tex = (int)n_tex;
    const int *d_which = s.alloc<int>(n * sizeof(int), which);
    const int *d_channel = s.alloc<int>(n * sizeof(int), channel);
    const float *d_st = s.alloc<float>(2 * n * sizeof(float), st);
    float *d_out = s.alloc<float>(n * sizeof(float));
    if (s.ok()) {
        hipLaunchKernelGGL(tex_channel_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ts, d_which, d_channel, d_st, (unsigned)n, d_out);
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(value_out, d_out, n * sizeof(float));
    return s.result(GLRTX_OK, fn);
}

}  // extern "C"

// ---- environment (glrtx_upload_environment, glrtx_set_environment_cfg, glrtx_debug_env_*; environment.hip.h)
namespace {
static_assert(sizeof(glrtx_env_cfg) == sizeof(glrt_detail::EnvCfg), "one environment configuration on the wire, the host and the device");
static_assert(GLRTX_ENV_ESCAPE == ENV_ESCAPE && GLRTX_ENV_SAMPLED == ENV_SAMPLED && glrt_detail::kEnvGridMax == kEnvGridMax, "environment constants");

// An environment on the device: the map's texels, the five tables, and the kernels' view of them
struct EnvDevice {
    DevBuf texels, row_q, row_alias, col_q, col_alias, cell_p;
    EnvArgs args{};
    void free_all() {
        for (DevBuf *b : {&texels, &row_q, &row_alias, &col_q, &col_alias, &cell_p}) dev_free(*b);
    }
};

// The configuration's part of EnvArgs, and the tables of the map at ed.texels: the weights kernel on `st`, Vose's method on the host, five uploads.
// weights_out (optional): the G * G cell weights.  The texels must be on the device already; on failure the caller frees ed.
int env_configure(glrtx_ctx *c, hipStream_t st, EnvDevice &ed, const glrtx_texture &map, const glrtx_env_cfg &cfg, float *weights_out) {
    EnvArgs &ea = ed.args;
    std::memcpy(&ea.desc, &map, sizeof ea.desc);
    ea.desc.offset = 0;
    ea.texels = (const unsigned char *)ed.texels.p;
    std::memcpy(ea.R, cfg.rotation, sizeof ea.R);
    std::memcpy(ea.scale, cfg.scale, sizeof ea.scale);
    ea.mode = cfg.mode;
    ea.p_env = cfg.light_pick;
    const int G = glrt_detail::env_grid(cfg.grid, map.width);
    ea.G = G;
    const size_t cells = (size_t)G * (size_t)G;
    DevBuf w;
    if (int rc = ensure(c, w, cells * sizeof(float))) return rc;
    hipLaunchKernelGGL(env_weights_kernel, dim3((unsigned)G, (unsigned)G), dim3(kEnvWeightThreads), 0, st, ea, (float *)w.p);
    std::vector<float> weights(cells);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipMemcpy(weights.data(), w.p, cells * sizeof(float), hipMemcpyDeviceToHost);
    dev_free(w);
    if (e != hipSuccess) return fail(c, GLRTX_EDEVICE, "env_weights_kernel: %s", hipGetErrorString(e));
    if (weights_out) std::memcpy(weights_out, weights.data(), cells * sizeof(float));
    const glrt_detail::EnvTables t = glrt_detail::env_tables(weights.data(), G);
    int rc;
    if ((rc = dev_upload(c, ed.row_q, t.row_q.data(), (size_t)G * sizeof(float))) || (rc = dev_upload(c, ed.row_alias, t.row_alias.data(), (size_t)G * sizeof(int32_t))) ||
        (rc = dev_upload(c, ed.col_q, t.col_q.data(), cells * sizeof(float))) || (rc = dev_upload(c, ed.col_alias, t.col_alias.data(), cells * sizeof(int32_t))) ||
        (rc = dev_upload(c, ed.cell_p, t.cell_p.data(), cells * sizeof(float))))
        return rc;
    ea.row_q = (const float *)ed.row_q.p; ea.row_alias = (const int *)ed.row_alias.p;
    ea.col_q = (const float *)ed.col_q.p; ea.col_alias = (const int *)ed.col_alias.p;
    ea.cell_p = (const float *)ed.cell_p.p;
    return GLRTX_OK;
}

size_t env_map_bytes(const glrtx_texture &map) { return (size_t)map.width * (size_t)map.height * glrt_detail::tex_texel_bytes(map.format); }

// What the three debug hooks share: the refusals, the map and its tables on the current device
int env_debug_setup(const char *fn, EnvDevice &ed, const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, float *weights_out) {
    const std::string bad = glrt_detail::env_error(reinterpret_cast<const glrt_detail::TexRecord *>(map), texels, texel_bytes, reinterpret_cast<const glrt_detail::EnvCfg *>(cfg));
    if (!bad.empty()) return fail(nullptr, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    if (int rc = dev_upload(nullptr, ed.texels, (const unsigned char *)texels + map->offset, env_map_bytes(*map))) return rc;
    return env_configure(nullptr, nullptr, ed, *map, *cfg, weights_out);
}

// The bound environment replaced by ed (the stream is idle)
void env_adopt(glrtx_ctx *c, EnvDevice &ed, const glrtx_env_cfg &cfg, bool keep_texels) {
    if (!keep_texels) { dev_free(c->envTexels); c->envTexels = ed.texels; }
    dev_free(c->envRowQ); dev_free(c->envRowAlias); dev_free(c->envColQ); dev_free(c->envColAlias); dev_free(c->envCellP);
    c->envRowQ = ed.row_q; c->envRowAlias = ed.row_alias; c->envColQ = ed.col_q; c->envColAlias = ed.col_alias; c->envCellP = ed.cell_p;
    c->env = ed.args;
    c->env_cfg = cfg;
    c->have_env = true;
}
}  // namespace

extern "C" {
int glrtx_upload_environment(glrtx_ctx *c, const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg) {
    const char *fn = "glrtx_upload_environment";
    if (!c) return fail(nullptr, GLRTX_EINVAL, "%s: NULL context", fn);
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!map) {  // unbind: the next launch is routed as before (the buffers stay until the context goes or another map comes)
        HIP_TRY(c, hipSetDevice(c->device));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        c->have_env = false;
        return GLRTX_OK;
    }
    const std::string bad = glrt_detail::env_error(reinterpret_cast<const glrt_detail::TexRecord *>(map), texels, texel_bytes, reinterpret_cast<const glrt_detail::EnvCfg *>(cfg));
    if (!bad.empty()) return fail(c, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (also behind every launch that reads an environment bound before)
    // fresh buffers first, the context's own replaced only once all are filled: a failure leaves the bound environment as it was
    EnvDevice ed;
    int rc = dev_upload(c, ed.texels, (const unsigned char *)texels + map->offset, env_map_bytes(*map));
    if (!rc) rc = env_configure(c, c->stream, ed, *map, *cfg, nullptr);
    if (rc) { ed.free_all(); return rc; }
    env_adopt(c, ed, *cfg, false);
    return GLRTX_OK;
}

int glrtx_set_environment_cfg(glrtx_ctx *c, const glrtx_env_cfg *cfg) {
    const char *fn = "glrtx_set_environment_cfg";
    if (!c) return fail(nullptr, GLRTX_EINVAL, "%s: NULL context", fn);
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    const std::string bad = glrt_detail::env_error(nullptr, nullptr, 0, reinterpret_cast<const glrt_detail::EnvCfg *>(cfg), false);
    if (!bad.empty()) return fail(c, GLRTX_EINVAL, "%s: %s", fn, bad.c_str());
    if (!c->have_env) return fail(c, GLRTX_EINVAL, "%s: no environment is bound (glrtx_upload_environment)", fn);
    const glrtx_env_cfg &old = c->env_cfg;
    const bool rebuild = std::memcmp(old.scale, cfg->scale, sizeof old.scale) != 0 || glrt_detail::env_grid(old.grid, c->env.desc.width) != glrt_detail::env_grid(cfg->grid, c->env.desc.width);
    if (!rebuild) {  // mode, light_pick, rotation: kernel arguments of the next launch
        c->env.mode = cfg->mode;
        std::memcpy(c->env.R, cfg->rotation, sizeof c->env.R);
        c->env_cfg = *cfg;
        return GLRTX_OK;
    }
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    EnvDevice ed;
    ed.texels = c->envTexels;  // (borrowed: the map stays)
    glrtx_texture map;
    std::memcpy(&map, &c->env.desc, sizeof map);
    const int rc = env_configure(c, c->stream, ed, map, *cfg, nullptr);
    if (rc) { ed.texels = DevBuf{}; ed.free_all(); return rc; }
    env_adopt(c, ed, *cfg, true);
    return GLRTX_OK;
}

int glrtx_debug_env_weights(const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, float *weights_out, int32_t *grid_out) {
    const char *fn = "glrtx_debug_env_weights";
    if (!weights_out || !grid_out) return fail(nullptr, GLRTX_EINVAL, "%s: NULL output", fn);
    EnvDevice ed;
    const int rc = env_debug_setup(fn, ed, map, texels, texel_bytes, cfg, weights_out);
    if (!rc) *grid_out = ed.args.G;
    ed.free_all();
    return rc;
}

int glrtx_debug_env_sample(const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, const float *u, size_t n, float *out) {
    const char *fn = "glrtx_debug_env_sample";
    if (n && (!u || !out)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n > (size_t)INT32_MAX / 8) return fail(nullptr, GLRTX_EINVAL, "%s: too many samples", fn);
    EnvDevice ed;
    int rc = env_debug_setup(fn, ed, map, texels, texel_bytes, cfg, nullptr);
    if (!rc && n) {
        DebugScratch s;
        const float *d_u = s.alloc<float>(6 * n * sizeof(float), u);
        float *d_out = s.alloc<float>(8 * n * sizeof(float));
        if (s.ok()) {
            hipLaunchKernelGGL(env_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ed.args, d_u, (unsigned)n, d_out);
            s.e = hipGetLastError();
        }
        s.sync();
        s.download(out, d_out, 8 * n * sizeof(float));
        rc = s.result(GLRTX_OK, fn);
    }
    ed.free_all();
    return rc;
}

int glrtx_debug_env_eval(const glrtx_texture *map, const void *texels, size_t texel_bytes, const glrtx_env_cfg *cfg, const float *dir, size_t n, float *out) {
    const char *fn = "glrtx_debug_env_eval";
    if (n && (!dir || !out)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (n > (size_t)INT32_MAX / 4) return fail(nullptr, GLRTX_EINVAL, "%s: too many directions", fn);
    EnvDevice ed;
    int rc = env_debug_setup(fn, ed, map, texels, texel_bytes, cfg, nullptr);
    if (!rc && n) {
        DebugScratch s;
        const float *d_dir = s.alloc<float>(3 * n * sizeof(float), dir);
        float *d_out = s.alloc<float>(4 * n * sizeof(float));
        if (s.ok()) {
            hipLaunchKernelGGL(env_eval_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, ed.args, d_dir, (unsigned)n, d_out);
            s.e = hipGetLastError();
        }
        s.sync();
        s.download(out, d_out, 4 * n * sizeof(float));
        rc = s.result(GLRTX_OK, fn);
    }
    ed.free_all();
    return rc;
}

int glrtx_set_extensions(glrtx_ctx *c, int flags) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (flags & ~(GLRTX_EXT_DIELECTRIC | GLRTX_EXT_WHITTED | GLRTX_EXT_VOLUME)) return fail(c, GLRTX_EINVAL, "glrtx_set_extensions: unknown flag bits 0x%x", flags);
    static_assert(GLRTX_EXT_DIELECTRIC == EXT_DIELECTRIC && GLRTX_EXT_WHITTED == EXT_WHITTED, "extension flag values");
    c->ext_flags = flags;
    return GLRTX_OK;
}

// Volume grids: argument checks shared by glrtx_upload_volume and the lookup export.  Returns 0 (valid), 1 (remove: no grid), or a GLRTX_E* code.
static int check_volume(glrtx_ctx *c, const char *fn, const float *density, const float *temperature, int nx, int ny, int nz, const float *bmin,
                        const float *bmax, bool need_temperature) {
    if (nx < 0 || ny < 0 || nz < 0) return fail(c, GLRTX_EINVAL, "%s: negative grid dimension %d x %d x %d", fn, nx, ny, nz);
    if (!density || nx == 0 || ny == 0 || nz == 0) return 1;
    if ((long long)nx * ny * nz > (1ll << 29)) return fail(c, GLRTX_EINVAL, "%s: %d x %d x %d texels exceed 2^29 (32-bit texel offsets)", fn, nx, ny, nz);
    if (need_temperature && !temperature) return fail(c, GLRTX_EINVAL, "%s: NULL temperature grid with a density grid", fn);
    if (!bmin || !bmax) return fail(c, GLRTX_EINVAL, "%s: NULL bbox", fn);
    for (int k = 0; k < 3; k++) {
        const float e = bmax[k] - bmin[k];
        if (e == 0.0f || !std::isfinite(e))
            return fail(c, GLRTX_EINVAL, "%s: bbox has zero or non-finite extent on axis %c (%g .. %g)", fn, "xyz"[k], bmin[k], bmax[k]);
    }
    return 0;
}
static VolArgs vol_args(const float *density, const float *temperature, int nx, int ny, int nz, const float *bmin, const float *bmax, float density_max) {
    VolArgs v{};
    v.density = density; v.temperature = temperature;
    v.nx = nx; v.ny = ny; v.nz = nz;
    v.min_x = bmin[0]; v.min_y = bmin[1]; v.min_z = bmin[2];
    v.ext_x = bmax[0] - bmin[0]; v.ext_y = bmax[1] - bmin[1]; v.ext_z = bmax[2] - bmin[2];
    v.density_max = density_max;
    return v;
}

int glrtx_upload_volume(glrtx_ctx *c, const float *density, const float *temperature, int nx, int ny, int nz, const float bbox_min[3],
                        const float bbox_max[3], float density_max) {
    if (!c) return fail(nullptr, GLRTX_EINVAL, "glrtx_upload_volume: NULL context");
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    const int chk = check_volume(c, "glrtx_upload_volume", density, temperature, nx, ny, nz, bbox_min, bbox_max, true);
    if (chk < 0) return chk;
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));  // (a launch in flight may still read the old grids)
    if (chk == 1) {
        dev_free(c->volDensity); dev_free(c->volTemp);
        c->vol = VolArgs{};
        c->have_volume = false;
        return GLRTX_OK;
    }
    c->have_volume = false;
    const size_t bytes = (size_t)nx * ny * nz * sizeof(float);
    int rc;
    if ((rc = dev_upload(c, c->volDensity, density, bytes))) return rc;
    if ((rc = dev_upload(c, c->volTemp, temperature, bytes))) return rc;
    c->vol = vol_args((const float *)c->volDensity.p, (const float *)c->volTemp.p, nx, ny, nz, bbox_min, bbox_max, density_max);
    c->have_volume = true;
    return GLRTX_OK;
}

// Debug export: one synchronous kernel on the current device, host arrays in and out.
static int vmath_run(const char *fn, const float *in, size_t n_in, const float *grid, size_t n_grid, const VolArgs *v, float *out, size_t n_out, int op) {
    if (n_in == 0) return GLRTX_OK;
    if (n_in > (size_t)INT32_MAX / 4) return fail(nullptr, GLRTX_EINVAL, "%s: n = %zu too large", fn, n_in);
    DebugScratch s;
    const float *d_in = s.alloc<float>(n_in * sizeof(float), in);
    float *d_out = s.alloc<float>(n_out * sizeof(float));
    const float *d_grid = grid ? s.alloc<float>(n_grid * sizeof(float), grid) : nullptr;
    if (s.ok()) {
        if (v) {
            VolArgs va = *v;
            va.density = d_grid; va.temperature = d_grid;
            const int n = (int)n_out;
            hipLaunchKernelGGL(volume_lookup_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, va, d_in, n, d_out);
        } else {
            const int n = (int)n_in;
            hipLaunchKernelGGL(volume_math_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, op, d_in, n, d_out);
        }
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(out, d_out, n_out * sizeof(float));
    return s.result(GLRTX_OK, fn);
}

int glrtx_debug_volume_math(int op, const float *in, size_t n, float *out) {
    if (op < GLRTX_VMATH_LOG || op > GLRTX_VMATH_BLACKBODY) return fail(nullptr, GLRTX_EINVAL, "glrtx_debug_volume_math: unknown op %d", op);
    if (n && (!in || !out)) return fail(nullptr, GLRTX_EINVAL, "glrtx_debug_volume_math: NULL buffer");
    return vmath_run("glrtx_debug_volume_math", in, n, nullptr, 0, nullptr, out, op == GLRTX_VMATH_BLACKBODY ? 3 * n : n, op);
}

int glrtx_debug_volume_lookup(const float *grid, int nx, int ny, int nz, const float bbox_min[3], const float bbox_max[3], const float *pos,
                              size_t n, float *out) {
    const int chk = check_volume(nullptr, "glrtx_debug_volume_lookup", grid, nullptr, nx, ny, nz, bbox_min, bbox_max, false);
    if (chk < 0) return chk;
    if (chk == 1) return fail(nullptr, GLRTX_EINVAL, "glrtx_debug_volume_lookup: no grid");
    if (n && (!pos || !out)) return fail(nullptr, GLRTX_EINVAL, "glrtx_debug_volume_lookup: NULL buffer");
    const VolArgs v = vol_args(nullptr, nullptr, nx, ny, nz, bbox_min, bbox_max, 0.0f);
    return vmath_run("glrtx_debug_volume_lookup", pos, 3 * n, grid, (size_t)nx * ny * nz, &v, out, n, 0);
}

int glrtx_set_partition(glrtx_ctx *c, int rank, int world, int stripe_rows) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (world < 1 || rank < 0 || rank >= world || stripe_rows < 1)
        return fail(c, GLRTX_EINVAL, "glrtx_set_partition: bad rank/world/stripe %d/%d/%d", rank, world, stripe_rows);
    if (stripe_rows % kStripeQuantum != 0)  // whole 8x8 work tiles per stripe (pixel -> row mapping itself works for any stripe height)
        return fail(c, GLRTX_EINVAL, "glrtx_set_partition: stripe_rows must be a multiple of %d", kStripeQuantum);
    if (c->bound && c->width > 0 && owned_rows_of(c->height, rank, world, stripe_rows) > c->bound_rows)
        return fail(c, GLRTX_EINVAL, "glrtx_set_partition: the new partition does not fit the bound accumulator (%d rows); unbind it first", c->bound_rows);
    c->rank = rank; c->world = world; c->stripe = stripe_rows;
    if (c->width > 0) return glrtx_resize(c, c->width, c->height);
    return GLRTX_OK;
}

int glrtx_local_row_to_y(const glrtx_ctx *c, int r) {
    if (!c || r < 0 || r >= c->owned_rows) return -1;
    return ((r / c->stripe) * c->world + c->rank) * c->stripe + r % c->stripe;
}

int glrtx_resize(glrtx_ctx *c, int width, int height) {
    if (!c) return GLRTX_EINVAL;
    if (present_held(c)) return fail(c, GLRTX_EINVAL, "glrtx_resize: a presented image is still acquired (glrtx_present_release it first)");
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (width < 1 || height < 1 || width > 65536 || height > 65536) return fail(c, GLRTX_EINVAL, "glrtx_resize: bad size %dx%d", width, height);
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->pres.copy) HIP_TRY(c, hipStreamSynchronize(c->pres.copy));  // (the device images change their size: no copy may still read them)
    if (c->bound) {  // a caller-owned accumulator is bound: the new shape must fit it (nothing here can grow it)
        const int rows = owned_rows_of(height, c->rank, c->world, c->stripe);
        if ((size_t)width * sizeof(float4) > c->pitch_bytes || rows > c->bound_rows)
            return fail(c, GLRTX_EINVAL, "glrtx_resize: %dx%d (%d owned rows) does not fit the bound accumulator (%zu-byte rows, %d rows); unbind it first",
                        width, height, rows, c->pitch_bytes, c->bound_rows);
    }
    denoise_release(c);  // (the feature planes and the filter's images have the old shape; the stream is idle)
    c->mmM.drop(); dev_free(c->mmM_spare);  // (so has the moments plane: allocated again on its next use)
    c->rwC.drop();  // (and the cascade planes)
    c->tmT.drop();  // (and the tone-mapped plane; the exposure block has no shape and stays)
    c->blB.drop(); dev_free(c->blPyr);  // (and the bloomed plane with its pyramid)
    c->width = width; c->height = height;
    c->owned_rows = owned_rows_of(height, c->rank, c->world, c->stripe);
    c->st.width = width; c->st.height = height; c->st.owned_rows = c->owned_rows;
    if (!c->bound) {
        // pitch: rows padded to 256 B so every 8-pixel tile row is one aligned 128 B segment
        const size_t pitch = ((size_t)width * sizeof(float4) + 255) / 256 * 256;
        const size_t bytes = pitch * (size_t)std::max(c->owned_rows, 1);
        if (c->accum_own.bytes < bytes) {
            dev_free(c->accum_own);
            HIP_TRY(c, hipMalloc(&c->accum_own.p, bytes));
            c->accum_own.bytes = bytes;
        }
        c->accum = (float4 *)c->accum_own.p;
        c->pitch_bytes = pitch;
    }
    return glrtx_clear(c);
}

int glrtx_clear(glrtx_ctx *c) {
    if (!c) return GLRTX_EINVAL;
    int rc_;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!c->accum) return fail(c, GLRTX_EINVAL, "glrtx_clear: no accumulator (call glrtx_resize first)");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipMemsetAsync(c->accum, 0, c->pitch_bytes * (size_t)c->owned_rows, c->stream));
    if (c->adHalf.buf.p && (rc_ = plane_zero(c, c->adHalf))) return rc_;  // (the half buffer follows the accumulator: zeroed, at the current size)
    if (c->mmM.buf.p && (rc_ = plane_zero(c, c->mmM))) return rc_;        // (and so does the moments plane)
    if (c->rwC.buf.p && (rc_ = plane_zero(c, c->rwC, reweight::kCascades))) return rc_;  // (and so do the cascade planes)
    c->pres.frame = 0;  // (images already produced keep their numbers)
    return GLRTX_OK;
}

int glrtx_bind_accum(glrtx_ctx *c, void *device_ptr, size_t pitch_bytes, int capacity_rows) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (c->width < 1) return fail(c, GLRTX_EINVAL, "glrtx_bind_accum: call glrtx_resize first");
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!device_ptr) {
        c->bound = false;
        c->bound_rows = 0;
        return glrtx_resize(c, c->width, c->height);
    }
    if (pitch_bytes < (size_t)c->width * sizeof(float4) || pitch_bytes % sizeof(float4) != 0 || ((uintptr_t)device_ptr & 15) != 0)
        return fail(c, GLRTX_EINVAL, "glrtx_bind_accum: pitch/alignment invalid");
    if (capacity_rows < c->owned_rows)
        return fail(c, GLRTX_EINVAL, "glrtx_bind_accum: the buffer holds %d rows, this partition owns %d", capacity_rows, c->owned_rows);
    c->bound = true;
    c->bound_rows = capacity_rows;
    c->accum = (float4 *)device_ptr;
    c->pitch_bytes = pitch_bytes;
    if (c->mmM.buf.p) { if (int rc = plane_zero(c, c->mmM)) return rc; }  // (another accumulator: the moments of the old one's samples say nothing about it)
    if (c->rwC.buf.p) { if (int rc = plane_zero(c, c->rwC, reweight::kCascades)) return rc; }  // (and neither do its cascades)
    if (c->adHalf.buf.p) return plane_zero(c, c->adHalf);  // (another accumulator: the half buffer of the old one would be compared with unrelated samples)
    return GLRTX_OK;
}

int glrtx_set_stream(glrtx_ctx *c, void *hip_stream) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (int rc = fold_launches(c, true)) return rc;
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return GLRTX_OK;
}

int glrtx_set_variant(glrtx_ctx *c, int variant) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (variant < 0 || variant > 2) return fail(c, GLRTX_EINVAL, "glrtx_set_variant: unknown variant %d", variant);
    c->variant = variant;
    return GLRTX_OK;
}

int glrtx_set_shadow_range_limit(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    c->sc.shadow_limited = enable != 0 ? 1 : 0;  // read by the next launch (the scene block is copied into every launch's arguments)
    return GLRTX_OK;
}

int glrtx_set_volume_wavefront(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    c->vol_wavefront = enable != 0;  // read by the next launch (route_of)
    return GLRTX_OK;
}

int glrtx_set_texture_wavefront(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    c->tex_wavefront = enable != 0;  // read by the next launch (route_of)
    return GLRTX_OK;
}

int glrtx_count_rays(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    c->count_rays = enable != 0;
    return GLRTX_OK;
}


static int render_one(glrtx_ctx *c, const glrtx_params *p, const RenderReq &req);

// n_frames frames (seeds_xy) of one kind as launches of at most `most` frames, of equal size -- 16 frames under a limit of 14 are 8 + 8, not 14 + 2 -- in order.  A
// helping's parameters carry its first frame's seed (a single-frame helping renders with it); every frame counts as a launch in the statistics.
static int render_helpings(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, int most, RenderReq::Kind kind) {
    const int n_launches = (n_frames + most - 1) / most;
    const int chunk = (n_frames + n_launches - 1) / n_launches;
    for (int f0 = 0; f0 < n_frames; f0 += chunk) {
        glrtx_params q = *p;
        q.seed[0] = seeds_xy[2 * f0]; q.seed[1] = seeds_xy[2 * f0 + 1];
        const RenderReq req{kind, seeds_xy + 2 * (size_t)f0, std::min(chunk, n_frames - f0)};
        if (int rc = render_one(c, &q, req)) return rc;
        c->st.launches += (uint64_t)(req.n_frames - 1);  // (render_one has counted one)
    }
    return GLRTX_OK;
}

int glrtx_render_frames(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames) {
    if (!c || !p) return GLRTX_EINVAL;
    if (n_frames < 0 || (n_frames > 0 && !seeds_xy)) return fail(c, GLRTX_EINVAL, "glrtx_render_frames: bad seeds/n_frames");
    if (n_frames == 0) return GLRTX_OK;
    if (int rc = present_prepare(c, n_frames)) return rc;  // (GLRTX_EBUSY: nothing has changed)
    if (n_frames == 1 || !on_wavefront(route_of(c, p, RenderReq::Ordinary))) return render_helpings(c, p, seeds_xy, n_frames, 1, RenderReq::Ordinary);  // the megakernels have no frames-in-flight form: one launch per frame
    HIP_TRY(c, hipSetDevice(c->device));
    // A launch of the same camera that is still open takes the frames itself (feed_append); otherwise they are issued as launches of at most `most` frames -- what the
    // frames-in-flight memory budget allows (frames_cap) -- of equal size, in order; each of them stays open for the next call.  An allocation that fails is reported,
    // not worked around.
    if (p->n_samples >= 0 && p->max_depth >= 0 && c->have_scene && c->accum && c->owned_rows > 0 && feed_append(c, p, seeds_xy, n_frames) == 1) {
        c->last_was_render = true; c->last_p = *p;
        return presenting(c) ? present_issue(c, n_frames) : GLRTX_OK;  // (the launch's pass, already queued, resolves them too)
    }
    const bool may_feed = c->feed_ok && std::getenv("GLRTX_NO_FEED") == nullptr && c->pipeline && c->stream == c->own_stream;
    int most = std::min(n_frames, may_feed ? std::min(frames_cap(c, p, (int)kFedSlots), kFeedMaxFrames) : frames_cap(c, p, 1));
    if (const char *v = std::getenv("GLRTX_FEED_CAP")) { if (may_feed) most = std::max(1, std::min(most, std::atoi(v))); }
    return render_helpings(c, p, seeds_xy, n_frames, most, RenderReq::Ordinary);
}

int glrtx_render(glrtx_ctx *c, const glrtx_params *p) {
    if (!c || !p) return GLRTX_EINVAL;
    if (int rc = present_prepare(c, 1)) return rc;  // (GLRTX_EBUSY: nothing has changed)
    return render_one(c, p, RenderReq{});
}

// What the four render calls with a side plane share once their refusals are past: the plane they fold into at the accumulator's shape (`plane`; a plane of zeros on
// first use; none for H, which the selection itself makes sure of), the selection (`select`: its cfg, or none), then n_frames frames of `kind` in launches of at most
// what the frames-in-flight budget allows -- all of them on the selection made here, at the start of the call.  Never a fed launch: an open one is sealed first, so
// that its frames are accumulated before these.
static int render_side(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, RenderReq::Kind kind, Plane *plane, const glrtx_adaptive *select) {
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (plane && !plane->current(accum_shape(c)))
        if (int rc = plane_zero(c, *plane, kind == RenderReq::Cascades ? reweight::kCascades : 1)) return rc;
    if (select)
        if (int rc = adapt_select(c, select, kind == RenderReq::AdaptiveMoments)) return rc;
    if (n_frames == 0 || c->owned_rows == 0) { c->st.launches += (uint64_t)n_frames; return GLRTX_OK; }
    const int rc = render_helpings(c, p, seeds_xy, n_frames, std::min(n_frames, frames_cap(c, p, 1)), kind);
    seal_feed(c);  // (the next render call starts a launch of its own)
    return rc;
}

// Adaptive call: the selection from H, then n_frames frames of the active tiles only.
int glrtx_render_adaptive(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg) {
    if (!c) return GLRTX_EINVAL;
    if (int rc = adapt_check(c, p, seeds_xy, n_frames, cfg)) return rc;
    return render_side(c, p, seeds_xy, n_frames, RenderReq::Adaptive, nullptr, cfg);
}

int glrtx_adaptive_active_tiles(glrtx_ctx *c, int *active, int *total) {
    if (!c || !active || !total) return GLRTX_EINVAL;
    if (!c->ad_selected) return fail(c, GLRTX_EINVAL, "glrtx_adaptive_active_tiles: no adaptive call yet");
    if (int rc = glrtx_sync(c)) return rc;
    unsigned n = 0;
    HIP_TRY(c, hipMemcpy(&n, c->adCount.p, sizeof n, hipMemcpyDeviceToHost));
    *active = (int)n;
    *total = c->ad_tiles;
    return GLRTX_OK;
}

int glrtx_read_tile_mask(glrtx_ctx *c, uint8_t *dst) {
    if (!c || !dst) return GLRTX_EINVAL;
    if (!c->ad_selected) return fail(c, GLRTX_EINVAL, "glrtx_read_tile_mask: no adaptive call yet");
    // (the caller sizes dst by the context's CURRENT shape: a mask of another tile grid -- the image was resized or repartitioned since -- is refused, not copied)
    if (c->ad_tiles_x != (c->width + 7) / 8 || c->ad_tiles != c->ad_tiles_x * ((c->owned_rows + 7) / 8))
        return fail(c, GLRTX_EINVAL, "glrtx_read_tile_mask: the image changed shape since the last adaptive call (%d tiles then, %d now)", c->ad_tiles,
                    ((c->width + 7) / 8) * ((c->owned_rows + 7) / 8));
    if (int rc = glrtx_sync(c)) return rc;
    if (c->ad_tiles > 0) HIP_TRY(c, hipMemcpy(dst, c->adMask.p, (size_t)c->ad_tiles, hipMemcpyDeviceToHost));
    return GLRTX_OK;
}

int glrtx_read_adaptive_half(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    if (!c || !dst) return GLRTX_EINVAL;
    if (!c->adHalf.buf.p) return fail(c, GLRTX_EINVAL, "glrtx_read_adaptive_half: no half buffer (no adaptive call yet)");
    if (dst_pitch_bytes < (size_t)c->width * sizeof(float4)) return fail(c, GLRTX_EINVAL, "glrtx_read_adaptive_half: dst pitch too small");
    if (!c->adHalf.current(accum_shape(c))) return fail(c, GLRTX_EINVAL, "glrtx_read_adaptive_half: the accumulator changed shape since the last adaptive call");
    return read_back(c, c->adHalf.buf.p, c->pitch_bytes, dst, dst_pitch_bytes);
}

}  // extern "C"
// The two debug selections: `in` (the accumulator and H, or M) on the device, `select` (the one launch they differ in: input planes, mask, errors), the compaction,
// and the results back.
template <class Select>
static int debug_select(const char *fn, std::initializer_list<const float *> in, int width, int rows, uint8_t *mask_out, float *err_out, int *list_out, int *count_out,
                        Select &&select) {
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!mask_out || std::find(in.begin(), in.end(), nullptr) != in.end()) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    const int tiles8_x = (width + 7) / 8, n_tiles = tiles8_x * ((rows + 7) / 8);
    DebugScratch s;
    const float4 *d_in[2] = {nullptr, nullptr};
    int n_in = 0;
    for (const float *a : in) d_in[n_in++] = s.alloc((size_t)width * rows * sizeof(float4), a);
    unsigned char *d_mask = s.alloc<unsigned char>((size_t)n_tiles);
    float *d_err = s.alloc<float>((size_t)n_tiles * sizeof(float));
    int *d_list = s.alloc<int>((size_t)n_tiles * sizeof(int));
    unsigned *d_count = s.alloc<unsigned>(sizeof(unsigned));
    if (s.ok()) {
        select(d_in, tiles8_x, n_tiles, d_mask, d_err);
        hipLaunchKernelGGL(adaptive_compact_kernel, dim3(1), dim3(kAdaptCompactThreads), 0, 0, (const unsigned char *)d_mask, n_tiles, d_list, d_count);
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(mask_out, d_mask, (size_t)n_tiles);
    s.download(err_out, d_err, (size_t)n_tiles * sizeof(float));
    s.download(list_out, d_list, (size_t)n_tiles * sizeof(int));
    s.download(count_out, d_count, sizeof(int));
    return s.result(GLRTX_OK, fn);
}
extern "C" {

int glrtx_debug_adaptive_select(const float *accum, const float *half, int width, int rows, float threshold, int min_samples, uint8_t *mask_out, float *err_out,
                                int *list_out, int *count_out) {
    return debug_select("glrtx_debug_adaptive_select", {accum, half}, width, rows, mask_out, err_out, list_out, count_out,
                        [&](const float4 *const *in, int tiles8_x, int n_tiles, unsigned char *mask, float *err) {
                            hipLaunchKernelGGL(adaptive_select_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, 0, in[0], in[1], width, width, rows, tiles8_x, n_tiles,
                                               threshold, min_samples, mask, err);
                        });
}

int glrtx_debug_adaptive_select_moments(const float *moments, int width, int rows, float threshold, int min_samples, uint8_t *mask_out, float *err_out, int *list_out,
                                        int *count_out) {
    return debug_select("glrtx_debug_adaptive_select_moments", {moments}, width, rows, mask_out, err_out, list_out, count_out,
                        [&](const float4 *const *in, int tiles8_x, int n_tiles, unsigned char *mask, float *err) {
                            hipLaunchKernelGGL(adaptive_moments::select_kernel, dim3((n_tiles + 3) / 4), dim3(256), 0, 0, in[0], width, width, rows, tiles8_x, n_tiles,
                                               threshold, min_samples, mask, err);
                        });
}


// ---- denoising
int glrtx_render_features(glrtx_ctx *c, const glrtx_params *p) {
    const char *fn = "glrtx_render_features";
    if (!c) return GLRTX_EINVAL;
    if (!p) return fail(c, GLRTX_EINVAL, "%s: NULL params", fn);
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (c->n_spheres > 0) return fail(c, GLRTX_EINVAL, "%s: spheres are uploaded (an analytic sphere has no triangle normal to report)", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no size (call glrtx_resize)", fn);
    const int tiles8_x = (c->width + 7) / 8, tiles8_y = (c->owned_rows + 7) / 8;
    if ((size_t)tiles8_x * tiles8_y >= ((size_t)1 << 25)) return fail(c, GLRTX_EINVAL, "%s: %dx%d owned pixels (at most 2^31 tile-order ids)", fn, c->width, c->owned_rows);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->width * (size_t)std::max(c->owned_rows, 1) * sizeof(float4);
    int rc;
    if ((rc = ensure(c, c->ftA, bytes)) || (rc = ensure(c, c->ftCounter, sizeof(unsigned)))) return rc;
    const bool geom = c->mt_on;  // glrtx_track_motion: the kernels on GeomArgs, which write G as well
    if ((geom && (rc = ensure(c, c->ftG, bytes))) || (rc = plane_packed(c, c->ftN))) return rc;
    const auto planes_written = [&]() {  // (glrtx_track_motion; only once nothing can fail any more) the scene as it stands is what these planes show
        if (geom) { c->mt_g_have = true; c->mt_geom = glrtx_ctx::kMtCurrent; }
        return GLRTX_OK;
    };
    if (c->owned_rows == 0) return planes_written();
    const bool vine = c->sc.n_vine > 0;
    const int fetch = wgwf_fetch(c, vine);
    const int lds_stack = 2 * c->sc.stack_entries * kBlockThreads * (int)sizeof(int), lds_ranks = c->sc.n_crank * (int)sizeof(uint2);
    bool compact = wgwf_compact(c, vine, fetch);  // the node layout, chosen as trace_launch chooses it
    if (const char *v = std::getenv("GLRTX_COMPACT_NODES")) compact = std::atoi(v) != 0 && !vine && c->sc.n_crank > 0;
    compact = compact && lds_stack + lds_ranks <= 160 * 1024;
    const bool tex = c->n_tex > 0, maps = tex && c->have_maps;
    // One launch over the argument type: q, one of features.hip.h's six (or, with cutouts bound, a CutArgs of one of the four textured ones), selects the tree kernel's instantiation (the vine kernel comes by name) and is filled with what its type adds to Args --
    // G and the wire table (glrtx_track_motion), the texture set (plane A carries the looked-up albedo; as Map*Args, plane N the mapped normal).
    const auto launch = [&](auto q, void (*vine_kernel)(const decltype(q))) -> int {
        using A = decltype(q);
        void (*const kernel)(const A) = vine ? vine_kernel : compact ? features::features_tree<true, A> : features::features_tree<false, A>;
        const int lds = vine ? 0 : lds_stack + (compact ? lds_ranks : 0);
        if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        int per_cu = 0;
        HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlockThreads, lds));
        per_cu = std::max(per_cu, 1);
        features::Args &a = q;
        a.sc = c->sc;
        std::memcpy(a.cam, p->c2w, 16 * sizeof(float));
        std::memcpy(a.cam + 16, p->s2c, 16 * sizeof(float));
        a.width = c->width; a.height = c->height;
        a.owned_rows = c->owned_rows; a.rank = c->rank; a.world = c->world; a.stripe = c->stripe;
        a.tiles8_x = tiles8_x;
        a.n = (unsigned)(tiles8_x * tiles8_y) * 64u;
        a.out_n = (float4 *)c->ftN.buf.p; a.out_a = (float4 *)c->ftA.p;
        a.counter = (unsigned *)c->ftCounter.p;
        if constexpr (std::is_base_of_v<features::GeomArgs, A>) { q.out_g = (float4 *)c->ftG.p; q.wire = (const int *)c->qwire.p; }
        if constexpr (std::is_base_of_v<features::TexArgs, A> || std::is_base_of_v<features::TexGeomArgs, A>) q.tex = tex_set(c);
        if constexpr (features::is_cut<A>::value) q.cut = CutSet{(const int *)c->cutTri.p, (const CutRec *)c->cutRec.p};
        if constexpr (features::is_emit<A>::value) q.emit = EmitSet{(const int *)c->emitMat.p, (const float2 *)c->emitSt.p};
        std::memcpy(c->ft_cam, a.cam, sizeof c->ft_cam);  // (glrtx_reproject: the camera these planes belong to)
        const size_t needed = (a.n + kBlockThreads - 1) / kBlockThreads;
        const unsigned grid = (unsigned)std::max<size_t>(1, std::min<size_t>((size_t)per_cu * (size_t)c->n_cu, needed));
        HIP_TRY(c, hipMemsetAsync(c->ftCounter.p, 0, sizeof(unsigned), c->stream));
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(kBlockThreads), lds, c->stream, q);
        HIP_TRY(c, hipGetLastError());
        return planes_written();
    };
    if (tex && c->have_cut && !vine) {  // cutouts bound (never on a vine: glrtx_bind_cutouts): the same arguments and planes, walked with the CUT step
        using namespace features;
        if (maps) return geom ? launch(CutArgs<MapGeomArgs>{}, nullptr) : launch(CutArgs<MapArgs>{}, nullptr);
        return geom ? launch(CutArgs<TexGeomArgs>{}, nullptr) : launch(CutArgs<TexArgs>{}, nullptr);
    }
    if (tex && c->have_emit) {  // emission maps bound (never beside cutouts): the same arguments, walk and planes, then the emitter's picture in A
        using namespace features;
        if (maps) return geom ? launch(EmitArgs<MapGeomArgs>{}, features_vine_emit<MapGeomArgs>) : launch(EmitArgs<MapArgs>{}, features_vine_emit<MapArgs>);
        return geom ? launch(EmitArgs<TexGeomArgs>{}, features_vine_emit<TexGeomArgs>) : launch(EmitArgs<TexArgs>{}, features_vine_emit<TexArgs>);
    }
    if (maps) return geom ? launch(features::MapGeomArgs{}, features::features_vine_geom_maps) : launch(features::MapArgs{}, features::features_vine_maps);
    if (tex) return geom ? launch(features::TexGeomArgs{}, features::features_vine_geom_tex) : launch(features::TexArgs{}, features::features_vine_tex);
    return geom ? launch(features::GeomArgs{}, features::features_vine_geom) : launch(features::Args{}, features::features_vine);
}

static int denoise_shape_check(glrtx_ctx *c, const char *fn, bool need_result) {
    if (need_result && c->dnD.current(packed_shape(c))) return GLRTX_OK;  // (glrtx_reweight writes D without feature planes; otherwise the refusals below are what they were)
    if (!c->ftN.stamped() || !c->ftN.buf.p) return fail(c, GLRTX_EINVAL, "%s: no feature planes (call glrtx_render_features first)", fn);
    if (!c->ftN.current(packed_shape(c))) return fail(c, GLRTX_EINVAL, "%s: the image changed shape since the features were rendered", fn);
    if (need_result && !c->dnD.stamped()) return fail(c, GLRTX_EINVAL, "%s: no denoised image (call glrtx_denoise first)", fn);
    return GLRTX_OK;
}

int glrtx_read_features(glrtx_ctx *c, float *normal_depth, float *albedo_id, size_t pitch_bytes) {
    const char *fn = "glrtx_read_features";
    if (!c || !normal_depth || !albedo_id) return GLRTX_EINVAL;
    if (int rc = denoise_shape_check(c, fn, false)) return rc;
    const size_t row = (size_t)c->width * sizeof(float4);
    if (pitch_bytes < row) return fail(c, GLRTX_EINVAL, "%s: pitch too small", fn);
    if (int rc = read_back(c, c->ftN.buf.p, row, normal_depth, pitch_bytes)) return rc;
    return read_back(c, c->ftA.p, row, albedo_id, pitch_bytes);
}

int glrtx_denoise(glrtx_ctx *c, const glrtx_denoise_cfg *cfg) {
    const char *fn = "glrtx_denoise";
    if (!c) return GLRTX_EINVAL;
    FilterCfg k;
    if (int rc = denoise_cfg_check(c, cfg, fn, k)) return rc;
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (int rc = denoise_shape_check(c, fn, false)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->width * (size_t)std::max(c->owned_rows, 1) * sizeof(float4);
    int rc;
    if ((rc = ensure(c, c->dnP[0], bytes)) || (rc = ensure(c, c->dnP[1], bytes)) || (rc = plane_packed(c, c->dnD))) return rc;
    if (c->owned_rows == 0) return GLRTX_OK;
    return denoise_passes(c, c->stream, c->accum, nullptr, (int)(c->pitch_bytes / sizeof(float4)), (const float4 *)c->ftN.buf.p, (const float4 *)c->ftA.p,
                          (float4 *)c->dnP[0].p, (float4 *)c->dnP[1].p, (float4 *)c->dnD.buf.p, nullptr, c->width, c->owned_rows, k);
}

int glrtx_read_denoised(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    const char *fn = "glrtx_read_denoised";
    if (!c || !dst) return GLRTX_EINVAL;
    if (int rc = denoise_shape_check(c, fn, true)) return rc;
    const size_t row = (size_t)c->width * sizeof(float4);
    if (dst_pitch_bytes < row) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    return read_back(c, c->dnD.buf.p, row, dst, dst_pitch_bytes);
}

// D through the resolve: resolve_kernel with D as its source (a mean with the count word 1: the kernel's division is exact).
int glrtx_resolve_denoised_rgba8(glrtx_ctx *c, uint8_t *dst, size_t dst_pitch_bytes, float gamma, int flip_y) {
    const char *fn = "glrtx_resolve_denoised_rgba8";
    if (!c || !dst) return GLRTX_EINVAL;
    if (int rc = denoise_shape_check(c, fn, true)) return rc;
    if (!(gamma > 0.f)) return fail(c, GLRTX_EINVAL, "%s: gamma must be positive", fn);
    if (dst_pitch_bytes < (size_t)c->width * 4) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    return resolve_to_caller(c, dst, dst_pitch_bytes, [&](uchar4 *out) {
        hipLaunchKernelGGL(resolve_kernel<kResolvePer>, resolve_grid(c->width, c->owned_rows), dim3(256), 0, c->stream, (const float4 *)c->dnD.buf.p, c->width, c->width,
                           c->owned_rows, out, c->width, 1.0f / gamma, flip_y ? 1 : 0);
        HIP_TRY(c, hipGetLastError());
        return GLRTX_OK;
    });
}

int glrtx_debug_denoise(const float *accum, const float *normal_depth, const float *albedo_id, int width, int rows, const glrtx_denoise_cfg *cfg, float *out) {
    const char *fn = "glrtx_debug_denoise";
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!accum || !normal_depth || !albedo_id || !out) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    FilterCfg k;
    if (int rc = denoise_cfg_check(nullptr, cfg, fn, k)) return rc;
    const size_t bytes = (size_t)width * rows * sizeof(float4);
    DebugScratch s;
    const float4 *acc = s.alloc(bytes, accum), *guide = s.alloc(bytes, normal_depth), *albedo = s.alloc(bytes, albedo_id);
    float4 *p0 = s.alloc(bytes), *p1 = s.alloc(bytes), *D = s.alloc(bytes);
    int rc = GLRTX_OK;
    if (s.ok()) rc = denoise_passes(nullptr, 0, acc, nullptr, width, guide, albedo, p0, p1, D, nullptr, width, rows, k);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(out, D, bytes);
    }
    return s.result(rc, fn);
}

// ---- variance guidance
int glrtx_track_moments(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    if (enable) { c->mm_on = true; return GLRTX_OK; }
    if (!c->mm_on) return GLRTX_OK;
    seal_feed(c);
    if (int rc = glrtx_sync(c)) return rc;
    c->mmM.drop(); dev_free(c->mmM_spare);
    c->mm_on = false;
    return GLRTX_OK;
}

// glrtx_render_adaptive's launches without a selection: plain launches with sample planes on the context's stream, each folded by accumulate_moments_kernel into
// the accumulator and M.
int glrtx_render_moments(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames) {
    if (!c) return GLRTX_EINVAL;
    if (int rc = moments_check(c, p, seeds_xy, n_frames)) return rc;
    return render_side(c, p, seeds_xy, n_frames, RenderReq::Moments, &c->mmM, nullptr);
}

// glrtx_render_adaptive with the selection made from M and the active tiles' samples folded into M: H is neither read, allocated nor written.
int glrtx_render_adaptive_moments(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg) {
    if (!c) return GLRTX_EINVAL;
    if (int rc = adapt_moments_check(c, p, seeds_xy, n_frames, cfg)) return rc;
    return render_side(c, p, seeds_xy, n_frames, RenderReq::AdaptiveMoments, &c->mmM, cfg);
}

int glrtx_read_moments(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    const char *fn = "glrtx_read_moments";
    if (!c || !dst) return GLRTX_EINVAL;
    if (!c->mm_on) return fail(c, GLRTX_EINVAL, "%s: moments are not tracked (glrtx_track_moments)", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (dst_pitch_bytes < (size_t)c->width * sizeof(float4)) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->mmM.current(accum_shape(c)))
        if (int rc = plane_zero(c, c->mmM)) return rc;  // (first use: a plane of zeros)
    return read_back(c, c->mmM.buf.p, c->pitch_bytes, dst, dst_pitch_bytes);
}

int glrtx_denoise_variance(glrtx_ctx *c, const glrtx_denoise_var_cfg *cfg) {
    const char *fn = "glrtx_denoise_variance";
    if (!c) return GLRTX_EINVAL;
    FilterCfg k;
    if (int rc = denoise_cfg_check(c, cfg, fn, k)) return rc;
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (!c->mm_on) return fail(c, GLRTX_EINVAL, "%s: moments are not tracked (glrtx_track_moments)", fn);
    if (!c->mmM.current(accum_shape(c))) return fail(c, GLRTX_EINVAL, "%s: no moments plane yet (call glrtx_render_moments first)", fn);
    if (int rc = denoise_shape_check(c, fn, false)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->width * (size_t)std::max(c->owned_rows, 1);
    int rc;
    if ((rc = ensure(c, c->dnP[0], px * sizeof(float4))) || (rc = ensure(c, c->dnP[1], px * sizeof(float4)))) return rc;
    for (DevBuf &v : c->dnV)
        if ((rc = ensure(c, v, px * sizeof(float)))) return rc;
    if ((rc = plane_packed(c, c->dnD))) return rc;
    if (c->owned_rows == 0) return GLRTX_OK;
    float *const v[3] = {(float *)c->dnV[0].p, (float *)c->dnV[1].p, (float *)c->dnV[2].p};
    return denoise_passes(c, c->stream, c->accum, (const float4 *)c->mmM.buf.p, (int)(c->pitch_bytes / sizeof(float4)), (const float4 *)c->ftN.buf.p, (const float4 *)c->ftA.p,
                          (float4 *)c->dnP[0].p, (float4 *)c->dnP[1].p, (float4 *)c->dnD.buf.p, v, c->width, c->owned_rows, k);
}

int glrtx_debug_denoise_variance(const float *accum, const float *moments, const float *normal_depth, const float *albedo_id, int width, int rows,
                                 const glrtx_denoise_var_cfg *cfg, float *out, float *v0_out) {
    const char *fn = "glrtx_debug_denoise_variance";
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!accum || !moments || !normal_depth || !albedo_id || !out) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    FilterCfg k;
    if (int rc = denoise_cfg_check(nullptr, cfg, fn, k)) return rc;
    const size_t bytes = (size_t)width * rows * sizeof(float4), vbytes = (size_t)width * rows * sizeof(float);
    DebugScratch s;
    const float4 *acc = s.alloc(bytes, accum), *M = s.alloc(bytes, moments), *guide = s.alloc(bytes, normal_depth), *albedo = s.alloc(bytes, albedo_id);
    float4 *p0 = s.alloc(bytes), *p1 = s.alloc(bytes), *D = s.alloc(bytes);
    float *const v[3] = {s.alloc<float>(vbytes), s.alloc<float>(vbytes), s.alloc<float>(vbytes)};
    int rc = GLRTX_OK;
    if (s.ok()) rc = denoise_passes(nullptr, 0, acc, M, width, guide, albedo, p0, p1, D, v, width, rows, k);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(out, D, bytes);
        s.download(v0_out, v[0], vbytes);
    }
    return s.result(rc, fn);
}

// ---- firefly re-weighting
int glrtx_track_cascades(glrtx_ctx *c, int enable, float start) {
    const char *fn = "glrtx_track_cascades";
    if (!c) return GLRTX_EINVAL;
    if (enable) {
        if (!cascade_start_ok(start)) return fail(c, GLRTX_EINVAL, "%s: start %g is not within 2^-20 .. 2^20", fn, (double)start);
        if (c->rw_on && c->rwC.buf.p && start != c->rw_start) {  // the bins were the old bounds'
            seal_feed(c);
            HIP_TRY(c, hipSetDevice(c->device));
            if (int rc = plane_zero(c, c->rwC, reweight::kCascades)) return rc;
        }
        c->rw_on = true; c->rw_start = start;
        return GLRTX_OK;
    }
    if (!c->rw_on) return GLRTX_OK;
    seal_feed(c);
    if (int rc = glrtx_sync(c)) return rc;
    c->rwC.drop();
    c->rw_on = false;
    return GLRTX_OK;
}

// glrtx_render_moments with the other sink: plain launches with sample planes on the context's stream, each folded by accumulate_cascades_kernel into the
// accumulator and C.
int glrtx_render_cascades(glrtx_ctx *c, const glrtx_params *p, const float *seeds_xy, int n_frames) {
    const char *fn = "glrtx_render_cascades";
    if (!c) return GLRTX_EINVAL;
    if (int rc = side_plane_check(c, p, seeds_xy, n_frames, fn, c->rw_on, "cascades are not tracked (glrtx_track_cascades)")) return rc;
    return render_side(c, p, seeds_xy, n_frames, RenderReq::Cascades, &c->rwC, nullptr);
}

int glrtx_read_cascades(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    const char *fn = "glrtx_read_cascades";
    if (!c || !dst) return GLRTX_EINVAL;
    if (!c->rw_on) return fail(c, GLRTX_EINVAL, "%s: cascades are not tracked (glrtx_track_cascades)", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (dst_pitch_bytes < (size_t)c->width * sizeof(float4)) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    HIP_TRY(c, hipSetDevice(c->device));
    if (!c->rwC.current(accum_shape(c)))
        if (int rc = plane_zero(c, c->rwC, reweight::kCascades)) return rc;  // (first use: planes of zeros)
    return read_back(c, c->rwC.buf.p, c->pitch_bytes, dst, dst_pitch_bytes, reweight::kCascades);
}

// Everything glrtx_reweight refuses, checked before anything changes.
static int reweight_check(glrtx_ctx *c, const glrtx_reweight_cfg *cfg, const char *fn) {
    if (int rc = reweight_cfg_check(c, cfg, fn)) return rc;
    if (!c->rw_on) return fail(c, GLRTX_EINVAL, "%s: cascades are not tracked (glrtx_track_cascades)", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no accumulator (call glrtx_resize)", fn);
    if (!c->rwC.current(accum_shape(c))) return fail(c, GLRTX_EINVAL, "%s: no cascade planes yet (call glrtx_render_cascades first)", fn);
    if (c->world > 1) return fail(c, GLRTX_EINVAL, "%s: the context is partitioned (rank %d of %d): the neighbourhood would stop at every stripe's seam", fn, c->rank, c->world);
    return GLRTX_OK;
}

int glrtx_reweight(glrtx_ctx *c, const glrtx_reweight_cfg *cfg) {
    const char *fn = "glrtx_reweight";
    if (!c) return GLRTX_EINVAL;
    if (int rc = reweight_check(c, cfg, fn)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = plane_packed(c, c->dnD)) return rc;
    if (c->owned_rows == 0) return GLRTX_OK;
    const int pitch_f4 = (int)(c->pitch_bytes / sizeof(float4));
    return reweight_pass(c, c->stream, (const float4 *)c->rwC.buf.p, (size_t)pitch_f4 * (size_t)c->owned_rows, pitch_f4, c->width, c->owned_rows, (float4 *)c->dnD.buf.p, *cfg);
}

int glrtx_debug_fold_cascades(const float *accum, const float *cascades, const float *frames, int n_frames, int width, int rows, float start, float *accum_out,
                              float *cascades_out) {
    const char *fn = "glrtx_debug_fold_cascades";
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!accum || !cascades || n_frames < 0 || (n_frames > 0 && !frames)) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer or negative n_frames", fn);
    if (!cascade_start_ok(start)) return fail(nullptr, GLRTX_EINVAL, "%s: start %g is not within 2^-20 .. 2^20", fn, (double)start);
    const size_t plane = (size_t)width * rows, bytes = plane * sizeof(float4);
    DebugScratch s;
    float4 *acc = s.alloc(bytes, accum), *C = s.alloc(reweight::kCascades * bytes, cascades);
    const float4 *F = s.alloc(std::max<size_t>((size_t)n_frames, 1) * bytes, n_frames > 0 ? frames : nullptr);
    if (s.ok() && n_frames > 0) {
        const accumulate::Image im{acc, width, width, rows};
        hipLaunchKernelGGL(reweight::accumulate_cascades_kernel, dim3((width + 63) / 64, (rows + 3) / 4), dim3(256), 0, 0, im, accumulate::Planes{F, n_frames, 1},
                           accumulate::Cascades{C, plane, start});
        s.e = hipGetLastError();
    }
    s.sync();
    s.download(accum_out, acc, bytes);
    s.download(cascades_out, C, reweight::kCascades * bytes);
    return s.result(GLRTX_OK, fn);
}

int glrtx_debug_reweight(const float *cascades, int width, int rows, const glrtx_reweight_cfg *cfg, float *out) {
    const char *fn = "glrtx_debug_reweight";
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!cascades || !out) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (int rc = reweight_cfg_check(nullptr, cfg, fn)) return rc;
    const size_t plane = (size_t)width * rows, bytes = plane * sizeof(float4);
    DebugScratch s;
    const float4 *C = s.alloc(reweight::kCascades * bytes, cascades);
    float4 *D = s.alloc(bytes);
    int rc = GLRTX_OK;
    if (s.ok()) rc = reweight_pass(nullptr, 0, C, plane, width, width, rows, D, *cfg);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(out, D, bytes);
    }
    return s.result(rc, fn);
}

// Device time of one resolve by itself, as glrtx_debug_tonemap_burst measures its passes.  Writes D as glrtx_reweight does.
int glrtx_debug_reweight_burst(glrtx_ctx *c, const glrtx_reweight_cfg *cfg, int reps, float *ms_per_launch) {
    const char *fn = "glrtx_debug_reweight_burst";
    if (!c || !ms_per_launch || reps < 1) return GLRTX_EINVAL;
    if (int rc = reweight_check(c, cfg, fn)) return rc;
    if (c->owned_rows == 0) return fail(c, GLRTX_EINVAL, "%s: no rows", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = plane_packed(c, c->dnD)) return rc;
    const int pitch_f4 = (int)(c->pitch_bytes / sizeof(float4));
    return burst_time(c, reps, ms_per_launch, [&] {
        return reweight_pass(c, c->stream, (const float4 *)c->rwC.buf.p, (size_t)pitch_f4 * (size_t)c->owned_rows, pitch_f4, c->width, c->owned_rows,
                             (float4 *)c->dnD.buf.p, *cfg);
    });
}

// ---- tone mapping
int glrtx_exposure_measure(glrtx_ctx *c, const glrtx_tonemap_cfg *cfg) {
    const char *fn = "glrtx_exposure_measure";
    if (!c) return GLRTX_EINVAL;
    const float4 *src = nullptr;
    int pitch_f4 = 0;
    if (int rc = tonemap_source(c, cfg, fn, src, pitch_f4)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = exposure_ensure(c)) return rc;
    return exposure_passes(c, c->stream, src, pitch_f4, c->width, c->owned_rows, (tonemap::Exposure *)c->tmExp.p, *cfg);
}

int glrtx_exposure_reset(glrtx_ctx *c) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (c->tmExp.p) HIP_TRY(c, hipMemsetAsync(c->tmExp.p, 0, sizeof(tonemap::Exposure), c->stream));
    return GLRTX_OK;
}

int glrtx_read_exposure(glrtx_ctx *c, glrtx_exposure *out) {
    if (!c || !out) return GLRTX_EINVAL;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = exposure_ensure(c)) return rc;
    if (int rc = glrtx_sync(c)) return rc;
    HIP_TRY(c, hipMemcpy(out, (const char *)c->tmExp.p + tonemap::kExposureOut, sizeof *out, hipMemcpyDeviceToHost));
    return GLRTX_OK;
}

int glrtx_tonemap(glrtx_ctx *c, const glrtx_tonemap_cfg *cfg) {
    const char *fn = "glrtx_tonemap";
    if (!c) return GLRTX_EINVAL;
    const float4 *src = nullptr;
    int pitch_f4 = 0;
    if (int rc = tonemap_source(c, cfg, fn, src, pitch_f4)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = exposure_ensure(c)) return rc;
    if (int rc = plane_packed(c, c->tmT)) return rc;
    if (c->owned_rows == 0) return GLRTX_OK;
    return tonemap_plane_pass(c, c->stream, src, pitch_f4, c->width, c->owned_rows, (float4 *)c->tmT.buf.p, (const tonemap::Exposure *)c->tmExp.p, *cfg);
}

int glrtx_read_tonemapped(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    const char *fn = "glrtx_read_tonemapped";
    if (!c || !dst) return GLRTX_EINVAL;
    if (!c->tmT.current(packed_shape(c))) return fail(c, GLRTX_EINVAL, "%s: no tone-mapped plane (call glrtx_tonemap first)", fn);
    const size_t row = (size_t)c->width * sizeof(float4);
    if (dst_pitch_bytes < row) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    return read_back(c, c->tmT.buf.p, row, dst, dst_pitch_bytes);
}

// Source -> bytes in one pass: the curve in front of the resolve's own arithmetic (tonemap_resolve); T is not touched.
int glrtx_resolve_tonemapped_rgba8(glrtx_ctx *c, uint8_t *dst, size_t dst_pitch_bytes, const glrtx_tonemap_cfg *cfg) {
    const char *fn = "glrtx_resolve_tonemapped_rgba8";
    if (!c || !dst) return GLRTX_EINVAL;
    const float4 *src = nullptr;
    int pitch_f4 = 0;
    if (int rc = tonemap_source(c, cfg, fn, src, pitch_f4)) return rc;
    if (dst_pitch_bytes < (size_t)c->width * 4) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = exposure_ensure(c)) return rc;
    return resolve_to_caller(c, dst, dst_pitch_bytes, [&](uchar4 *out) {
        return tonemap_resolve_pass(c, c->stream, src, pitch_f4, c->width, c->owned_rows, out, (const tonemap::Exposure *)c->tmExp.p, *cfg);
    });
}

int glrtx_debug_tonemap(const float *src, int width, int rows, const glrtx_tonemap_cfg *cfg, const float *exposure_in, glrtx_exposure *exp_out, float *t_out,
                        uint8_t *rgba8_out) {
    const char *fn = "glrtx_debug_tonemap";
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!src) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (int rc = tonemap_cfg_check(nullptr, cfg, fn)) return rc;
    const size_t px = (size_t)width * rows;
    tonemap::Exposure init{};
    if (exposure_in) { init.exposure = *exposure_in; init.measurements = 1; }
    DebugScratch s;
    const float4 *in = s.alloc(px * sizeof(float4), src);
    tonemap::Exposure *st = s.alloc<tonemap::Exposure>(sizeof init, &init);
    float4 *T = s.alloc(px * sizeof(float4));
    uchar4 *bytes = s.alloc<uchar4>(px * 4);
    int rc = GLRTX_OK;
    if (s.ok()) rc = exposure_passes(nullptr, 0, in, width, width, rows, st, *cfg);
    if (s.ok() && rc == GLRTX_OK) rc = tonemap_plane_pass(nullptr, 0, in, width, width, rows, T, st, *cfg);
    if (s.ok() && rc == GLRTX_OK) rc = tonemap_resolve_pass(nullptr, 0, in, width, width, rows, bytes, st, *cfg);
    if (rc == GLRTX_OK) {
        s.sync();
        if (exp_out) {
            s.download(exp_out, (const char *)st + tonemap::kExposureOut, sizeof *exp_out);
            if (s.ok() && exposure_in) exp_out->measurements = 1;  // (one measurement, whatever stood before it)
        }
        s.download(t_out, T, px * sizeof(float4));
        s.download(rgba8_out, bytes, px * 4);
    }
    return s.result(rc, fn);
}

// Device time of one tone-mapping pass by itself, as glrtx_debug_resolve_burst measures the resolve: `reps` launches back to back between one pair of events, after
// a warm-up pass.  which: 0 the plain resolve kernel on the cfg's source (the yardstick beside it), 1 tonemap_resolve, 2 tonemap_plane, 3 a measurement (histogram
// + reduce).  3 moves E like `reps` measurements; nothing else the context owns changes but T (2) and the byte image.
int glrtx_debug_tonemap_burst(glrtx_ctx *c, const glrtx_tonemap_cfg *cfg, int which, int reps, float *ms_per_launch) {
    const char *fn = "glrtx_debug_tonemap_burst";
    if (!c || !ms_per_launch || reps < 1 || which < 0 || which > 3) return GLRTX_EINVAL;
    const float4 *src = nullptr;
    int pitch_f4 = 0;
    if (int rc = tonemap_source(c, cfg, fn, src, pitch_f4)) return rc;
    if (c->owned_rows == 0) return fail(c, GLRTX_EINVAL, "%s: no rows", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = exposure_ensure(c)) || (rc = ensure(c, c->rgba8, (size_t)c->width * 4 * (size_t)c->owned_rows))) return rc;
    if (which == 2 && (rc = plane_packed(c, c->tmT))) return rc;
    tonemap::Exposure *st = (tonemap::Exposure *)c->tmExp.p;
    return burst_time(c, reps, ms_per_launch, [&] {
        if (which == 1) return tonemap_resolve_pass(c, c->stream, src, pitch_f4, c->width, c->owned_rows, (uchar4 *)c->rgba8.p, st, *cfg);
        if (which == 2) return tonemap_plane_pass(c, c->stream, src, pitch_f4, c->width, c->owned_rows, (float4 *)c->tmT.buf.p, st, *cfg);
        if (which == 3) return exposure_passes(c, c->stream, src, pitch_f4, c->width, c->owned_rows, st, *cfg);
        hipLaunchKernelGGL(resolve_kernel<kResolvePer>, resolve_grid(c->width, c->owned_rows), dim3(256), 0, c->stream, src, pitch_f4, c->width, c->owned_rows,
                           (uchar4 *)c->rgba8.p, c->width, 1.0f / cfg->gamma, cfg->flip_y ? 1 : 0);
        return GLRTX_OK;
    });
}


// ---- bloom
int glrtx_bloom(glrtx_ctx *c, const glrtx_bloom_cfg *cfg) {
    const char *fn = "glrtx_bloom";
    if (!c) return GLRTX_EINVAL;
    const float4 *src = nullptr;
    int pitch_f4 = 0;
    if (int rc = bloom_source(c, cfg, fn, src, pitch_f4)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = bloom_ensure(c)) return rc;
    const BloomLevels L = bloom_levels(c->width, c->owned_rows, cfg->levels);
    if (int rc = bloom_down_passes(c, c->stream, src, pitch_f4, L, (float4 *)c->blPyr.p, *cfg)) return rc;
    return bloom_up_passes(c, c->stream, src, pitch_f4, L, (float4 *)c->blPyr.p, (float4 *)c->blB.buf.p, *cfg);
}

int glrtx_read_bloomed(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    const char *fn = "glrtx_read_bloomed";
    if (!c || !dst) return GLRTX_EINVAL;
    if (!c->blB.current(packed_shape(c))) return fail(c, GLRTX_EINVAL, "%s: no bloomed plane (call glrtx_bloom first)", fn);
    const size_t row = (size_t)c->width * sizeof(float4);
    if (dst_pitch_bytes < row) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    return read_back(c, c->blB.buf.p, row, dst, dst_pitch_bytes);
}

// glrtx_tonemap with B as its source: tonemap_plane, B -> T.
int glrtx_tonemap_bloomed(glrtx_ctx *c, const glrtx_tonemap_cfg *cfg) {
    const char *fn = "glrtx_tonemap_bloomed";
    if (!c) return GLRTX_EINVAL;
    glrtx_tonemap_cfg k;
    if (int rc = tonemap_bloomed_cfg(c, cfg, fn, k)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = exposure_ensure(c)) return rc;
    if (int rc = plane_packed(c, c->tmT)) return rc;
    return tonemap_plane_pass(c, c->stream, (const float4 *)c->blB.buf.p, c->width, c->width, c->owned_rows, (float4 *)c->tmT.buf.p, (const tonemap::Exposure *)c->tmExp.p, k);
}

// glrtx_resolve_tonemapped_rgba8 with B as its source: tonemap_resolve, B -> bytes.
int glrtx_resolve_bloomed_rgba8(glrtx_ctx *c, uint8_t *dst, size_t dst_pitch_bytes, const glrtx_tonemap_cfg *cfg) {
    const char *fn = "glrtx_resolve_bloomed_rgba8";
    if (!c || !dst) return GLRTX_EINVAL;
    glrtx_tonemap_cfg k;
    if (int rc = tonemap_bloomed_cfg(c, cfg, fn, k)) return rc;
    if (dst_pitch_bytes < (size_t)c->width * 4) return fail(c, GLRTX_EINVAL, "%s: dst pitch too small", fn);
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = exposure_ensure(c)) return rc;
    return resolve_to_caller(c, dst, dst_pitch_bytes, [&](uchar4 *out) {
        return tonemap_resolve_pass(c, c->stream, (const float4 *)c->blB.buf.p, c->width, c->width, c->owned_rows, out, (const tonemap::Exposure *)c->tmExp.p, k);
    });
}

int glrtx_debug_bloom(const float *src, int width, int rows, const glrtx_bloom_cfg *cfg, float *d_out, float *b_out) {
    const char *fn = "glrtx_debug_bloom";
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536) return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!src) return fail(nullptr, GLRTX_EINVAL, "%s: NULL buffer", fn);
    if (int rc = bloom_cfg_check(nullptr, cfg, fn)) return rc;
    const size_t px = (size_t)width * rows;
    const BloomLevels L = bloom_levels(width, rows, cfg->levels);
    const size_t pyr_bytes = L.at[L.n + 1] * sizeof(float4);
    DebugScratch s;
    const float4 *in = s.alloc(px * sizeof(float4), src);
    float4 *pyr = s.alloc(pyr_bytes);
    float4 *B = s.alloc(px * sizeof(float4));
    int rc = GLRTX_OK;
    if (s.ok()) rc = bloom_down_passes(nullptr, 0, in, width, L, pyr, *cfg);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(d_out, pyr, pyr_bytes);  // (D_1 .. D_levels, before the up chain turns them into U_k)
    }
    if (s.ok() && rc == GLRTX_OK) rc = bloom_up_passes(nullptr, 0, in, width, L, pyr, B, *cfg);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(b_out, B, px * sizeof(float4));
    }
    return s.result(rc, fn);
}

// Device time of one glrtx_bloom (2 * levels launches) by itself, as glrtx_debug_tonemap_burst measures its passes: `reps` calls' launches back to back between
// one pair of events, after a warm-up pass.  Leaves B as glrtx_bloom does.
int glrtx_debug_bloom_burst(glrtx_ctx *c, const glrtx_bloom_cfg *cfg, int reps, float *ms_per_call) {
    const char *fn = "glrtx_debug_bloom_burst";
    if (!c || !ms_per_call || reps < 1) return GLRTX_EINVAL;
    const float4 *src = nullptr;
    int pitch_f4 = 0;
    if (int rc = bloom_source(c, cfg, fn, src, pitch_f4)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = bloom_ensure(c)) return rc;
    const BloomLevels L = bloom_levels(c->width, c->owned_rows, cfg->levels);
    return burst_time(c, reps, ms_per_call, [&] {
        if (int rc = bloom_down_passes(c, c->stream, src, pitch_f4, L, (float4 *)c->blPyr.p, *cfg)) return rc;
        return bloom_up_passes(c, c->stream, src, pitch_f4, L, (float4 *)c->blPyr.p, (float4 *)c->blB.buf.p, *cfg);
    });
}

// ---- reprojection (glrtx_reproject)
static int reproject_setup_check(glrtx_ctx *c, const char *fn, const float *c2w_prev, const float *s2c_prev, const glrtx_reproject_cfg *cfg, glrt_detail::ReprojectSetup &st) {
    switch (glrt_detail::reproject_setup(c2w_prev, s2c_prev, cfg->max_history, cfg->depth_tolerance, cfg->normal_tolerance, st)) {
        case 0: return GLRTX_OK;
        case 1: return fail(c, GLRTX_EINVAL, "%s: max_history %d < 1", fn, cfg->max_history);
        case 2: return fail(c, GLRTX_EINVAL, "%s: depth_tolerance %g is not a positive finite number", fn, (double)cfg->depth_tolerance);
        case 3: return fail(c, GLRTX_EINVAL, "%s: normal_tolerance %g is not finite", fn, (double)cfg->normal_tolerance);
        case 4: return fail(c, GLRTX_EINVAL, "%s: the previous camera's c2w is singular", fn);
        default: return fail(c, GLRTX_EINVAL, "%s: the previous camera's s2c is singular", fn);
    }
}

// The kernel on `stream`: old accumulator (pitch_f4) and planes, new planes -> `out` (pitch_f4); `counts` (reproject::kCountBytes) is zeroed first.
static hipError_t reproject_counts(const void *dev_counts, int *carried, int *hit_pixels) {
    unsigned long long w[reproject::kCountSlots * reproject::kCountStride], sum = 0;
    const hipError_t e = hipMemcpy(w, dev_counts, sizeof w, hipMemcpyDeviceToHost);
    for (int i = 0; i < reproject::kCountSlots; i++) sum += w[i * reproject::kCountStride];  // (both halves stay below 2^31: no carry between them)
    if (carried) *carried = (int)(sum & 0xFFFFFFFFull);
    if (hit_pixels) *hit_pixels = (int)(sum >> 32);
    return e;
}

// glrtx_reproject (motion false) and glrtx_reproject_motion (true): one sequence, two kernels.
static int reproject_call(glrtx_ctx *c, const glrtx_params *cur, const glrtx_reproject_cfg *cfg, const char *fn, bool motion) {
    if (!c) return GLRTX_EINVAL;
    if (!cur || !cfg) return fail(c, GLRTX_EINVAL, "%s: NULL params or cfg", fn);
    // everything glrtx_render_features refuses, before anything changes
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "%s: no scene uploaded", fn);
    if (c->n_spheres > 0) return fail(c, GLRTX_EINVAL, "%s: spheres are uploaded (an analytic sphere has no triangle normal to report)", fn);
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "%s: no size (call glrtx_resize)", fn);
    if ((size_t)((c->width + 7) / 8) * (size_t)((c->owned_rows + 7) / 8) >= ((size_t)1 << 25))
        return fail(c, GLRTX_EINVAL, "%s: %dx%d owned pixels (at most 2^31 tile-order ids)", fn, c->width, c->owned_rows);
    if (c->world > 1) return fail(c, GLRTX_EINVAL, "%s: the context is partitioned (rank %d of %d): a pixel's history may lie on another rank", fn, c->rank, c->world);
    if (c->bound) return fail(c, GLRTX_EINVAL, "%s: a caller-owned accumulator is bound (glrtx_bind_accum): the call swaps accumulators", fn);
    if (int rc = denoise_shape_check(c, fn, false)) return rc;
    if (motion) {
        if (!c->mt_on) return fail(c, GLRTX_EINVAL, "%s: motion tracking is off (glrtx_track_motion)", fn);
        if (!c->ftG.p || !c->mt_g_have) return fail(c, GLRTX_EINVAL, "%s: no geometry plane (call glrtx_render_features with tracking on first)", fn);
        if (c->mt_geom == glrtx_ctx::kMtNone)
            return fail(c, GLRTX_EINVAL, "%s: the previous geometry is not known (a scene was uploaded since the last glrtx_render_features)", fn);
    }
    glrt_detail::ReprojectSetup st;
    if (int rc = reproject_setup_check(c, fn, c->ft_cam, c->ft_cam + 16, cfg, st)) return rc;
    seal_feed(c);
    HIP_TRY(c, hipSetDevice(c->device));
    const size_t acc_bytes = c->pitch_bytes * (size_t)std::max(c->owned_rows, 1);
    int rc;
    if ((rc = ensure(c, c->accum_spare, acc_bytes)) || (rc = ensure(c, c->rpCount, reproject::kCountBytes))) return rc;
    const bool carry_m = c->mmM.current(accum_shape(c));  // glrtx_track_moments is on and M exists: a second M is written by the same pass and swapped in as the accumulator is
    if (carry_m && (rc = ensure(c, c->mmM_spare, acc_bytes))) return rc;
    if (motion && c->mt_geom == glrtx_ctx::kMtCurrent && (rc = motion_snapshot(c))) return rc;  // nothing moved since the planes: previous = current
    for (auto &sl : c->pipe)  // behind every launch that may still add to the accumulator or read the scene (refit_run's rule)
        if (sl.stream && sl.used) {
            HIP_TRY(c, hipEventRecord(c->rf.slot_ev, sl.stream));
            HIP_TRY(c, hipStreamWaitEvent(c->stream, c->rf.slot_ev, 0));
        }
    std::swap(c->ftN.buf, c->ftN_spare);  // the planes as they stand become N0 / A0; glrtx_render_features fills (on first use: allocates) the other pair
    std::swap(c->ftA, c->ftA_spare);
    if (c->mt_on) std::swap(c->ftG, c->ftG_spare);  // (glrtx_track_motion: the third pair goes with them)
    float cam_prev[32];
    std::memcpy(cam_prev, c->ft_cam, sizeof cam_prev);
    if ((rc = glrtx_render_features(c, cur))) {  // (only an allocation or a launch can fail here: the planes and their camera are put back)
        std::swap(c->ftN.buf, c->ftN_spare);
        std::swap(c->ftA, c->ftA_spare);
        if (c->mt_on) std::swap(c->ftG, c->ftG_spare);
        std::memcpy(c->ft_cam, cam_prev, sizeof cam_prev);
        return rc;
    }
    const int pitch_f4 = (int)(c->pitch_bytes / sizeof(float4));
    const reproject::Common common =
        reproject_common(st, c->accum, (const float4 *)c->ftN_spare.p, (const float4 *)c->ftA_spare.p, (const float4 *)(motion ? c->ftG.p : c->ftN.buf.p),
                         (const float4 *)c->ftA.p, (float4 *)c->accum_spare.p, pitch_f4,
                         c->width, c->owned_rows, c->rpCount.p, carry_m ? (const float4 *)c->mmM.buf.p : nullptr, carry_m ? (float4 *)c->mmM_spare.p : nullptr);
    if (motion) rc = reproject_motion_pass(c, c->stream, common, (const float4 *)c->mtPos.p, (const float4 *)c->mtNrm.p, c->n_tri);
    else rc = reproject_pass(c, c->stream, common, cur->c2w, cur->s2c, c->stripe);
    if (rc) return rc;
    std::swap(c->accum_own, c->accum_spare);  // the accumulator rendered into from here on (glrtx_accum_device_ptr changes)
    c->accum = (float4 *)c->accum_own.p;
    c->rp_have = true;
    if (c->adHalf.buf.p && (rc = plane_zero(c, c->adHalf))) return rc;  // H held every second sample of the OLD view's pixels: zeroed, every tile is active again
    if (c->rwC.buf.p && (rc = plane_zero(c, c->rwC, reweight::kCascades))) return rc;  // C held the OLD pixel grid's bins: zeroed like H (carrying it is out of scope)
    if (carry_m) std::swap(c->mmM.buf, c->mmM_spare);  // M is CARRIED, not zeroed like H: a variance is a property of the surface point, and it came along with its mean
    return GLRTX_OK;
}

int glrtx_reproject(glrtx_ctx *c, const glrtx_params *cur, const glrtx_reproject_cfg *cfg) { return reproject_call(c, cur, cfg, "glrtx_reproject", false); }
int glrtx_reproject_motion(glrtx_ctx *c, const glrtx_params *cur, const glrtx_reproject_cfg *cfg) { return reproject_call(c, cur, cfg, "glrtx_reproject_motion", true); }

int glrtx_track_motion(glrtx_ctx *c, int enable) {
    if (!c) return GLRTX_EINVAL;
    const bool on = enable != 0;
    if (on == c->mt_on) return GLRTX_OK;
    if (!on) {  // forget the previous geometry and the planes: nothing may still read them
        seal_feed(c);
        if (int rc = glrtx_sync(c)) return rc;
        HIP_TRY(c, hipSetDevice(c->device));
        dev_free(c->ftG); dev_free(c->ftG_spare); dev_free(c->mtPos); dev_free(c->mtNrm);
    }
    c->mt_on = on;
    c->mt_g_have = false;
    c->mt_geom = glrtx_ctx::kMtNone;
    return GLRTX_OK;
}

int glrtx_read_features_geom(glrtx_ctx *c, float *geom, size_t pitch_bytes) {
    const char *fn = "glrtx_read_features_geom";
    if (!c || !geom) return GLRTX_EINVAL;
    if (!c->mt_on) return fail(c, GLRTX_EINVAL, "%s: motion tracking is off (glrtx_track_motion)", fn);
    if (int rc = denoise_shape_check(c, fn, false)) return rc;
    if (!c->ftG.p || !c->mt_g_have) return fail(c, GLRTX_EINVAL, "%s: no geometry plane (call glrtx_render_features with tracking on first)", fn);
    const size_t row = (size_t)c->width * sizeof(float4);
    if (pitch_bytes < row) return fail(c, GLRTX_EINVAL, "%s: pitch too small", fn);
    return read_back(c, c->ftG.p, row, geom, pitch_bytes);
}

int glrtx_reproject_last(glrtx_ctx *c, int *carried, int *hit_pixels) {
    const char *fn = "glrtx_reproject_last";
    if (!c) return GLRTX_EINVAL;
    if (!carried || !hit_pixels) return fail(c, GLRTX_EINVAL, "%s: NULL output", fn);
    if (!c->rp_have || !c->rpCount.p) return fail(c, GLRTX_EINVAL, "%s: no reprojection yet (or the image was resized since)", fn);
    if (int rc = glrtx_sync(c)) return rc;
    HIP_TRY(c, reproject_counts(c->rpCount.p, carried, hit_pixels));
    return GLRTX_OK;
}

}  // extern "C"
static int debug_reproject_impl(const char *fn, const float *accum, const float *mom, const float *n0, const float *a0, const float *n1, const float *a1,
                                const float *c2w_prev, const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows,
                                const glrtx_reproject_cfg *cfg, float *out, float *mom_out, int *carried, int *hit_pixels) {
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || (size_t)width * (size_t)rows > ((size_t)1 << 31))
        return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!accum || !n0 || !a0 || !n1 || !a1 || !c2w_prev || !s2c_prev || !c2w_cur || !s2c_cur || !cfg || !out) return fail(nullptr, GLRTX_EINVAL, "%s: NULL argument", fn);
    glrt_detail::ReprojectSetup st;
    if (int rc = reproject_setup_check(nullptr, fn, c2w_prev, s2c_prev, cfg, st)) return rc;
    const size_t bytes = (size_t)width * rows * sizeof(float4);
    DebugScratch s;
    const float4 *acc = s.alloc(bytes, accum), *N0 = s.alloc(bytes, n0), *A0 = s.alloc(bytes, a0), *N1 = s.alloc(bytes, n1), *A1 = s.alloc(bytes, a1);
    float4 *o = s.alloc(bytes);
    void *counts = s.alloc<void>(reproject::kCountBytes);
    const float4 *M = mom ? s.alloc(bytes, mom) : nullptr;
    float4 *Mo = mom ? s.alloc(bytes) : nullptr;
    int rc = GLRTX_OK;
    if (s.ok()) rc = reproject_pass(nullptr, 0, reproject_common(st, acc, N0, A0, N1, A1, o, width, width, rows, counts, M, Mo), c2w_cur, s2c_cur, 16);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(out, o, bytes);
        s.download(mom_out, Mo, bytes);
        if (s.ok()) s.e = reproject_counts(counts, carried, hit_pixels);
    }
    return s.result(rc, fn);
}
extern "C" {
int glrtx_debug_reproject(const float *accum, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev, const float *s2c_prev,
                          const float *c2w_cur, const float *s2c_cur, int width, int rows, const glrtx_reproject_cfg *cfg, float *out, int *carried, int *hit_pixels) {
    return debug_reproject_impl("glrtx_debug_reproject", accum, nullptr, n0, a0, n1, a1, c2w_prev, s2c_prev, c2w_cur, s2c_cur, width, rows, cfg, out, nullptr, carried,
                                hit_pixels);
}
int glrtx_debug_reproject_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *n1, const float *a1, const float *c2w_prev,
                                  const float *s2c_prev, const float *c2w_cur, const float *s2c_cur, int width, int rows, const glrtx_reproject_cfg *cfg, float *out,
                                  float *moments_out, int *carried, int *hit_pixels) {
    if (!moments || !moments_out) return fail(nullptr, GLRTX_EINVAL, "glrtx_debug_reproject_moments: NULL moments");
    return debug_reproject_impl("glrtx_debug_reproject_moments", accum, moments, n0, a0, n1, a1, c2w_prev, s2c_prev, c2w_cur, s2c_cur, width, rows, cfg, out,
                                moments_out, carried, hit_pixels);
}

}  // extern "C"
static int debug_reproject_motion_impl(const char *fn, const float *accum, const float *mom, const float *n0, const float *a0, const float *g1, const float *a1,
                                       const float *vert_prev, size_t n_vert, const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width,
                                       int rows, const glrtx_reproject_cfg *cfg, float *out, float *mom_out, int *carried, int *hit_pixels) {
    if (width < 1 || rows < 1 || width > 65536 || rows > 65536 || (size_t)width * (size_t)rows > ((size_t)1 << 31))
        return fail(nullptr, GLRTX_EINVAL, "%s: bad size %dx%d", fn, width, rows);
    if (!accum || !n0 || !a0 || !g1 || !a1 || !c2w_prev || !s2c_prev || !cfg || !out) return fail(nullptr, GLRTX_EINVAL, "%s: NULL argument", fn);
    if ((n_tri && (!tri || !vert_prev)) || n_tri > (size_t)INT32_MAX / 4) return fail(nullptr, GLRTX_EINVAL, "%s: NULL geometry or too many triangles", fn);
    glrt_detail::ReprojectSetup st;
    if (int rc = reproject_setup_check(nullptr, fn, c2w_prev, s2c_prev, cfg, st)) return rc;
    // the previous records as pack_scene forms a triangle's: {p0} {p1 - p0} {p2 - p0}, {n0} {n1} {n2}
    std::vector<float4> pos(3 * std::max<size_t>(n_tri, 1), make_float4(0.f, 0.f, 0.f, 0.f)), nrm(pos.size(), make_float4(0.f, 0.f, 0.f, 0.f));
    for (size_t t = 0; t < n_tri; t++) {
        const float *v[3];
        for (int k = 0; k < 3; k++) {
            const float f = tri[4 * t + k];
            if (!(f >= 0.0f) || (size_t)f >= n_vert) return fail(nullptr, GLRTX_EINVAL, "%s: triangle %zu: vertex index %g out of range", fn, t, (double)f);
            v[k] = vert_prev + 15 * (size_t)f;
        }
        pos[3 * t] = make_float4(v[0][0], v[0][1], v[0][2], 0.f);
        pos[3 * t + 1] = make_float4(v[1][0] - v[0][0], v[1][1] - v[0][1], v[1][2] - v[0][2], 0.f);
        pos[3 * t + 2] = make_float4(v[2][0] - v[0][0], v[2][1] - v[0][1], v[2][2] - v[0][2], 0.f);
        for (int k = 0; k < 3; k++) nrm[3 * t + k] = make_float4(v[k][3], v[k][4], v[k][5], 0.f);
    }
    const size_t bytes = (size_t)width * rows * sizeof(float4), gbytes = pos.size() * sizeof(float4);
    DebugScratch s;
    const float4 *acc = s.alloc(bytes, accum), *N0 = s.alloc(bytes, n0), *A0 = s.alloc(bytes, a0), *G1 = s.alloc(bytes, g1), *A1 = s.alloc(bytes, a1);
    const float4 *prev_pos = s.alloc(gbytes, pos.data()), *prev_nrm = s.alloc(gbytes, nrm.data());
    float4 *o = s.alloc(bytes);
    void *counts = s.alloc<void>(reproject::kCountBytes);
    const float4 *M = mom ? s.alloc(bytes, mom) : nullptr;
    float4 *Mo = mom ? s.alloc(bytes) : nullptr;
    int rc = GLRTX_OK;
    if (s.ok())
        rc = reproject_motion_pass(nullptr, 0, reproject_common(st, acc, N0, A0, G1, A1, o, width, width, rows, counts, M, Mo), prev_pos, prev_nrm, (int)n_tri);
    if (rc == GLRTX_OK) {
        s.sync();
        s.download(out, o, bytes);
        s.download(mom_out, Mo, bytes);
        if (s.ok()) s.e = reproject_counts(counts, carried, hit_pixels);
    }
    return s.result(rc, fn);
}
extern "C" {
int glrtx_debug_reproject_motion(const float *accum, const float *n0, const float *a0, const float *g1, const float *a1, const float *vert_prev, size_t n_vert,
                                 const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev, int width, int rows, const glrtx_reproject_cfg *cfg,
                                 float *out, int *carried, int *hit_pixels) {
    return debug_reproject_motion_impl("glrtx_debug_reproject_motion", accum, nullptr, n0, a0, g1, a1, vert_prev, n_vert, tri, n_tri, c2w_prev, s2c_prev, width, rows,
                                       cfg, out, nullptr, carried, hit_pixels);
}
int glrtx_debug_reproject_motion_moments(const float *accum, const float *moments, const float *n0, const float *a0, const float *g1, const float *a1,
                                         const float *vert_prev, size_t n_vert, const float *tri, size_t n_tri, const float *c2w_prev, const float *s2c_prev,
                                         int width, int rows, const glrtx_reproject_cfg *cfg, float *out, float *moments_out, int *carried, int *hit_pixels) {
    if (!moments || !moments_out) return fail(nullptr, GLRTX_EINVAL, "glrtx_debug_reproject_motion_moments: NULL moments");
    return debug_reproject_motion_impl("glrtx_debug_reproject_motion_moments", accum, moments, n0, a0, g1, a1, vert_prev, n_vert, tri, n_tri, c2w_prev, s2c_prev,
                                       width, rows, cfg, out, moments_out, carried, hit_pixels);
}

// glrtx_render behind the presentation check (glrtx_render_frames checks for all its frames at once)
static int render_one(glrtx_ctx *c, const glrtx_params *p, const RenderReq &req) {
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "glrtx_render: no scene uploaded");
    if (!c->accum || c->width < 1) return fail(c, GLRTX_EINVAL, "glrtx_render: no accumulator (call glrtx_resize)");
    if (p->n_samples < 0 || p->max_depth < 0) return fail(c, GLRTX_EINVAL, "glrtx_render: negative n_samples/max_depth");
    const Route route = route_of(c, p, req.kind);  // once; everything below reads it
    if (int rc = route_refusal(c, route, "glrtx_render")) return rc;  // (a call of another kind has asked for its own list before it got here: what is left is the volume's)
    HIP_TRY(c, hipSetDevice(c->device));
    const bool wavefront = on_wavefront(route);
    if (c->owned_rows > 0 && wavefront && req.kind == RenderReq::Ordinary && req.n_frames == 1 && feed_append(c, p, p->seed, 1) == 1) {  // a launch of the same camera that is still open takes the frame itself
        c->last_was_render = true; c->last_p = *p;
        return presenting(c) ? present_issue(c, 1) : GLRTX_OK;
    }
    if (!wavefront) seal_feed(c);
    c->st.launches++;
    if (c->owned_rows == 0) return req.presents(c) ? present_issue(c, req.n_frames) : GLRTX_OK;  // (images without rows: the frame numbers stay in step)

    KernelArgs a;
    a.sc = c->sc;
    static_assert(sizeof a.cam == kCamFloats * sizeof(float), "camera block layout");
    std::memcpy(a.cam, p->c2w, 16 * sizeof(float));
    std::memcpy(a.cam + 16, p->s2c, 16 * sizeof(float));
    a.cam[32] = p->aperture; a.cam[33] = p->focal;
    a.seed_x = p->seed[0]; a.seed_y = p->seed[1];
    a.n_samples = p->n_samples; a.max_depth = p->max_depth;
    a.width = c->width; a.height = c->height;
    a.owned_rows = c->owned_rows;
    a.rank = c->rank; a.world = c->world; a.stripe = c->stripe;
    a.accum = req.accum(c);
    a.pitch_f4 = (int)(c->pitch_bytes / sizeof(float4));
    a.ray_counter = (unsigned long long *)c->counter.p;
    a.hit_hist = req.hit_hist;  // (null outside glrtx_hit_histogram)
    a.tiles_x = (c->width + kTile - 1) / kTile;
    const int tiles_y = (c->owned_rows + kTile - 1) / kTile;
    a.n_tiles = a.tiles_x * tiles_y;

    // Host-side shape checks before launching a hand-written kernel.
    const int lds = lds_bytes_for(c->sc);
    if (lds > 160 * 1024) return fail(c, GLRTX_EDEVICE, "render kernel needs %d B of LDS (> 160 KiB)", lds);
    if (a.pitch_f4 < c->width) return fail(c, GLRTX_EINVAL, "accumulator pitch smaller than a row");

    if ((size_t)a.pitch_f4 * (size_t)c->owned_rows >= (size_t)INT32_MAX)
        return fail(c, GLRTX_EINVAL, "accumulator too large for 32-bit pixel offsets");

    // The kernel family, and -- not silently -- why variant 2 was left and a count of such launches: the route's
    c->st.variant_last = route.family;
    c->st.fallback_last = route.fallback;
    if (route.fallback_counts) c->st.fallback_launches++;
    if (wavefront) {
        const int rc = launch_wgwf(c, a, p, req, route);
        if (rc == GLRTX_OK) { c->last_was_render = true; c->last_p = *p; } else seal_feed(c);
        return rc;
    }
    glrtx_ctx::LaunchRec *rec = nullptr;
    if (int rc = next_launch_rec(c, rec)) return rc;
    if (route.family == glrt_detail::kRoutePersistent) {
        PersistLaunch k;
        if (int rc = persist_kernel(c, route, lds, k)) return rc;
        if (int rc = persist_launch(c, route, k, a, rec->ev0)) return rc;
    } else {
        static constexpr void (*kTileKernel[2])(const KernelArgs) = {pt_render_kernel<false>, pt_render_kernel<true>};  // [count_rays]
        const auto tk = kTileKernel[c->count_rays];
        HIP_TRY(c, hipEventRecord(rec->ev0, c->stream));
        c->last_kernel = route.kernel;
        if (lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void *)tk, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
        hipLaunchKernelGGL(tk, dim3(a.n_tiles), dim3(kBlockThreads), lds, c->stream, a);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipEventRecord(rec->evm, c->stream));
    HIP_TRY(c, hipEventRecord(rec->ev1, c->stream));
    rec->kernel = c->last_kernel; rec->frames = 1; rec->has_eva = false;
    c->ring_head++;
    c->counters_stale = c->counters_stale || c->count_rays;
    c->st.frames_last = 1;
    c->st.paths += (uint64_t)c->owned_rows * (uint64_t)c->width * (uint64_t)p->n_samples;
    if (presenting(c)) return present_resolve(c);  // (the megakernels accumulate by themselves: the resolve kernel behind them)
    return GLRTX_OK;
}

int glrtx_sync(glrtx_ctx *c) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->counters_stale && c->counter.p &&  // the device is idle here: bring the ray counters over now, so that glrtx_get_stats after a sync touches nothing
        hipMemcpy(c->counters_host, c->counter.p, sizeof c->counters_host, hipMemcpyDeviceToHost) == hipSuccess)
        c->counters_stale = false;
    return fold_launches(c, true);
}

int glrtx_read_accum(glrtx_ctx *c, float *dst, size_t dst_pitch_bytes) {
    if (!c || !dst) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!c->accum) return fail(c, GLRTX_EINVAL, "glrtx_read_accum: no accumulator");
    if (dst_pitch_bytes < (size_t)c->width * sizeof(float4)) return fail(c, GLRTX_EINVAL, "glrtx_read_accum: dst pitch too small");
    return read_back(c, c->accum, c->pitch_bytes, dst, dst_pitch_bytes);
}

int glrtx_accum_device_ptr(const glrtx_ctx *c, void **ptr_out, size_t *pitch_out) {
    if (!c || !ptr_out || !pitch_out) return GLRTX_EINVAL;
    seal_feed(const_cast<glrtx_ctx *>(c));  // (the caller is about to look at the accumulator: nothing more goes into a launch that is already queued in front of that)
    *ptr_out = c->accum;
    *pitch_out = c->pitch_bytes;
    return GLRTX_OK;
}

// resolve_kernel's instantiation for a call and its grid: kResolvePer pixels per lane; GLRTX_RESOLVE_PER=1/2/4 overrides (A/B; read at every call)
using ResolveFn = void (*)(const float4 *, int, int, int, uchar4 *, int, float, int);
struct ResolvePick { ResolveFn fn; dim3 grid; };
static ResolvePick resolve_pick(const glrtx_ctx *c) {
    int per = kResolvePer;
    if (const char *v = std::getenv("GLRTX_RESOLVE_PER")) per = std::atoi(v);
    per = per == 1 || per == 4 ? per : 2;
    return {per == 1 ? resolve_kernel<1> : (per == 4 ? resolve_kernel<4> : resolve_kernel<2>), resolve_grid(c->width, c->owned_rows, per)};
}

int glrtx_resolve_rgba8(glrtx_ctx *c, uint8_t *dst, size_t dst_pitch_bytes, float gamma, int flip_y) {
    if (!c || !dst) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (!c->accum) return fail(c, GLRTX_EINVAL, "glrtx_resolve_rgba8: no accumulator");
    if (!(gamma > 0.f)) return fail(c, GLRTX_EINVAL, "glrtx_resolve_rgba8: gamma must be positive");
    if (dst_pitch_bytes < (size_t)c->width * 4) return fail(c, GLRTX_EINVAL, "glrtx_resolve_rgba8: dst pitch too small");
    HIP_TRY(c, hipSetDevice(c->device));
    const int rc = resolve_to_caller(c, dst, dst_pitch_bytes, [&](uchar4 *out) {
        const ResolvePick rk = resolve_pick(c);
        HIP_TRY(c, hipEventRecord(c->rs0, c->stream));
        hipLaunchKernelGGL(rk.fn, rk.grid, dim3(256), 0, c->stream, (const float4 *)c->accum, (int)(c->pitch_bytes / sizeof(float4)),
                           c->width, c->owned_rows, out, c->width, 1.0f / gamma, flip_y ? 1 : 0);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->rs1, c->stream));
        return GLRTX_OK;
    });
    if (rc == GLRTX_OK && c->owned_rows > 0) HIP_TRY(c, hipEventElapsedTime(&c->st.resolve_ms_last, c->rs0, c->rs1));  // (the copy's sync has seen rs1)
    return rc;
}

// Device time of the resolve kernel by itself: `reps` launches back to back between one pair of events, per launch.  A single launch between two events (what
// glrtx_stats.resolve_ms_last reports) carries the command processor's latency on both sides -- ~6 us of a 15-us measurement at 1080p -- which says nothing about the kernel.
int glrtx_debug_resolve_burst(glrtx_ctx *c, float gamma, int reps, float *ms_per_launch) {
    if (!c || !ms_per_launch || reps < 1 || !(gamma > 0.f)) return GLRTX_EINVAL;
    seal_feed(c);
    if (!c->accum || c->owned_rows == 0) return fail(c, GLRTX_EINVAL, "glrtx_debug_resolve_burst: no accumulator");
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = ensure(c, c->rgba8, (size_t)c->width * 4 * (size_t)c->owned_rows)) return rc;
    const ResolvePick rk = resolve_pick(c);
    return burst_time(c, reps, ms_per_launch, [&] {
        hipLaunchKernelGGL(rk.fn, rk.grid, dim3(256), 0, c->stream, (const float4 *)c->accum, (int)(c->pitch_bytes / sizeof(float4)), c->width, c->owned_rows,
                           (uchar4 *)c->rgba8.p, c->width, 1.0f / gamma, 1);
        return GLRTX_OK;
    });
}

// Profile of a calibration frame: how often every triangle of the uploaded scene is the CLOSEST hit of a path ray (camera rays and bounces), counted by the render
// kernel itself while it shades one frame of `p` into a scratch accumulator -- the context's own accumulator, its statistics and its open launches are left alone.
// What it is for: glrt_bvh_order_by_hits (glrt_host.h) puts, at every fork, the child whose subtree is hit more often into the slot the reference's traversal visits
// first (raytrace.frag:299-307) -- a hit found early culls the sibling.  The order of a fork's children is the builder's choice (bvh.cpp:72-160); images stay the
// reference's for the re-ordered tree (exact ties between two triangles may resolve to the other one: INTEGRATION.md).
int glrtx_hit_histogram(glrtx_ctx *c, const glrtx_params *p, uint32_t *hist_out, size_t n_tri) {
    if (!c || !p || !hist_out) return GLRTX_EINVAL;
    seal_feed(c);
    if (!c->have_scene) return fail(c, GLRTX_EINVAL, "glrtx_hit_histogram: no scene uploaded");
    if (!c->accum || c->width < 1 || c->owned_rows < 1) return fail(c, GLRTX_EINVAL, "glrtx_hit_histogram: no image size (call glrtx_resize)");
    if (n_tri != (size_t)c->n_tri) return fail(c, GLRTX_EINVAL, "glrtx_hit_histogram: the scene has %d triangles, room for %zu", c->n_tri, n_tri);
    if (int rc = route_refusal(c, route_of(c, p, RenderReq::Calibration), "glrtx_hit_histogram")) return rc;
    HIP_TRY(c, hipSetDevice(c->device));
    if (int rc = glrtx_sync(c)) return rc;
    const size_t n_rec = c->leaf_tri.size() + 1;
    DevBuf hist, scratch;
    int rc = GLRTX_OK;
    const glrtx_stats st_was = c->st;
    if ((rc = ensure(c, hist, n_rec * sizeof(unsigned))) == GLRTX_OK && (rc = ensure(c, scratch, c->pitch_bytes * (size_t)c->owned_rows)) == GLRTX_OK) {
        hipError_t e = hipMemsetAsync(hist.p, 0, n_rec * sizeof(unsigned), c->stream);
        if (e == hipSuccess) e = hipMemsetAsync(scratch.p, 0, c->pitch_bytes * (size_t)c->owned_rows, c->stream);
        if (e != hipSuccess) rc = fail(c, GLRTX_EDEVICE, "glrtx_hit_histogram: %s", hipGetErrorString(e));
        if (rc == GLRTX_OK) {
            rc = render_one(c, p, RenderReq{RenderReq::Calibration, nullptr, 1, (unsigned *)hist.p, (float4 *)scratch.p});
            seal_feed(c);
            if (rc == GLRTX_OK) rc = glrtx_sync(c);
        }
        if (rc == GLRTX_OK) {
            std::vector<unsigned> h(n_rec);
            if (hipMemcpy(h.data(), hist.p, n_rec * sizeof(unsigned), hipMemcpyDeviceToHost) != hipSuccess) rc = fail(c, GLRTX_EDEVICE, "glrtx_hit_histogram: read-back failed");
            else {
                std::fill(hist_out, hist_out + n_tri, 0u);
                for (size_t k = 0; k + 1 < n_rec; k++) hist_out[c->leaf_tri[k]] += h[k + 1];
            }
        }
    }
    dev_free(hist); dev_free(scratch);
    c->st = st_was;  // (the calibration frame is not part of the caller's statistics)
    return rc;
}

int glrtx_get_stats(const glrtx_ctx *c, glrtx_stats *out) {
    if (!c || !out) return GLRTX_EINVAL;
    // a getter leaves the calling thread's current device as it found it
    int dev_before = -1;
    const bool have_dev = hipGetDevice(&dev_before) == hipSuccess;
    if (hipSetDevice(c->device) == hipSuccess) (void)fold_launches(const_cast<glrtx_ctx *>(c), false);  // launches that have finished; never waits, never consumes a failed one
    *out = c->st;
    // the ray counters live on the device; glrtx_sync brings them over, so after a sync this call touches nothing.  Only when a
    // counting launch was issued since the last sync / read are they fetched here (a blocking copy); polling the stats of a
    // non-counting render loop costs no device round trip
    if (c->counters_stale && c->counter.p && hipSetDevice(c->device) == hipSuccess &&
        hipMemcpy(c->counters_host, c->counter.p, sizeof c->counters_host, hipMemcpyDeviceToHost) == hipSuccess)
        c->counters_stale = false;
    out->rays = c->counters_host[0]; out->rays_untraced = c->counters_host[1];
    out->shadow_limited = c->sc.shadow_limited;
    if (have_dev && dev_before != c->device) (void)hipSetDevice(dev_before);
    return GLRTX_OK;
}

int glrtx_reset_stats(glrtx_ctx *c) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    if (int rc = glrtx_sync(c)) return rc;
    HIP_TRY(c, hipMemset(c->counter.p, 0, 2 * sizeof(unsigned long long)));
    c->counters_host[0] = c->counters_host[1] = 0; c->counters_stale = false;
    c->st.rays = 0; c->st.rays_untraced = 0; c->st.paths = 0; c->st.launches = 0; c->st.kernel_launches = 0; c->st.kernel_ms_total = 0.0; c->st.accumulate_ms_total = 0.0; c->st.kernel_ms_last = 0.f; c->st.fallback_launches = 0; c->st.pipe_resident_max = 0; c->st.feed_launches = 0; c->st.feed_appended = 0;
    return GLRTX_OK;
}

int glrtx_present_enable(glrtx_ctx *c, int ring_images, float gamma, int flip_y) {
    if (!c) return GLRTX_EINVAL;
    return present_start(c, ring_images, gamma, flip_y, false);
}

int glrtx_present_acquire(glrtx_ctx *c, int wait, glrtx_image *out) {
    if (!c || !out) return GLRTX_EINVAL;
    glrtx_ctx::Present &P = c->pres;
    if (P.ring == 0) return fail(c, GLRTX_EINVAL, "glrtx_present_acquire: presentation is off (glrtx_present_enable)");
    if (P.acq == P.seq) { P.st.busy_returns++; return fail(c, GLRTX_EBUSY, "glrtx_present_acquire: no frame rendered since the last image was acquired"); }
    glrtx_ctx::Present::Image &im = P.img[P.acq % P.ring];
    HIP_TRY(c, hipSetDevice(c->device));
    const hipError_t e = wait ? hipEventSynchronize(im.ev) : hipEventQuery(im.ev);
    if (e == hipErrorNotReady) { (void)hipGetLastError(); P.st.busy_returns++; return fail(c, GLRTX_EBUSY, "glrtx_present_acquire: the next image is not ready"); }
    if (e != hipSuccess) return fail(c, GLRTX_EDEVICE, "glrtx_present_acquire: the image's copy failed: %s", hipGetErrorString(e));
    im.state = glrtx_ctx::Present::Image::HELD;
    P.acq++;
    P.st.delivered++;
    out->rgba = im.host;
    out->pitch_bytes = (size_t)im.width * 4;
    out->width = im.width;
    out->rows = im.rows;
    out->frame = im.frame;
    return GLRTX_OK;
}

int glrtx_present_release(glrtx_ctx *c, const glrtx_image *img) {
    if (!c || !img) return GLRTX_EINVAL;
    for (auto &im : c->pres.img)
        if (im.state == glrtx_ctx::Present::Image::HELD && im.host == img->rgba) { im.state = glrtx_ctx::Present::Image::FREE; return GLRTX_OK; }
    return fail(c, GLRTX_EINVAL, "glrtx_present_release: not an acquired image of this context");
}

int glrtx_present_get_stats(const glrtx_ctx *c, glrtx_present_stats *out) {
    if (!c || !out) return GLRTX_EINVAL;
    glrtx_ctx::Present &P = const_cast<glrtx_ctx *>(c)->pres;
    if (P.timed && P.t1) {  // the last pass, once it has completed (never waits)
        int dev_before = -1;
        const bool have_dev = hipGetDevice(&dev_before) == hipSuccess;
        if (hipSetDevice(c->device) == hipSuccess && hipEventQuery(P.t1) == hipSuccess) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, P.t0, P.t1) == hipSuccess) P.st.pass_ms_last = ms;
            P.timed = false;
        }
        (void)hipGetLastError();
        if (have_dev && dev_before != c->device) (void)hipSetDevice(dev_before);
    }
    *out = P.st;
    out->ring_images = P.ring;
    out->pending = (int32_t)(P.seq - P.acq);
    out->held = 0;
    for (const auto &im : P.img) out->held += im.state == glrtx_ctx::Present::Image::HELD;
    out->copies_last = P.copies_last;
    return GLRTX_OK;
}

#ifdef GLRTX_TRAV_STATS
int glrtx_debug_trav_stats(unsigned long long out[8]) { return take_symbol(g_trav_stats, out); }
int glrtx_debug_trav_trips(unsigned long long out[4]) { return take_symbol(g_trav_trips, out); }
int glrtx_debug_trav_sp_hist(unsigned long long out[16]) { return take_symbol(g_trav_sp_hist, out); }
int glrtx_debug_trav_hist(unsigned long long out[16]) { return take_symbol(g_trav_hist, out); }
#endif

#ifdef GLRTX_RAY_LOG
// diagnostic build only (tools/gpu_replay.py): record the ray queues of the following launches / replay their traverse phases alone
int glrtx_debug_ray_log_begin(glrtx_ctx *c, unsigned long long max_rays, unsigned max_trips) {
    if (!c) return GLRTX_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    int rc;
    if ((rc = ensure(c, g_dbg_log_rays, (size_t)max_rays * 2 * sizeof(float4)))) return rc;
    if ((rc = ensure(c, g_dbg_log_trips, (size_t)max_trips * sizeof(uint2)))) return rc;
    RayLog lg{(float4 *)g_dbg_log_rays.p, (uint2 *)g_dbg_log_trips.p, max_rays, max_trips, max_rays > 0 ? 1u : 0u};
    unsigned long long z = 0; unsigned zt = 0;
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_ray_log), &lg, sizeof lg));
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_ray_log_n), &z, sizeof z));
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_ray_log_trips), &zt, sizeof zt));
    return GLRTX_OK;
}
// the log's ray records (2 float4 each) and trips to / from the host: reordering experiments (tools/gpu_replay.py)
int glrtx_debug_ray_log_copy(glrtx_ctx *c, float *rays_host, unsigned long long n_records, unsigned *trips_host, unsigned n_trips, int to_device) {
    if (!c) return GLRTX_EINVAL;
    if (int rc = glrtx_sync(c)) return rc;
    if ((size_t)n_records * 32 > g_dbg_log_rays.bytes || (size_t)n_trips * 8 > g_dbg_log_trips.bytes) return fail(c, GLRTX_EINVAL, "ray log: copy larger than the log");
    if (rays_host) HIP_TRY(c, to_device ? hipMemcpy(g_dbg_log_rays.p, rays_host, (size_t)n_records * 32, hipMemcpyHostToDevice)
                                        : hipMemcpy(rays_host, g_dbg_log_rays.p, (size_t)n_records * 32, hipMemcpyDeviceToHost));
    if (trips_host) HIP_TRY(c, to_device ? hipMemcpy(g_dbg_log_trips.p, trips_host, (size_t)n_trips * 8, hipMemcpyHostToDevice)
                                         : hipMemcpy(trips_host, g_dbg_log_trips.p, (size_t)n_trips * 8, hipMemcpyDeviceToHost));
    return GLRTX_OK;
}
// stops recording and runs the traverse phase alone over the log `reps` times; out: {ms of the last replay, rays logged, trips logged, rays offered}
int glrtx_debug_ray_log_replay(glrtx_ctx *c, int reps, double out[4]) {
    if (!c) return GLRTX_EINVAL;
    if (int rc = glrtx_sync(c)) return rc;
    RayLog lg{};
    unsigned long long n = 0; unsigned nt = 0;
    HIP_TRY(c, hipMemcpyFromSymbol(&lg, HIP_SYMBOL(g_ray_log), sizeof lg));
    HIP_TRY(c, hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_ray_log_n), sizeof n));
    HIP_TRY(c, hipMemcpyFromSymbol(&nt, HIP_SYMBOL(g_ray_log_trips), sizeof nt));
    lg.on = 0u;
    HIP_TRY(c, hipMemcpyToSymbol(HIP_SYMBOL(g_ray_log), &lg, sizeof lg));
    nt = std::min(nt, lg.cap_trips);
    std::vector<uint2> tr(nt);
    HIP_TRY(c, hipMemcpy(tr.data(), lg.trips, (size_t)nt * sizeof(uint2), hipMemcpyDeviceToHost));
    unsigned long long logged = 0;
    for (const uint2 &t : tr) logged += t.y;
    DbgLastLaunch L = g_dbg_last;
    L.w.suspend_max = 0;
    using RKernel = void (*)(const KernelArgs, const WfArgs, unsigned *, float4 *, const float4 *, const uint2 *, int);
    int fetch = L.fetch;
    if (const char *v = std::getenv("GLRTX_REPLAY_PAIR_FETCH")) fetch = std::max(0, std::min(2, std::atoi(v)));  // the same log through another form of the node fetch
    const RKernel rk = fetch == 2 ? (RKernel)pt_replay_traverse<2> : fetch == 1 ? (RKernel)pt_replay_traverse<1> : (RKernel)pt_replay_traverse<0>;
    if (L.lds > 64 * 1024) HIP_TRY(c, hipFuncSetAttribute((const void *)rk, hipFuncAttributeMaxDynamicSharedMemorySize, L.lds));
    int per_cu = 0;
    HIP_TRY(c, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, rk, kBlockThreads, L.lds));
    if (const char *v = std::getenv("GLRTX_WGS_PER_CU")) per_cu = std::max(1, std::min(per_cu, std::atoi(v)));
    const int grid = std::max(1, std::min(L.grid, per_cu * c->n_cu));
    float ms = 0.f;
    for (int r = 0; r < reps; r++) {
        HIP_TRY(c, hipMemsetAsync(c->work.p, 0, sizeof(unsigned), c->stream));
        HIP_TRY(c, hipEventRecord(c->tm0, c->stream));
        hipLaunchKernelGGL(rk, dim3(grid), dim3(kBlockThreads), L.lds, c->stream, L.a, L.w, (unsigned *)c->work.p, L.queues,
                           (const float4 *)lg.rays, (const uint2 *)lg.trips, (int)nt);
        HIP_TRY(c, hipGetLastError());
        HIP_TRY(c, hipEventRecord(c->tm1, c->stream));
        HIP_TRY(c, hipEventSynchronize(c->tm1));
        HIP_TRY(c, hipEventElapsedTime(&ms, c->tm0, c->tm1));
    }
    out[0] = ms; out[1] = (double)logged; out[2] = (double)nt; out[3] = (double)n;
    return GLRTX_OK;
}
#endif

#ifdef GLRTX_STEP_TIMING
int glrtx_debug_step_timing(unsigned long long out[4]) { return take_symbol(g_step_timing, out); }
#endif

#ifdef GLRTX_PHASE_STATS
int glrtx_debug_trip_log(unsigned out[16 * 64 * 4]) { return take_symbol(g_trip_log, out); }
int glrtx_debug_phase_cycles(unsigned long long out[8]) { return take_symbol(g_phase_cycles, out); }
#endif

int glrtx_timer_begin(glrtx_ctx *c) {
    if (!c) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventRecord(c->tm0, c->stream));
    return GLRTX_OK;
}

int glrtx_timer_end(glrtx_ctx *c, float *ms) {
    if (!c || !ms) return GLRTX_EINVAL;
    seal_feed(c);  // (nothing is appended to an open launch across this call: glrtx_ctx::OpenFeed)
    HIP_TRY(c, hipSetDevice(c->device));
    HIP_TRY(c, hipEventRecord(c->tm1, c->stream));
    HIP_TRY(c, hipEventSynchronize(c->tm1));
    HIP_TRY(c, hipEventElapsedTime(ms, c->tm0, c->tm1));
    return GLRTX_OK;
}

// ---------------------------------------------------------------------------------------------------------------- groups
// Several contexts -- one per GPU of the node -- behind one handle, driven by one host thread: the multi-GPU form of the
// same entry points.  Context i owns the 8-row stripes s with s % n == i (glrtx_set_partition), renders
// them on its own stream with global pixel coordinates, and keeps its accumulator rows resident.  Nothing is exchanged while
// rendering.  Only when an image is wanted (read_accum / resolve) are the stripes copied, device to device, into a full-frame
// buffer on the first context's GPU (peer copies over xGMI; hipMemcpyPeerAsync also serves the same-device case the tests use).
}  // extern "C"

struct glrtx_group {
    std::vector<glrtx_ctx *> ctx;
    std::vector<hipEvent_t> done;  // per context: "its render stream has reached this point"
    DevBuf full, full8;            // on ctx[0]'s device: gathered accumulator (pitch = ctx[0]'s), resolved RGBA8
    std::vector<char> peer_ok;     // per context: its device can write the root's memory directly (same device, or peer access enabled)
    int gather_copies = 0;         // copies the last gather issued (tests)
    int width = 0, height = 0;
    std::vector<uint8_t *> pres_host;  // presentation: the full pinned images the members land their stripes in (glrtx_group_present_enable)
    std::vector<size_t> pres_bytes;
    std::string err;
};

namespace {

int gfail(glrtx_group *g, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g) g->err = buf; else g_create_error = buf;
    return code;
}
// forward a member context's failure
int gsub(glrtx_group *g, int i, int rc) {
    if (rc != GLRTX_OK) g->err = "context " + std::to_string(i) + " (device " + std::to_string(g->ctx[i]->device) + "): " + g->ctx[i]->err;
    return rc;
}
#define GHIP_TRY(g, call)                                                                       \
    do {                                                                                        \
        hipError_t e_ = (call);                                                                 \
        if (e_ != hipSuccess) return gfail(g, GLRTX_EDEVICE, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// All stripes -> g->full on ctx[0]'s device, ordered behind every context's outstanding work.  ONE strided copy per member
// (hipMemcpy2DAsync: a row of the copy is a whole stripe -- stripe x pitch bytes, contiguous on both sides -- the source steps by a
// stripe, the destination by world stripes), plus one for a partial last stripe, issued on the MEMBER's own stream right behind its
// render work: the members' copies run side by side over their own xGMI links, and the root stream only waits for their events.
// (Round 2 issued every stripe as its own hipMemcpyPeerAsync on the root's stream: 135 serialised copies at 1080p / 8 members.)
// Members without peer access to the root's memory fall back to hipMemcpyPeerAsync per stripe on the root's stream.
int group_gather(glrtx_group *g) {
    for (glrtx_ctx *m : g->ctx) seal_feed(m);  // (the copies read the members' accumulators in stream order: nothing is appended to a launch queued in front of them)
    glrtx_ctx *r = g->ctx[0];
    if (g->width < 1) return gfail(g, GLRTX_EINVAL, "glrtx_group: call glrtx_group_resize first");
    const size_t pitch = r->pitch_bytes;
    GHIP_TRY(g, hipSetDevice(r->device));
    if (g->full.bytes < pitch * (size_t)g->height) {
        dev_free(g->full);
        GHIP_TRY(g, hipMalloc(&g->full.p, pitch * (size_t)g->height));
        g->full.bytes = pitch * (size_t)g->height;
    }
    const int n = (int)g->ctx.size();
    g->gather_copies = 0;
    for (int i = 0; i < n; i++) {
        glrtx_ctx *c = g->ctx[i];
        if (c->pitch_bytes != pitch) return gfail(g, GLRTX_EINVAL, "glrtx_group: member accumulators have different pitches");
        if (c->owned_rows == 0) continue;
        const size_t stripe_b = (size_t)c->stripe * pitch;
        const int full_stripes = c->owned_rows / c->stripe, tail_rows = c->owned_rows % c->stripe;
        char *dst0 = (char *)g->full.p + (size_t)c->rank * stripe_b;  // stripe s of this member lies at global stripe s * world + rank
        if (g->peer_ok[i]) {
            GHIP_TRY(g, hipSetDevice(c->device));
            if (full_stripes > 0) {
                GHIP_TRY(g, hipMemcpy2DAsync(dst0, (size_t)c->world * stripe_b, c->accum, stripe_b, stripe_b, (size_t)full_stripes, hipMemcpyDeviceToDevice, c->stream));
                g->gather_copies++;
            }
            if (tail_rows > 0) {
                GHIP_TRY(g, hipMemcpyAsync(dst0 + (size_t)full_stripes * c->world * stripe_b, (const char *)c->accum + (size_t)full_stripes * stripe_b,
                                           (size_t)tail_rows * pitch, hipMemcpyDeviceToDevice, c->stream));
                g->gather_copies++;
            }
            GHIP_TRY(g, hipEventRecord(g->done[i], c->stream));
            GHIP_TRY(g, hipSetDevice(r->device));
            GHIP_TRY(g, hipStreamWaitEvent(r->stream, g->done[i], 0));
        } else {
            GHIP_TRY(g, hipSetDevice(c->device));
            GHIP_TRY(g, hipEventRecord(g->done[i], c->stream));
            GHIP_TRY(g, hipSetDevice(r->device));
            GHIP_TRY(g, hipStreamWaitEvent(r->stream, g->done[i], 0));
            for (int row = 0; row < c->owned_rows; row += c->stripe) {  // one contiguous block per stripe
                const int rows = std::min(c->stripe, c->owned_rows - row);
                const int y = ((row / c->stripe) * c->world + c->rank) * c->stripe;
                GHIP_TRY(g, hipMemcpyPeerAsync((char *)g->full.p + (size_t)y * pitch, r->device, (const char *)c->accum + (size_t)row * pitch, c->device,
                                               (size_t)rows * pitch, r->stream));
                g->gather_copies++;
            }
        }
    }
    return GLRTX_OK;
}

// Presentation, before a group render call of n frames: every member has a free image for each of them (else GLRTX_EBUSY, nothing changed), and the pinned full images
// those frames go to hold the current size (an image is only reallocated while it is free in every member).
int group_present_prepare(glrtx_group *g, int n) {
    if (g->pres_host.empty() || n < 1) return GLRTX_OK;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, present_prepare(g->ctx[i], n))) return rc;
    glrtx_ctx::Present &P0 = g->ctx[0]->pres;
    const size_t bytes = std::max<size_t>((size_t)g->width * 4 * (size_t)g->height, 64);
    for (int k = 0; k < n; k++) {
        const size_t at = (size_t)((P0.seq + k) % (uint64_t)P0.ring);
        if (g->pres_bytes[at] >= bytes) continue;
        if (g->pres_host[at]) GHIP_TRY(g, hipHostFree(g->pres_host[at]));
        g->pres_host[at] = nullptr; g->pres_bytes[at] = 0;
        GHIP_TRY(g, hipHostMalloc((void **)&g->pres_host[at], bytes, hipHostMallocPortable));
        g->pres_bytes[at] = bytes;
        for (glrtx_ctx *m : g->ctx) m->pres.img[at].host = g->pres_host[at];
    }
    return GLRTX_OK;
}

int group_present_stop(glrtx_group *g) {
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, present_stop(g->ctx[i]))) return rc;
    for (uint8_t *h : g->pres_host)
        if (h) (void)hipHostFree(h);
    g->pres_host.clear();
    g->pres_bytes.clear();
    return GLRTX_OK;
}

}  // namespace

extern "C" {

int glrtx_group_create(glrtx_group **out, const int *device_ids, int n_devices) {
    if (!out) return gfail(nullptr, GLRTX_EINVAL, "glrtx_group_create: out is NULL");
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return gfail(nullptr, GLRTX_EINVAL, "glrtx_group_create: need 1..64 device ids");
    glrtx_group *g = new (std::nothrow) glrtx_group;
    if (!g) return gfail(nullptr, GLRTX_ENOMEM, "out of host memory");
    for (int i = 0; i < n_devices; i++) {
        glrtx_ctx *c = nullptr;
        const int rc = glrtx_create(&c, device_ids[i]);
        if (rc != GLRTX_OK) { glrtx_group_destroy(g); return rc; }  // message already in the create-error slot
        g->ctx.push_back(c);
        hipEvent_t ev = nullptr;
        if (hipSetDevice(c->device) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            glrtx_group_destroy(g);
            return gfail(nullptr, GLRTX_EDEVICE, "glrtx_group_create: event creation failed on device %d", device_ids[i]);
        }
        g->done.push_back(ev);
    }
    // every member's device gets direct access to the root's memory where the platform offers it (its gather copy then runs on its own
    // stream over its own link); without it that member's stripes are copied by the root with hipMemcpyPeerAsync
    g->peer_ok.assign((size_t)n_devices, 1);
    for (int i = 1; i < n_devices; i++) {
        if (g->ctx[i]->device == g->ctx[0]->device) continue;
        int can = 0;
        g->peer_ok[i] = 0;
        if (hipDeviceCanAccessPeer(&can, g->ctx[i]->device, g->ctx[0]->device) == hipSuccess && can) {
            (void)hipSetDevice(g->ctx[i]->device);
            const hipError_t e = hipDeviceEnablePeerAccess(g->ctx[0]->device, 0);
            (void)hipGetLastError();  // "already enabled" is fine
            if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) g->peer_ok[i] = 1;
        }
    }
    // members that share a GPU also share its memory: the frames-in-flight budget is split between them
    for (int i = 0; i < n_devices; i++) {
        int same = 0;
        for (int j = 0; j < n_devices; j++) same += g->ctx[j]->device == g->ctx[i]->device;
        g->ctx[i]->budget_share = same;
    }
    *out = g;
    return GLRTX_OK;
}

void glrtx_group_destroy(glrtx_group *g) {
    if (!g) return;
    for (glrtx_ctx *c : g->ctx)  // (the members' copies land in the group's pinned images: they end first)
        if (c->pres.copy) { (void)hipSetDevice(c->device); (void)hipStreamSynchronize(c->pres.copy); }
    for (uint8_t *h : g->pres_host)
        if (h) (void)hipHostFree(h);
    for (size_t i = 0; i < g->done.size(); i++) { (void)hipSetDevice(g->ctx[i]->device); (void)hipEventDestroy(g->done[i]); }
    if (!g->ctx.empty()) { (void)hipSetDevice(g->ctx[0]->device); (void)hipStreamSynchronize(g->ctx[0]->stream); dev_free(g->full); dev_free(g->full8); }
    for (glrtx_ctx *c : g->ctx) glrtx_destroy(c);
    delete g;
}

const char *glrtx_group_last_error(const glrtx_group *g) { return g ? g->err.c_str() : g_create_error.c_str(); }
int glrtx_group_size(const glrtx_group *g) { return g ? (int)g->ctx.size() : 0; }
glrtx_ctx *glrtx_group_ctx(glrtx_group *g, int i) { return (g && i >= 0 && i < (int)g->ctx.size()) ? g->ctx[i] : nullptr; }

int glrtx_group_upload_scene(glrtx_group *g, const float *vert, size_t n_vert, const float *tri, size_t n_tri, const float *mat, size_t n_mat,
                             const float *light, size_t n_light, const float *bvh, size_t n_nodes) {
    if (!g) return GLRTX_EINVAL;
    for (size_t i = 0; i < g->ctx.size(); i++)  // the scene is replicated: <= 27 MB even for 100k triangles
        if (int rc = gsub(g, (int)i, glrtx_upload_scene(g->ctx[i], vert, n_vert, tri, n_tri, mat, n_mat, light, n_light, bvh, n_nodes))) return rc;
    return GLRTX_OK;
}

int glrtx_group_update_vertices(glrtx_group *g, const float *vert, size_t n_vert) {
    if (!g) return GLRTX_EINVAL;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, glrtx_update_vertices(g->ctx[i], vert, n_vert))) return rc;
    return GLRTX_OK;
}

int glrtx_group_upload_volume(glrtx_group *g, const float *density, const float *temperature, int nx, int ny, int nz, const float bbox_min[3],
                              const float bbox_max[3], float density_max) {
    if (!g) return fail(nullptr, GLRTX_EINVAL, "glrtx_group_upload_volume: NULL group");
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, glrtx_upload_volume(g->ctx[i], density, temperature, nx, ny, nz, bbox_min, bbox_max, density_max))) return rc;
    return GLRTX_OK;
}

int glrtx_group_resize(glrtx_group *g, int width, int height) {
    if (!g) return GLRTX_EINVAL;
    const int n = (int)g->ctx.size();
    for (int i = 0; i < n; i++) {
        glrtx_ctx *c = g->ctx[i];
        c->rank = i; c->world = n; c->stripe = kGroupStripe;  // == glrtx_set_partition(c, i, n, 8) without the intermediate resize
        if (int rc = gsub(g, i, glrtx_resize(c, width, height))) return rc;
    }
    g->width = width; g->height = height;
    return GLRTX_OK;
}

int glrtx_group_clear(glrtx_group *g) {
    if (!g) return GLRTX_EINVAL;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, glrtx_clear(g->ctx[i]))) return rc;
    return GLRTX_OK;
}

int glrtx_group_render(glrtx_group *g, const glrtx_params *p) {
    if (!g) return GLRTX_EINVAL;
    if (int rc = group_present_prepare(g, 1)) return rc;
    for (size_t i = 0; i < g->ctx.size(); i++)  // asynchronous launches: the GPUs run concurrently
        if (int rc = gsub(g, (int)i, glrtx_render(g->ctx[i], p))) return rc;
    return GLRTX_OK;
}

int glrtx_group_render_frames(glrtx_group *g, const glrtx_params *p, const float *seeds_xy, int n_frames) {
    if (!g) return GLRTX_EINVAL;
    if (int rc = group_present_prepare(g, n_frames)) return rc;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, glrtx_render_frames(g->ctx[i], p, seeds_xy, n_frames))) return rc;
    return GLRTX_OK;
}

int glrtx_group_render_adaptive(glrtx_group *g, const glrtx_params *p, const float *seeds_xy, int n_frames, const glrtx_adaptive *cfg) {
    if (!g) return GLRTX_EINVAL;
    for (size_t i = 0; i < g->ctx.size(); i++)  // (every member's refusals before any member changes anything)
        if (int rc = gsub(g, (int)i, adapt_check(g->ctx[i], p, seeds_xy, n_frames, cfg))) return rc;
    for (size_t i = 0; i < g->ctx.size(); i++)  // each member selects on its own accumulator
        if (int rc = gsub(g, (int)i, glrtx_render_adaptive(g->ctx[i], p, seeds_xy, n_frames, cfg))) return rc;
    return GLRTX_OK;
}

int glrtx_group_adaptive_active_tiles(glrtx_group *g, int *active, int *total) {
    if (!g || !active || !total) return GLRTX_EINVAL;
    int a = 0, t = 0;
    for (size_t i = 0; i < g->ctx.size(); i++) {
        int ai = 0, ti = 0;
        if (int rc = gsub(g, (int)i, glrtx_adaptive_active_tiles(g->ctx[i], &ai, &ti))) return rc;
        a += ai; t += ti;
    }
    *active = a; *total = t;
    return GLRTX_OK;
}

int glrtx_group_sync(glrtx_group *g) {
    if (!g) return GLRTX_EINVAL;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, glrtx_sync(g->ctx[i]))) return rc;
    return GLRTX_OK;
}

int glrtx_group_read_accum(glrtx_group *g, float *dst, size_t dst_pitch_bytes) {
    if (!g || !dst) return GLRTX_EINVAL;
    if (dst_pitch_bytes < (size_t)g->width * sizeof(float4)) return gfail(g, GLRTX_EINVAL, "glrtx_group_read_accum: dst pitch too small");
    if (int rc = group_gather(g)) return rc;
    glrtx_ctx *r = g->ctx[0];
    GHIP_TRY(g, hipStreamSynchronize(r->stream));
    GHIP_TRY(g, hipMemcpy2D(dst, dst_pitch_bytes, g->full.p, r->pitch_bytes, (size_t)g->width * sizeof(float4), (size_t)g->height, hipMemcpyDeviceToHost));
    return glrtx_group_sync(g);
}

int glrtx_group_resolve_rgba8(glrtx_group *g, uint8_t *dst, size_t dst_pitch_bytes, float gamma, int flip_y) {
    if (!g || !dst) return GLRTX_EINVAL;
    if (!(gamma > 0.f)) return gfail(g, GLRTX_EINVAL, "glrtx_group_resolve_rgba8: gamma must be positive");
    if (dst_pitch_bytes < (size_t)g->width * 4) return gfail(g, GLRTX_EINVAL, "glrtx_group_resolve_rgba8: dst pitch too small");
    if (int rc = group_gather(g)) return rc;
    glrtx_ctx *r = g->ctx[0];
    const size_t bytes = (size_t)g->width * 4 * (size_t)g->height;
    if (g->full8.bytes < bytes) {
        dev_free(g->full8);
        GHIP_TRY(g, hipMalloc(&g->full8.p, bytes));
        g->full8.bytes = bytes;
    }
    const dim3 grid = resolve_grid(g->width, g->height);
    hipLaunchKernelGGL(resolve_kernel<kResolvePer>, grid, dim3(256), 0, r->stream, (const float4 *)g->full.p, (int)(r->pitch_bytes / sizeof(float4)), g->width, g->height,
                       (uchar4 *)g->full8.p, g->width, 1.0f / gamma, flip_y ? 1 : 0);
    GHIP_TRY(g, hipGetLastError());
    GHIP_TRY(g, hipStreamSynchronize(r->stream));
    GHIP_TRY(g, hipMemcpy2D(dst, dst_pitch_bytes, g->full8.p, (size_t)g->width * 4, (size_t)g->width * 4, (size_t)g->height, hipMemcpyDeviceToHost));
    return glrtx_group_sync(g);
}

int glrtx_group_gather_copies(const glrtx_group *g) { return g ? g->gather_copies : 0; }

int glrtx_group_present_enable(glrtx_group *g, int ring_images, float gamma, int flip_y) {
    if (!g) return GLRTX_EINVAL;
    if (int rc = group_present_stop(g)) return rc;
    if (ring_images == 0) return GLRTX_OK;
    if (g->width < 1) return gfail(g, GLRTX_EINVAL, "glrtx_group_present_enable: call glrtx_group_resize first");
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, present_start(g->ctx[i], ring_images, gamma, flip_y, true))) { (void)group_present_stop(g); return rc; }
    g->pres_host.assign((size_t)ring_images, nullptr);
    g->pres_bytes.assign((size_t)ring_images, 0);
    const size_t bytes = std::max<size_t>((size_t)g->width * 4 * (size_t)g->height, 64);
    for (int k = 0; k < ring_images; k++) {  // (up front: pinning memory waits for the device)
        if (hipHostMalloc((void **)&g->pres_host[k], bytes, hipHostMallocPortable) != hipSuccess) {
            g->pres_host[k] = nullptr;
            (void)group_present_stop(g);
            return gfail(g, GLRTX_ENOMEM, "glrtx_group_present_enable: %zu bytes of pinned host memory", bytes);
        }
        g->pres_bytes[k] = bytes;
        for (glrtx_ctx *m : g->ctx) m->pres.img[k].host = g->pres_host[k];
    }
    return GLRTX_OK;
}

int glrtx_group_present_acquire(glrtx_group *g, int wait, glrtx_image *out) {
    if (!g || !out) return GLRTX_EINVAL;
    if (g->pres_host.empty()) return gfail(g, GLRTX_EINVAL, "glrtx_group_present_acquire: presentation is off (glrtx_group_present_enable)");
    glrtx_ctx::Present &P0 = g->ctx[0]->pres;
    if (P0.acq == P0.seq) { P0.st.busy_returns++; return gfail(g, GLRTX_EBUSY, "glrtx_group_present_acquire: no frame rendered since the last image was acquired"); }
    for (glrtx_ctx *m : g->ctx) {  // the image is there when every member's stripes are
        glrtx_ctx::Present::Image &im = m->pres.img[m->pres.acq % m->pres.ring];
        GHIP_TRY(g, hipSetDevice(m->device));
        const hipError_t e = wait ? hipEventSynchronize(im.ev) : hipEventQuery(im.ev);
        if (e == hipErrorNotReady) { (void)hipGetLastError(); P0.st.busy_returns++; return gfail(g, GLRTX_EBUSY, "glrtx_group_present_acquire: the next image is not ready"); }
        if (e != hipSuccess) return gfail(g, GLRTX_EDEVICE, "glrtx_group_present_acquire: a member's copy failed (device %d): %s", m->device, hipGetErrorString(e));
    }
    const glrtx_ctx::Present::Image &im0 = P0.img[P0.acq % P0.ring];
    out->rgba = im0.host;
    out->pitch_bytes = (size_t)im0.width * 4;
    out->width = im0.width;
    out->rows = im0.rows;
    out->frame = im0.frame;
    for (glrtx_ctx *m : g->ctx) {
        m->pres.img[m->pres.acq % m->pres.ring].state = glrtx_ctx::Present::Image::HELD;
        m->pres.acq++;
        m->pres.st.delivered++;
    }
    return GLRTX_OK;
}

int glrtx_group_present_release(glrtx_group *g, const glrtx_image *img) {
    if (!g || !img) return GLRTX_EINVAL;
    for (size_t i = 0; i < g->ctx.size(); i++)
        if (int rc = gsub(g, (int)i, glrtx_present_release(g->ctx[i], img))) return rc;
    return GLRTX_OK;
}

int glrtx_group_present_get_stats(const glrtx_group *g, glrtx_present_stats *out) {
    if (!g || !out || g->ctx.empty()) return GLRTX_EINVAL;
    int copies = 0;
    for (size_t i = 0; i < g->ctx.size(); i++) {
        glrtx_present_stats t{};
        if (int rc = glrtx_present_get_stats(g->ctx[i], &t)) return rc;
        if (i == 0) *out = t;
        else out->pass_ms_last = std::max(out->pass_ms_last, t.pass_ms_last);  // (the members' passes run side by side)
        copies += t.copies_last;
    }
    out->copies_last = copies;
    return GLRTX_OK;
}

int glrtx_group_get_stats(const glrtx_group *g, glrtx_stats *out) {
    if (!g || !out || g->ctx.empty()) return GLRTX_EINVAL;
    glrtx_stats s{};
    for (size_t i = 0; i < g->ctx.size(); i++) {
        glrtx_stats t{};
        if (int rc = glrtx_get_stats(g->ctx[i], &t)) return rc;
        if (i == 0) s = t;
        else {
            s.rays += t.rays; s.rays_untraced += t.rays_untraced; s.paths += t.paths; s.owned_rows += t.owned_rows;
            s.fallback_launches += t.fallback_launches; s.fallback_last |= t.fallback_last;
            s.kernel_ms_total = std::max(s.kernel_ms_total, t.kernel_ms_total);  // the GPUs run side by side
            s.accumulate_ms_total = std::max(s.accumulate_ms_total, t.accumulate_ms_total);
            s.kernel_ms_last = std::max(s.kernel_ms_last, t.kernel_ms_last);
        }
    }
    *out = s;
    return GLRTX_OK;
}

}  // extern "C"
