// reproject.hip.h -- temporal reprojection (glrtx_reproject / glrtx_debug_reproject, include/glrtx.h "Reprojection"): carries the accumulator's mean and count
// from the previous camera's view into the new one, per pixel, where the old view saw the same surface (the reprojection step of SVGF, Schied et al. 2017).
//
// No reference counterpart (the reference clears on every camera move).  The arithmetic is the header's text: host/reproject.cpp (glrt_reproject) and
// tests/reproject_math.py state it again, and all three agree bit for bit -- every fp32 operation below is one correctly rounded operation in the order
// written (-ffp-contract=off), denormals flushed, a NaN that is stored is 0x7FC00000.  The new view's ray is features::centre_ray's, the function the feature
// pass made the new planes with.
//
// One pass on the context's stream.  A wave is one 8x8 tile (lane k at (k & 7, k >> 3), the wavefront kernel's and the denoiser's order), a workgroup four
// consecutive tiles.  Per pixel: the new planes N1 / A1 are read once with non-temporal 16-byte loads (they bypass L1, which the taps then have to
// themselves); the four taps are plain 16-byte loads from the old accumulator and the old planes -- under a smooth camera move the 64 footprints of a wave
// fall into about nine rows of 128 to 160 contiguous bytes per buffer, and neighbouring pixels share three of their four taps, so most taps are L1 / L2 hits; the result is
// one plain 16-byte store (the next frame's accumulation pass reads it from L2).  The two counters take one ballot each and ONE 64-bit vector atomic per wave,
// spread over kCountSlots words.
//
// reproject_motion_kernel (reproject_motion.hip.h) differs in where the world point and the normal to test come from, and in nothing else: the arguments both
// read (Common), the pixel of a lane (pixel_of), the lookup in the old view (history_lookup), the store (store_pixel) and the counters (count_wave) are stated here,
// once.  canon and tiny are denoise.hip.h's.
#pragma once
#include "denoise.hip.h"
#include "features.hip.h"

namespace glrtx {
namespace reproject {

constexpr float kMinWeight = 1.0e-6f;  // a pixel whose taps weigh less than this in sum has no history
// The counters: kCountSlots 64-bit words, one per 64-byte line, a workgroup adding to slot blockIdx.x % kCountSlots; the host sums them.  (32,400 waves at
// 1080p adding to ONE word queue up behind each other at that word's memory channel: the kernel then takes the time of its atomics, not of its pixels.)
constexpr int kCountSlots = 64, kCountStride = 8;
constexpr size_t kCountBytes = (size_t)kCountSlots * kCountStride * sizeof(unsigned long long);

// What reproject_kernel and reproject_motion_kernel (reproject_motion.hip.h) share: the old view and its camera, the new view's two planes, the output, the
// counters.  The launch code fills it once for both (glrtx.hip: reproject_common).
struct Common {
    float W[16], S[16];       // inverse(c2w_prev), inverse(s2c_prev)
    float opx, opy, opz;      // the previous camera's origin (centre_ray's, formed on the host)
    const float4 *acc;        // the old view: accumulator (pitch_f4 per row) and planes (packed rows of width)
    const float4 *n0, *a0;
    const float4 *x1, *a1;    // the new view's planes: x1 is N1 {n, t} for reproject_kernel, G1 {wire triangle, u, v} for reproject_motion_kernel; A1 {albedo, id}
    float4 *out;              // pitch_f4 per row
    int pitch_f4, width, rows, tiles_x, n_tiles;
    float max_history, depth_tol, normal_tol;  // (max_history as a float; the tolerances with denormals flushed)
    unsigned long long *counts;  // kCountSlots words kCountStride apart: carried in the low half, hit pixels in the high half
    const float4 *mom;        // the old view's moments plane M (pitch_f4 per row), or null: no moments are carried
    float4 *mom_out;          // the new view's (pitch_f4 per row)
};

struct Args {
    features::Args cam;       // the new view: cam[32], width, height, rank 0 of world 1 (only what features::centre_ray reads is set)
    Common c;                 // (x1: N1)
};

using denoise::canon;
using denoise::tiny;
DEV bool pos_finite(float x) { return (__float_as_uint(x) - 0x00800000u) < 0x7F000000u; }  // sign clear, exponent neither 0 nor 255

// The moments plane through the same taps (include/glrtx.h "Variance guidance": "Carrying M"), shared with reproject_motion_kernel as centre_ray is shared with the
// feature pass.  A tap that counts for the accumulator counts for M if M.w is neither a zero nor a denormal.
struct MomSum { float sm, smc, s1, s2; };
DEV void moments_tap(MomSum &s, float w, float4 M) {
    if (tiny(M.w)) return;
    s.sm = s.sm + w;
    s.smc = s.smc + w * M.w;
    s.s1 = s.s1 + w * (M.x / M.w);
    s.s2 = s.s2 + w * (M.y / M.w);
}
DEV float4 moments_out(const MomSum &s, float max_history) {
    if (!(s.sm > kMinWeight)) return make_float4(0.f, 0.f, 0.f, 0.f);
    const float r = __builtin_rintf(s.smc / s.sm);
    const float nm = r > max_history ? max_history : r;
    if (!(nm >= 1.0f)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(canon((s.s1 / s.sm) * nm), canon((s.s2 / s.sm) * nm), 0.f, nm);
}

// A wave's 8x8 tile and a lane's pixel in it; `in`: the tile exists and the pixel is inside the image.
struct Pixel { int x, y; bool in; };
DEV Pixel pixel_of(const Common &a) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), k = threadIdx.x & 63;
    const int x = (tile % a.tiles_x) * 8 + (k & 7), y = (tile / a.tiles_x) * 8 + (k >> 3);
    return {x, y, tile < a.n_tiles && x < a.width && y < a.rows};
}

// The history of the world point P in the old view: P through W and S to the old image, the four taps around it that show material `id` with a count, a
// normal within normal_tol of (nx, ny, nz) and a depth within depth_tol of P's distance to the old camera; their weighted mean times the rounded, capped
// count.  o4 / m4 / carried are written only where there is a history (the callers start them at zero / false).
DEV void history_lookup(const Common &a, float Px, float Py, float Pz, float nx, float ny, float nz, int id, float4 &o4, float4 &m4, bool &carried) {
    const float *W = a.W, *S = a.S;
    const float qx = ((W[0] * Px + W[4] * Py) + W[8] * Pz) + W[12];
    const float qy = ((W[1] * Px + W[5] * Py) + W[9] * Pz) + W[13];
    const float qz = ((W[2] * Px + W[6] * Py) + W[10] * Pz) + W[14];
    const float qw = ((W[3] * Px + W[7] * Py) + W[11] * Pz) + W[15];
    const float sx = ((S[0] * qx + S[4] * qy) + S[8] * qz) + S[12] * qw;
    const float sy = ((S[1] * qx + S[5] * qy) + S[9] * qz) + S[13] * qw;
    const float sw4 = ((S[3] * qx + S[7] * qy) + S[11] * qz) + S[15] * qw;
    const float Wf = (float)a.width, Hf = (float)a.rows;
    const float u = ((sx / sw4 + 1.0f) * 0.5f) * Wf + -1.0f;
    const float v = ((sy / sw4 + 1.0f) * 0.5f) * Hf + -1.0f;
    // (outside [-1, size) no tap lies inside the image; a NaN fails the comparisons)
    if (!(pos_finite(sw4) && u >= -1.0f && u < Wf && v >= -1.0f && v < Hf)) return;
    const float ex = Px - a.opx, ey = Py - a.opy, ez = Pz - a.opz;
    const float e = __builtin_sqrtf((ez * ez + ey * ey) + ex * ex);
    const float lim = a.depth_tol * e;
    const float fx0 = __builtin_floorf(u), fy0 = __builtin_floorf(v);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const float fx = u - fx0, fy = v - fy0;
    const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
    float sw = 0.f, sc = 0.f, sr = 0.f, sg = 0.f, sb = 0.f;
    MomSum ms = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; j++) {
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int tx = x0 + i, ty = y0 + j;
            if (tx < 0 || tx >= a.width || ty < 0 || ty >= a.rows) continue;
            const size_t q = (size_t)ty * a.width + tx;
            const float4 A0 = a.a0[q];
            if (__float_as_int(A0.w) != id) continue;
            const float4 C = a.acc[(size_t)ty * a.pitch_f4 + tx];
            const float4 N0 = a.n0[q];
            if (tiny(C.w)) continue;
            if (!(dot3(nx, ny, nz, N0.x, N0.y, N0.z) >= a.normal_tol)) continue;
            if (!(__builtin_fabsf(N0.w - e) <= lim)) continue;
            const float w = wx[i] * wy[j];
            sw = sw + w;
            sc = sc + w * C.w;
            sr = sr + w * (C.x / C.w); sg = sg + w * (C.y / C.w); sb = sb + w * (C.z / C.w);
            if (a.mom) moments_tap(ms, w, a.mom[(size_t)ty * a.pitch_f4 + tx]);
        }
    }
    if (!(sw > kMinWeight)) return;
    const float r = __builtin_rintf(sc / sw);
    const float n = r > a.max_history ? a.max_history : r;
    if (!(n >= 1.0f)) return;
    o4 = make_float4(canon((sr / sw) * n), canon((sg / sw) * n), canon((sb / sw) * n), n);
    carried = true;
    if (a.mom) m4 = moments_out(ms, a.max_history);
}

// The end of both kernels: the pixel's store(s), inside the kernel's own test of `in`; then, for every lane, one ballot per counter and ONE atomic per wave.
DEV void store_pixel(const Common &a, const Pixel &px, float4 o4, float4 m4) {
    a.out[(size_t)px.y * a.pitch_f4 + px.x] = o4;
    if (a.mom_out) a.mom_out[(size_t)px.y * a.pitch_f4 + px.x] = m4;
}
DEV void count_wave(const Common &a, bool carried, bool hit) {
    const unsigned long long nc = __popcll(__ballot(carried)), nh = __popcll(__ballot(hit));
    if ((threadIdx.x & 63) == 0 && (nc | nh) != 0ull) atomicAdd(a.counts + (size_t)(blockIdx.x % kCountSlots) * kCountStride, nc | (nh << 32));
}

__global__ __launch_bounds__(256) void reproject_kernel(const Args a) {
    const Pixel px = pixel_of(a.c);
    bool hit = false, carried = false;
    float4 o4 = make_float4(0.f, 0.f, 0.f, 0.f), m4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (px.in) {
        const size_t p = (size_t)px.y * a.c.width + px.x;
        const float4 N1 = ld_stream(a.c.x1 + p), A1 = ld_stream(a.c.a1 + p);
        const int id = __float_as_int(A1.w);
        hit = id >= 0;  // (the reserved id INT32_MIN is negative)
        const float t = N1.w;
        if (hit && pos_finite(t)) {
            float4 o, d;
            (void)features::centre_ray(a.cam, px.x, px.y, o, d);
            history_lookup(a.c, o.x + t * d.x, o.y + t * d.y, o.z + t * d.z, N1.x, N1.y, N1.z, id, o4, m4, carried);
        }
        store_pixel(a.c, px, o4, m4);
    }
    count_wave(a.c, carried, hit);
}

}  // namespace reproject
}  // namespace glrtx
