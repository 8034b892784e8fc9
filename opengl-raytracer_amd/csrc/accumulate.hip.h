// accumulate.hip.h -- the accumulation pass behind a render launch that wrote sample planes (glrtx.hip: wgwf_issue), stated ONCE.
//
// Per pixel the pass is one chain of float additions -- acc.xyz += v.xyz; acc.w += 1 -- over the launch's planes, frame by frame, sample by sample: the chain that
// consecutive single-frame launches perform inside the render kernel.  Every bit-exactness guarantee of the library rests on that chain, so it is written in one
// template (pass) and the eight kernels are entry points over it.  They differ in two things only:
//   the SOURCE  Planes -- one flat array [frame][sample][rows][pitch_f4] (plain and overlapped launches);
//               Fed -- a fed launch's chunks of kFeedChunkFrames frames behind FeedDev, however many frames the launch ended up taking (FeedDev::frames_known, final
//               once the render kernel has ended);
//   the SINK    None;
//               Half (glrtx_render_adaptive) -- ACTIVE tiles only: an inactive tile's planes were not written, its accumulator and H entries are not touched; a sample
//               also goes into the half buffer H when the pixel's count BEFORE the add is odd: H holds every second sample (tests/adaptive_math.py);
//               Moments (glrtx_render_moments) -- the sample's luminance and its square go into the moments plane M {sum l, sum l^2, 0, count} (tests/variance_math.py);
//               MomentsMasked (glrtx_render_adaptive_moments) -- Moments on ACTIVE tiles only: an inactive tile's accumulator and M entries are not touched;
//               Cascades (glrtx_render_cascades) -- the sample is split by luminance over the six cascade planes C_0 .. C_5 {sum w rgb, count} (reweight.hip.h: fold;
//               tests/reweight_math.py); the six float4 are loaded before the sample loop and stored after it;
//               Present (glrtx_present_enable) -- behind every frame f the pixel's screen.frag value (rs_pixel, byte-identical to resolve_kernel's) goes into image
//               (slot0 + f) % n_ring of the device ring, packed rows of `width` texels, row y at rows - 1 - y when flipped (within the owned rows, like
//               glrtx_resolve_rgba8): one launch and one read of the accumulator instead of a pass plus a resolve per frame.
// Bandwidth-bound: 16 B per plane and pixel in, one 16-B read-modify-write of the accumulator (Half, Moments, MomentsMasked: two; Cascades: seven), 4 B per frame and
// pixel out (Present).
#pragma once
#include <type_traits>

#include "denoise.hip.h"  // (pt_kernel.hip.h: FeedDev, rs_pixel; lum)
#include "reweight.hip.h"

namespace glrtx {
namespace accumulate {

struct Image { float4 *accum; int pitch_f4, width, rows; };  // the accumulator: the owned rows
struct Planes {
    const float4 *planes;
    int n_frames, n_samples;
    static constexpr bool kContiguous = true;  // frame f + 1's planes follow frame f's
    DEV int frames() const { return n_frames; }
    DEV const float4 *frame(int f, size_t plane) const { return planes + (size_t)f * (size_t)n_samples * plane; }
};
struct Fed {
    const FeedDev *fd;
    int n_samples;
    static constexpr bool kContiguous = false;
    DEV int frames() const { return (int)(fd->frames_known & ~kFeedClosed); }
    DEV const float4 *frame(int f, size_t plane) const { return reinterpret_cast<const float4 *>(fd->chunks[f / kFeedChunkFrames]) + (size_t)(f % kFeedChunkFrames) * (size_t)n_samples * plane; }
};

struct None {};
struct Half { float4 *half; const unsigned char *mask; int tiles8_x; };  // H and the selection's mask byte per 8x8 tile
struct Moments { float4 *moments; };                                     // M, of the accumulator's pitch
struct MomentsMasked { float4 *moments; const unsigned char *mask; int tiles8_x; };  // M and the selection's mask byte per 8x8 tile
struct Cascades { float4 *c; size_t plane; float start; };                           // C_0 .. C_5, `plane` float4 apart, of the accumulator's pitch
struct Present { uchar4 *ring; size_t slot_px; int n_ring, slot0; float inv_gamma; int flip; };

// One lane per pixel, a wave is 64 consecutive pixels of a row, four rows per workgroup: a grid of (width + 63) / 64 x (rows + 3) / 4.
// Two lane disciplines.  Present keeps the lanes past the row's end in the wave, with the texel (0, 0, 0, 1), because rs_pixel votes across the wave; they load and
// store nothing.  Every other sink has nothing to vote on and returns early.
// Per sample, the sink's own update comes BEFORE the accumulator's add (Half decides by the count's parity before the add).
// A flat source's frames are contiguous, so a sink without a per-frame step takes them as one run of n_frames * n_samples planes: one loop for the compiler to unroll.
template <class Src, class Sink>
DEV void pass(const Image im, const Src src, const Sink sink) {
    constexpr bool kHalf = std::is_same_v<Sink, Half>, kMasked = std::is_same_v<Sink, MomentsMasked>, kMoments = std::is_same_v<Sink, Moments> || kMasked,
                   kPresent = std::is_same_v<Sink, Present>, kCascades = std::is_same_v<Sink, Cascades>;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (y >= im.rows) return;  // (a whole wave)
    if (!kPresent && x >= im.width) return;
    const bool in = kPresent ? x < im.width : true;
    if constexpr (kHalf || kMasked)
        if (sink.mask[(y >> 3) * sink.tiles8_x + (x >> 3)] == 0) return;
    const size_t at = (size_t)y * im.pitch_f4 + x, plane = (size_t)im.rows * im.pitch_f4;
    int runs = src.frames(), len = src.n_samples;
    if constexpr (Src::kContiguous && !kPresent) { len *= runs; runs = 1; }
    float4 acc = in ? im.accum[at] : make_float4(0.f, 0.f, 0.f, 1.f);
    float4 side = make_float4(0.f, 0.f, 0.f, 0.f);  // H or M
    if constexpr (kHalf) side = sink.half[at];
    if constexpr (kMoments) side = sink.moments[at];
    [[maybe_unused]] float4 cas[kCascades ? reweight::kCascades : 1];
    [[maybe_unused]] reweight::Bounds bounds;
    if constexpr (kCascades) {
        bounds = reweight::bounds_of(sink.start);
#pragma unroll
        for (int k = 0; k < reweight::kCascades; k++) cas[k] = sink.c[(size_t)k * sink.plane + at];
    }
    for (int f = 0; f < runs; f++) {
        if (in) {
            const float4 *p = src.frame(f, plane) + at;
            for (int k = 0; k < len; k++) {
                const float4 v = p[(size_t)k * plane];
                if constexpr (kHalf)
                    if (((unsigned)acc.w & 1u) != 0u) {
                        side.x = side.x + v.x; side.y = side.y + v.y; side.z = side.z + v.z;
                        side.w = side.w + 1.0f;
                    }
                if constexpr (kMoments) {
                    const float l = denoise::lum(v.x, v.y, v.z);
                    side.x = side.x + l; side.y = side.y + l * l; side.w = side.w + 1.0f;
                }
                if constexpr (kCascades) reweight::fold(cas, bounds, v);
                acc.x = acc.x + v.x; acc.y = acc.y + v.y; acc.z = acc.z + v.z;
                acc.w = acc.w + 1.0f;
            }
        }
        if constexpr (kPresent) {
            const uchar4 px = rs_pixel(acc, sink.inv_gamma);  // (every lane of the wave)
            const int oy = sink.flip ? im.rows - 1 - y : y;
            if (in) sink.ring[(size_t)((sink.slot0 + f) % sink.n_ring) * sink.slot_px + (size_t)oy * im.width + x] = px;
        }
    }
    if (in) im.accum[at] = acc;
    if constexpr (kHalf) sink.half[at] = side;
    if constexpr (kMoments) sink.moments[at] = side;
    if constexpr (kCascades) {
#pragma unroll
        for (int k = 0; k < reweight::kCascades; k++) sink.c[(size_t)k * sink.plane + at] = cas[k];
    }
}

}  // namespace accumulate

// ---- the entry points: one per (source, sink) pair that a launch can ask for
__global__ __launch_bounds__(256) void accumulate_planes_kernel(const accumulate::Image im, const accumulate::Planes src, const accumulate::None sink) { accumulate::pass(im, src, sink); }
__global__ __launch_bounds__(256) void accumulate_feed_kernel(const accumulate::Image im, const accumulate::Fed src, const accumulate::None sink) { accumulate::pass(im, src, sink); }
__global__ __launch_bounds__(256) void accumulate_adaptive_kernel(const accumulate::Image im, const accumulate::Planes src, const accumulate::Half sink) { accumulate::pass(im, src, sink); }
__global__ __launch_bounds__(256) void accumulate_present_planes_kernel(const accumulate::Image im, const accumulate::Planes src, const accumulate::Present sink) { accumulate::pass(im, src, sink); }
__global__ __launch_bounds__(256) void accumulate_present_feed_kernel(const accumulate::Image im, const accumulate::Fed src, const accumulate::Present sink) { accumulate::pass(im, src, sink); }
namespace variance { __global__ __launch_bounds__(256) void accumulate_moments_kernel(const accumulate::Image im, const accumulate::Planes src, const accumulate::Moments sink) { accumulate::pass(im, src, sink); } }
namespace adaptive_moments { __global__ __launch_bounds__(256) void accumulate_kernel(const accumulate::Image im, const accumulate::Planes src, const accumulate::MomentsMasked sink) { accumulate::pass(im, src, sink); } }
namespace reweight { __global__ __launch_bounds__(256) void accumulate_cascades_kernel(const accumulate::Image im, const accumulate::Planes src, const accumulate::Cascades sink) { accumulate::pass(im, src, sink); } }

namespace accumulate {
inline auto entry(Planes, None) { return accumulate_planes_kernel; }
inline auto entry(Fed, None) { return accumulate_feed_kernel; }
inline auto entry(Planes, Half) { return accumulate_adaptive_kernel; }
inline auto entry(Planes, Moments) { return variance::accumulate_moments_kernel; }
inline auto entry(Planes, MomentsMasked) { return adaptive_moments::accumulate_kernel; }
inline auto entry(Planes, Cascades) { return reweight::accumulate_cascades_kernel; }
inline auto entry(Planes, Present) { return accumulate_present_planes_kernel; }
inline auto entry(Fed, Present) { return accumulate_present_feed_kernel; }
}  // namespace accumulate

// In front of a fed launch's render kernel, on its stream: the frames the launch starts with go into the device mirror by ONE wave (left to the render kernel, every
// workgroup would fetch them across PCIe in its first top-up: a thousand times the same reads).
__global__ __launch_bounds__(64) void feed_prefill_kernel(FeedDev *fd, const FeedHost *fh, int n_frames) {
    const int lane = threadIdx.x;
    for (int f = lane; f < n_frames; f += 64) fd->seeds[f] = (unsigned long long)__float_as_uint(fh->seeds[f].x) | ((unsigned long long)__float_as_uint(fh->seeds[f].y) << 32);
    for (int c = lane; c <= (n_frames - 1) / kFeedChunkFrames; c += 64) fd->chunks[c] = (unsigned long long)fh->chunks[c];
    if (lane == 0) fd->frames_known = (unsigned)n_frames;
}

}  // namespace glrtx
