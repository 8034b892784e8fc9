// tonemap.hip.h -- the display passes behind glrtx_exposure_measure / glrtx_tonemap / glrtx_resolve_tonemapped_rgba8 / glrtx_debug_tonemap (include/glrtx.h
// "Tone mapping"): a luminance histogram and its reduction to an exposure E, and a tone curve from an HDR float4 image to the plane T or straight to bytes.
//
// No reference counterpart (the reference's screen.frag is op 0 at exposure 1).  The arithmetic is the header's text: host/tonemap.cpp (glrt_exposure_measure,
// glrt_tonemap) and tests/tonemap_math.py state it again, and all three agree bit for bit -- every fp32 operation below is one correctly rounded operation in the
// order written (-ffp-contract=off; lp_exp and the resolve's rs_* carry the only fused ones), denormals flushed, min / max written as selects.  The histogram is
// integers: bins from the bit pattern, counts by integer atomics, so there is no order of summation to agree on.
//
// Passes, all on the context's stream:
//   exposure_histogram  a wave takes 64 * kHistPer consecutive pixels of a row (coalesced 16-byte loads, the resolve's shape) per trip of a grid-stride loop; the
//                       workgroup keeps 256 counters in LDS (ds_add_u32) and ends with one global vector atomic per nonzero bin into Exposure::work.  A wave whose
//                       counted lanes all fall into one bin (a flat image: 64 lanes on one LDS address) adds their number once, from one lane.
//   exposure_reduce     one workgroup of 256 threads, thread k = bin k: prefix sum, window, K and S (uint64), the double quotient, E; copies work -> hist and
//                       zeroes work for the next measurement.
//   tonemap_plane       source -> T {y, 1}, packed rows.
//   tonemap_resolve<PER>  source -> bytes: resolve_kernel's shape with the curve in front of rs_pixel on {y, 1}.  Every lane of a wave stays in (rs_pixel votes);
//                       lanes past the row's end carry (0, 0, 0, 1), which the curve maps to y = 0 under every op.
// The tone-map kernels read E from the Exposure block in device memory: measure-then-resolve needs no host round trip.
#pragma once
#include "denoise.hip.h"

namespace glrtx {
namespace tonemap {

// Device image of glrtx_exposure (include/glrtx.h) behind the working histogram the atomics go to.  measurements == 0: there is no E yet.
struct Exposure {
    uint32_t work[256];
    uint32_t hist[256];
    unsigned long long counted, kept;
    float mean_log2, target, exposure;
    int measurements;
};
constexpr size_t kExposureOut = 256 * sizeof(uint32_t);  // offset of the part glrtx_read_exposure returns

struct Curve {
    int op;            // 0 clamp, 1 Reinhard extended, 2 ACES fit
    int auto_exposure;
    float exposure, white;
};

DEV bool dead(float w) { return denoise::tiny(w) || w != w; }
// The scale s: exposure, or E * exposure with the context's measured E (1 while there is none)
DEV float scale_of(const Curve &c, const Exposure *st) {
    if (!c.auto_exposure) return c.exposure;
    const float E = st->measurements > 0 ? st->exposure : 1.0f;
    return E * c.exposure;
}
DEV float curve(float I, float s, int op, float ww) {
    float x = I * s;
    x = x > 0.0f ? x : 0.0f;  // (a NaN: 0)
    x = x < 65504.0f ? x : 65504.0f;
    if (op == 1) return (x * (1.0f + x / ww)) / (1.0f + x);
    if (op == 2) return (x * (2.51f * x + 0.03f)) / (x * (2.43f * x + 0.59f) + 0.14f);
    return x;
}
DEV float4 tone(float4 v, float s, int op, float ww) {
    if (dead(v.w)) return make_float4(0.f, 0.f, 0.f, 1.f);
    return make_float4(curve(v.x / v.w, s, op, ww), curve(v.y / v.w, s, op, ww), curve(v.z / v.w, s, op, ww), 1.0f);
}

// The bin of a pixel, -1 when it is not counted: dead, or a luminance that is NaN, +inf or <= 0.
DEV int bin_of(float4 v) {
    if (dead(v.w)) return -1;
    const float l = denoise::lum(v.x / v.w, v.y / v.w, v.z / v.w);
    if (!(l > 0.0f) || l == __builtin_inff()) return -1;
    const int k = (int)(__float_as_uint(l) >> 20) - 888;  // eight bins an octave from 2^-16
    return k < 0 ? 0 : (k > 255 ? 255 : k);
}

constexpr int kHistPer = 4;
__global__ __launch_bounds__(256) void exposure_histogram(const float4 *src, int pitch_f4, int width, int rows, Exposure *st) {
    constexpr int SEG = 64 * kHistPer;
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int segs = (width + SEG - 1) / SEG;
    const long long tasks = (long long)segs * rows;
    for (long long task = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); task < tasks; task += (long long)gridDim.x * 4) {  // (a whole wave per task)
        const int y = (int)(task / segs), x0 = (int)(task - (long long)y * segs) * SEG + lane;
        const float4 *row = src + (size_t)y * pitch_f4;
        float4 v[kHistPer];
#pragma unroll
        for (int j = 0; j < kHistPer; j++) {
            const int x = x0 + 64 * j;
            v[j] = x < width ? row[x] : make_float4(0.f, 0.f, 0.f, 0.f);  // (past the row's end: a dead pixel)
        }
#pragma unroll
        for (int j = 0; j < kHistPer; j++) {
            const int k = bin_of(v[j]);
            const unsigned long long counted = __ballot(k >= 0);
            if (counted == 0ull) continue;
            const int k0 = __shfl(k, __ffsll((long long)counted) - 1);
            if (__ballot(k == k0) == counted) {  // one bin for the whole wave: one add
                if (lane == 0) atomicAdd(&h[k0], (uint32_t)__popcll(counted));
            } else if (k >= 0) atomicAdd(&h[k], 1u);
        }
    }
    __syncthreads();
    const uint32_t n = h[threadIdx.x];
    if (n) atomicAdd(&st->work[threadIdx.x], n);
}

struct ReduceArgs {
    Exposure *st;
    float key, adapt;
    int low_permille, high_permille;
};
__global__ __launch_bounds__(256) void exposure_reduce(const ReduceArgs a) {
    __shared__ unsigned long long sc[256], sk[256], ss[256];
    const int k = threadIdx.x;
    Exposure *st = a.st;
    const uint32_t h = st->work[k];
    st->work[k] = 0u;
    st->hist[k] = h;
    sc[k] = h;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {  // inclusive prefix sum
        const unsigned long long add = k >= d ? sc[k - d] : 0ull;
        __syncthreads();
        sc[k] += add;
        __syncthreads();
    }
    const unsigned long long N = sc[255], c1 = sc[k], c0 = c1 - h;
    const unsigned long long lo = N * (unsigned long long)a.low_permille / 1000ull, hi = N * (unsigned long long)a.high_permille / 1000ull;
    const unsigned long long top = c1 < hi ? c1 : hi, bot = c0 > lo ? c0 : lo;
    const unsigned long long kept = top > bot ? top - bot : 0ull;
    sk[k] = kept;
    ss[k] = kept * (unsigned long long)(2 * k + 1);
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (k < d) { sk[k] += sk[k + d]; ss[k] += ss[k + d]; }
        __syncthreads();
    }
    if (k != 0) return;
    const unsigned long long K = sk[0], S = ss[0];
    const bool first = st->measurements <= 0;
    const float prev = st->exposure;
    float mean = 0.0f, target = first ? 1.0f : prev;
    if (K != 0ull) {
        mean = (float)((double)S / (double)(16ull * K) - 16.0);
        target = a.key * lp_exp((0.0f - mean) * 0x1.62e430p-1f);
    }
    st->counted = N; st->kept = K;
    st->mean_log2 = mean; st->target = target;
    st->exposure = first ? target : prev + (target - prev) * a.adapt;
    st->measurements = first ? 1 : st->measurements + 1;
}

__global__ __launch_bounds__(256) void tonemap_plane(const float4 *src, int pitch_f4, int width, int rows, float4 *dst, const Curve c, const Exposure *st) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63);
    const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= width || y >= rows) return;
    dst[(size_t)y * width + x] = tone(src[(size_t)y * pitch_f4 + x], scale_of(c, st), c.op, c.white * c.white);
}

template <int PER>
__global__ __launch_bounds__(256) void tonemap_resolve(const float4 *src, int pitch_f4, int width, int rows, uchar4 *out, int out_pitch_px, float inv_gamma, int flip,
                                                       const Curve c, const Exposure *st) {
    constexpr int SEG = 64 * PER;
    const int lane = threadIdx.x & 63;
    const int segs = (width + SEG - 1) / SEG;
    const int task = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int y = task / segs, x0 = (task - y * segs) * SEG + lane;
    if (y >= rows) return;  // (a whole wave)
    const float4 *row = src + (size_t)y * pitch_f4;
    float4 v[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int x = x0 + 64 * j;
        v[j] = x < width ? row[x] : make_float4(0.f, 0.f, 0.f, 1.f);
    }
    const float s = scale_of(c, st), ww = c.white * c.white;
    const int oy = flip ? rows - 1 - y : y;
    uchar4 *orow = out + (size_t)oy * out_pitch_px;
#pragma unroll
    for (int j = 0; j < PER; j++) {
        const int x = x0 + 64 * j;
        const uchar4 px = rs_pixel(tone(v[j], s, c.op, ww), inv_gamma);  // (every lane of the wave: rs_pixel votes)
        if (x < width) orow[x] = px;
    }
}

inline dim3 histogram_grid(int width, int rows) {
    const size_t tasks = (size_t)((width + 64 * kHistPer - 1) / (64 * kHistPer)) * (size_t)rows;
    return dim3((unsigned)std::min<size_t>((tasks + 3) / 4, 512));  // two workgroups a CU: at most 512 x 256 global atomics a measurement
}

}  // namespace tonemap
}  // namespace glrtx
