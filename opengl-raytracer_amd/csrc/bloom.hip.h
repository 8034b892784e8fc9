// bloom.hip.h -- the image pyramid behind glrtx_bloom / glrtx_debug_bloom (include/glrtx.h "Bloom"): a bright pass, a binomial down chain, a bilinear up chain
// that sums the levels, and the glow added to the linear HDR image in front of the tone curve.
//
// No reference counterpart.  The arithmetic is the header's text: host/bloom.cpp (glrt_bloom) and tests/bloom_math.py state it again, and all three agree bit
// for bit -- every fp32 operation below is one correctly rounded operation in the order written (-ffp-contract=off; nothing here is fused), denormals flushed,
// min / max written as selects.  Pyramid planes are float4 {rgb, 0}, packed rows.
//
// Passes, all on the context's stream; one glrtx_bloom is 2 * levels launches:
//   bloom_down<FIRST>   a 256-thread workgroup produces a 16 x 16 tile of level k + 1.  It stages the 35 x 35 footprint of level k in LDS -- clamped to the
//                       edge as it is loaded, 16-byte loads, each texel once per workgroup; with FIRST the texel is the source's and the bright pass runs on it, so
//                       D_0 is never stored -- with the even and the odd columns of a row apart (kDownOdd): the decimating horizontal pass then reads unit
//                       strides, and with a row pitch of 48 float4 (a multiple of 16) the lane groups of a 16-byte LDS read -- rows y and y + 1, eight columns each; the
//                       compiler reads 12 of the 16 bytes, w being a constant 0, and ds_read_b96's eight-lane groups fare the same -- fall on distinct banks.  The
//                       horizontal c5 goes to a second LDS plane of pitch 16, the vertical one reads that at a row stride of 2, which leaves the banks alone.
//   bloom_up<LAST>      a workgroup produces a 64 x 4 tile of level k (a wave: one row, 1 KiB of stores) from the 34 x 4 coarse texels around it, staged in LDS
//                       clamped to the edge.  Not LAST: D_k += up, in place (the update is pointwise on D_k).  LAST: reads the source again, recomputes x and
//                       stores B = {x + strength * glow, 1}.
#pragma once
#include "tonemap.hip.h"

namespace glrtx {
namespace bloom {

constexpr int kDownT = 16;              // the output tile's edge
constexpr int kDownIn = 2 * kDownT + 3; // the input footprint's edge: 35
constexpr int kDownPitch = 48;          // float4 per staged row: even columns at 0 .. 17, odd ones at kDownOdd .. kDownOdd + 16
constexpr int kDownOdd = 20;            // (4 mod 8: eight neighbouring lanes of the staging ds_write_b128 alternate between the halves without sharing a bank)
constexpr int kUpW = 64, kUpH = 4;      // the up pass's output tile
constexpr int kUpCw = kUpW / 2 + 2, kUpCh = kUpH / 2 + 2;

DEV int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// x: the pixel's value in front of the bright pass and of B
DEV float value_of(float s, float w) {
    const float I = s / w;
    const float x = I > 0.0f ? I : 0.0f;  // (a NaN: 0)
    return x < 65504.0f ? x : 65504.0f;
}
DEV float4 pixel_value(float4 v) {
    if (tonemap::dead(v.w)) return make_float4(0.f, 0.f, 0.f, 0.f);
    return make_float4(value_of(v.x, v.w), value_of(v.y, v.w), value_of(v.z, v.w), 0.f);
}
// D_0 = x * g
DEV float4 bright(float4 v, float threshold) {
    const float4 x = pixel_value(v);
    const float l = denoise::lum(x.x, x.y, x.z);
    float n = l - threshold;
    n = n > 0.0f ? n : 0.0f;
    const float m = l > 1.0e-4f ? l : 1.0e-4f;
    const float g = n / m;
    return make_float4(x.x * g, x.y * g, x.z * g, 0.f);
}
DEV float c5(float a, float b, float c, float d, float e) { return ((a + e) + 4.0f * (b + d)) + 6.0f * c; }
DEV float4 c5(float4 a, float4 b, float4 c, float4 d, float4 e) {
    return make_float4(c5(a.x, b.x, c.x, d.x, e.x), c5(a.y, b.y, c.y, d.y, e.y), c5(a.z, b.z, c.z, d.z, e.z), 0.f);
}
DEV float mix31(float near, float far) { return 0.75f * near + 0.25f * far; }
DEV float4 mix31(float4 n, float4 f) { return make_float4(mix31(n.x, f.x), mix31(n.y, f.y), mix31(n.z, f.z), 0.f); }

// Level k (w x h, rows of `pitch_f4`; with FIRST the source image) -> level k + 1 (wn x hn, packed).
template <bool FIRST>
__global__ __launch_bounds__(256) void bloom_down(const float4 *in, int pitch_f4, int w, int h, float4 *out, int wn, int hn, float threshold) {
    __shared__ float4 st[kDownIn * kDownPitch];
    __shared__ float4 hz[kDownIn * kDownT];
    const int X0 = blockIdx.x * kDownT, Y0 = blockIdx.y * kDownT;
    const int sx0 = 2 * X0 - 2, sy0 = 2 * Y0 - 2;
    for (int i = threadIdx.x; i < kDownIn * kDownIn; i += 256) {
        const int r = i / kDownIn, c = i - r * kDownIn;
        const int gx = clampi(sx0 + c, 0, w - 1), gy = clampi(sy0 + r, 0, h - 1);
        float4 v = in[(size_t)gy * pitch_f4 + gx];
        if (FIRST) v = bright(v, threshold);
        st[r * kDownPitch + ((c & 1) ? kDownOdd : 0) + (c >> 1)] = v;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kDownIn * kDownT; i += 256) {  // staged column 2x + 2 + i is X(i) of output x
        const float4 *e = st + (i >> 4) * kDownPitch + (i & (kDownT - 1)), *o = e + kDownOdd;
        hz[i] = c5(e[0], o[0], e[1], o[1], e[2]);
    }
    __syncthreads();
    const int lx = threadIdx.x & (kDownT - 1), ly = threadIdx.x >> 4;
    const float4 *p = hz + (2 * ly) * kDownT + lx;
    const float4 s = c5(p[0], p[kDownT], p[2 * kDownT], p[3 * kDownT], p[4 * kDownT]);
    const int x = X0 + lx, y = Y0 + ly;
    if (x < wn && y < hn) out[(size_t)y * wn + x] = make_float4(s.x * 0x1p-8f, s.y * 0x1p-8f, s.z * 0x1p-8f, 0.f);
}

// up(coarse, w, h) added to the plane `fine` in place (w x h, packed), or with LAST: B = {x(src) + strength * (up * inv_levels), 1}.
template <bool LAST>
__global__ __launch_bounds__(256) void bloom_up(const float4 *coarse, int wc, int hc, float4 *fine, int w, int h, const float4 *src, int src_pitch_f4, float4 *B,
                                                float strength, float inv_levels) {
    __shared__ float4 st[kUpCh * kUpCw];
    const int lx = threadIdx.x & (kUpW - 1), ly = threadIdx.x >> 6;
    const int x = blockIdx.x * kUpW + lx, y = blockIdx.y * kUpH + ly;
    const bool inside = x < w && y < h;
    float4 mine = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) mine = LAST ? src[(size_t)y * src_pitch_f4 + x] : fine[(size_t)y * w + x];
    if (threadIdx.x < kUpCh * kUpCw) {
        const int r = threadIdx.x / kUpCw, c = threadIdx.x - r * kUpCw;
        const int gx = clampi(blockIdx.x * (kUpW / 2) - 1 + c, 0, wc - 1), gy = clampi(blockIdx.y * (kUpH / 2) - 1 + r, 0, hc - 1);
        st[threadIdx.x] = coarse[(size_t)gy * wc + gx];
    }
    __syncthreads();
    const int nx = (lx >> 1) + 1, fx = (lx & 1) ? nx + 1 : nx - 1;
    const int ny = (ly >> 1) + 1, fy = (ly & 1) ? ny + 1 : ny - 1;
    const float4 hn = mix31(st[ny * kUpCw + nx], st[ny * kUpCw + fx]);
    const float4 hf = mix31(st[fy * kUpCw + nx], st[fy * kUpCw + fx]);
    const float4 u = mix31(hn, hf);
    if (!inside) return;
    if (LAST) {
        const float4 xv = pixel_value(mine);
        B[(size_t)y * w + x] = make_float4(xv.x + strength * (u.x * inv_levels), xv.y + strength * (u.y * inv_levels), xv.z + strength * (u.z * inv_levels), 1.0f);
    } else
        fine[(size_t)y * w + x] = make_float4(mine.x + u.x, mine.y + u.y, mine.z + u.z, 0.f);
}

inline dim3 down_grid(int wn, int hn) { return dim3((unsigned)((wn + kDownT - 1) / kDownT), (unsigned)((hn + kDownT - 1) / kDownT)); }
inline dim3 up_grid(int w, int h) { return dim3((unsigned)((w + kUpW - 1) / kUpW), (unsigned)((h + kUpH - 1) / kUpH)); }

}  // namespace bloom
}  // namespace glrtx
