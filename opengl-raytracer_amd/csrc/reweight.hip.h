// reweight.hip.h -- firefly re-weighting by luminance cascades (glrtx_track_cascades, glrtx_render_cascades, glrtx_reweight, include/glrtx.h "Firefly
// re-weighting"; Zirr, Hanika and Dachsbacher, "Re-weighting Firefly Samples for Improved Finite-Sample Monte Carlo Estimates", CGF 37(6), 2018).
//
// No reference counterpart.  The arithmetic is the header's text: host/reweight.cpp and tests/reweight_math.py state it again, and all three agree bit for bit under
// denoise.hip.h's rules (one correctly rounded fp32 operation at a time in the order written, -ffp-contract=off; denormals flushed; a stored NaN is 0x7FC00000).
//
//   fold  one sample into the six cascade planes C_0 .. C_5 {sum w r, sum w g, sum w b, count}, held in registers by the accumulation pass (accumulate.hip.h: the
//       Cascades sink; accumulate_cascades_kernel is in this namespace).  The planes are addressed with compile-time indices only -- `if (k == j)` inside unrolled
//       loops -- because a register array indexed at run time goes to scratch.
//   reweight_kernel  the resolve, in the filters' shape: a workgroup owns a 16x16 tile, a wave an 8x8 sub-tile in tile order.  T_0 .. T_4 ("samples at level k or
//       brighter") of tile + a one-pixel halo are staged in LDS (18^2 x 5 floats, 6.3 KiB): a tile pixel from the six float4 it needs anyway, one of the 68 halo
//       pixels from the six count words alone.  A tap outside the image is staged as +0: the sums start at +0, so adding it equals skipping it.  No atomics.
//       Per pixel 6 x 16 B in, 16 B out: 112 B compulsory; the halo adds 68 / 256 x 24 B.
#pragma once
#include "denoise.hip.h"

namespace glrtx {
namespace reweight {

constexpr int kCascades = 6;

// The bounds b_k = start * 8^k (exact scalings: start is within 2^-20 .. 2^20).
struct Bounds { float b[kCascades]; };
DEV Bounds bounds_of(float start) {
    Bounds B;
    float s = start;
#pragma unroll
    for (int k = 0; k < kCascades; k++) { B.b[k] = s; s = s * 8.0f; }
    return B;
}

// One sample into the cascades (the header's "Fold").  Every index of c is a compile-time constant after unrolling.
DEV void fold(float4 (&c)[kCascades], const Bounds &B, const float4 v) {
    const float l = denoise::lum(v.x, v.y, v.z);
    int j = 0;
#pragma unroll
    for (int k = 1; k <= 4; k++)
        if (l >= B.b[k]) j = k;
    float lower = B.b[0], upper = B.b[1];
#pragma unroll
    for (int k = 1; k <= 4; k++)
        if (k == j) { lower = B.b[k]; upper = B.b[k + 1]; }
    float wl, wu;
    int jc = j;
    if (!(l > lower)) { wl = 1.0f; wu = 0.0f; }
    else if (l >= upper) { wl = 0.0f; wu = 1.0f; jc = 5; }
    else {
        const float q = lower / l;
        wl = (q - 0.125f) / 0.875f;
        wl = wl > 0.0f ? wl : 0.0f;
        wl = wl < 1.0f ? wl : 1.0f;
        wu = 1.0f - wl;
    }
    const float lx = wl * v.x, ly = wl * v.y, lz = wl * v.z;
    const float ux = wu * v.x, uy = wu * v.y, uz = wu * v.z;
#pragma unroll
    for (int k = 0; k < kCascades; k++) {
        if (k == j) { c[k].x = c[k].x + lx; c[k].y = c[k].y + ly; c[k].z = c[k].z + lz; }
        if (k == j + 1) { c[k].x = c[k].x + ux; c[k].y = c[k].y + uy; c[k].z = c[k].z + uz; }
        if (k == jc) c[k].w = c[k].w + 1.0f;
    }
}

struct Args {
    const float4 *c;   // six planes of `plane` float4 each, pitch_f4 per row
    size_t plane;
    float4 *out;       // D: packed rows of `width`
    int pitch_f4, width, rows;
    float kappa;
};

constexpr int kSideRw = denoise::kTileDn + 2, kRingRw = kSideRw * kSideRw - denoise::kTileDn * denoise::kTileDn;  // 18, 68

// T_0 .. T_4 from the six count words: T_5 = w_5; T_k = T_{k+1} + w_k.
DEV void counts_above(const float (&w)[kCascades], float (&T)[kCascades - 1]) {
    float t = w[5];
#pragma unroll
    for (int k = 4; k >= 0; k--) { t = t + w[k]; T[k] = t; }
}

inline dim3 reweight_grid(int width, int rows) {
    return dim3((unsigned)(((width + denoise::kTileDn - 1) / denoise::kTileDn) * ((rows + denoise::kTileDn - 1) / denoise::kTileDn)));
}

__global__ __launch_bounds__(256) void reweight_kernel(const Args a) {
    __shared__ float sT[kCascades - 1][kSideRw * kSideRw];
    const denoise::Tile16 t = denoise::tile16(a.width);
    const int x = t.x0 + t.tx, y = t.y0 + t.ty;
    const bool inside = x < a.width && y < a.rows;
    const int ci = (t.ty + 1) * kSideRw + t.tx + 1;
    float4 c[kCascades];
    float T[kCascades - 1] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (inside) {
        const size_t at = (size_t)y * a.pitch_f4 + x;
        float w[kCascades];
#pragma unroll
        for (int k = 0; k < kCascades; k++) { c[k] = a.c[(size_t)k * a.plane + at]; w[k] = c[k].w; }
        counts_above(w, T);
    }
#pragma unroll
    for (int k = 0; k < kCascades - 1; k++) sT[k][ci] = T[k];
    if (threadIdx.x < kRingRw) {  // the halo ring: top row, bottom row, left column, right column
        const int i = threadIdx.x;
        int sx, sy;
        if (i < kSideRw) { sx = i; sy = 0; }
        else if (i < 2 * kSideRw) { sx = i - kSideRw; sy = kSideRw - 1; }
        else if (i < 2 * kSideRw + denoise::kTileDn) { sx = 0; sy = i - 2 * kSideRw + 1; }
        else { sx = kSideRw - 1; sy = i - 2 * kSideRw - denoise::kTileDn + 1; }
        const int gx = t.x0 - 1 + sx, gy = t.y0 - 1 + sy;
        float Th[kCascades - 1] = {0.f, 0.f, 0.f, 0.f, 0.f};
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.rows) {
            const size_t q = (size_t)gy * a.pitch_f4 + gx;
            float w[kCascades];
#pragma unroll
            for (int k = 0; k < kCascades; k++) w[k] = a.c[(size_t)k * a.plane + q].w;
            counts_above(w, Th);
        }
#pragma unroll
        for (int k = 0; k < kCascades - 1; k++) sT[k][sy * kSideRw + sx] = Th[k];
    }
    __syncthreads();
    if (!inside) return;
    const float n = T[0];
    float4 o = make_float4(0.f, 0.f, 0.f, 1.f);
    if (!denoise::tiny(n) && n == n) {
        float ax = c[0].x, ay = c[0].y, az = c[0].z;
#pragma unroll
        for (int j = 1; j < kCascades; j++) {
            float s = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++)
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) s = s + sT[j - 1][ci + dy * kSideRw + dx];
            s = s - 1.0f;
            s = s > 0.0f ? s : 0.0f;
            float r = s / a.kappa;
            r = r < 1.0f ? r : 1.0f;
            ax = ax + r * c[j].x; ay = ay + r * c[j].y; az = az + r * c[j].z;
        }
        o.x = denoise::canon(ax / n); o.y = denoise::canon(ay / n); o.z = denoise::canon(az / n);
    }
    a.out[(size_t)y * a.width + x] = o;
}

}  // namespace reweight
}  // namespace glrtx
