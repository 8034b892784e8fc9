// variance.hip.h -- the moments fold and the variance pass of the variance-guided denoiser (glrtx_render_moments, glrtx_denoise_variance, include/glrtx.h
// "Variance guidance"; the variance estimation step of SVGF, Schied et al. 2017).  The filter itself is denoise.hip.h's atrous<S, LAST, true>, and the tile
// arithmetic, the normal/depth term, lum, canon and tiny used below are that file's own.
//
// No reference counterpart.  The arithmetic is the header's text: host/variance.cpp and tests/variance_math.py state it again, and all three agree bit for bit
// under denoise.hip.h's rules (one correctly rounded fp32 operation at a time in the order written, -ffp-contract=off; denormals flushed; a stored NaN is 0x7FC00000).
//
//   accumulate_moments_kernel  lives in accumulate.hip.h (the one accumulation pass, its Moments sink; still in this namespace): every sample plane is added to the
//       accumulator (the same chain of additions, so the accumulator is glrtx_render_frames') and its luminance and squared luminance to the moments plane M.
//   variance_estimate  the filter's shape: a workgroup owns a 16x16 tile, a wave an 8x8 sub-tile in tile order; tile + a 3-pixel halo (22^2 pixels) is staged in
//       LDS as two float4 per pixel -- {mu1, mu2, id, M.w} and the feature plane's {n, t}, 15.1 KiB -- from four 16-byte loads per pixel (accumulator, M, A, N).
//       A dead or outside pixel is staged with the reserved id, so one compare per tap applies all three exclusions.  A pixel with M.w >= 4 needs no tap at all.
//   adaptive_moments::select_kernel  the selection of glrtx_render_adaptive_moments (include/glrtx.h "Adaptive sampling by variance"): adaptive_select_kernel's layout
//       -- one wave per 8x8 tile, four tiles per workgroup, the same tree sum -- over M alone: one streaming 16-byte load per pixel where the H form takes two.
#pragma once
#include "denoise.hip.h"

namespace glrtx {
namespace variance {

using denoise::albedo_of;
using denoise::canon;
using denoise::kNoPixel;
using denoise::kTileDn;
using denoise::lum;
using denoise::tiny;

DEV float max0(float x) { return x > 0.0f ? x : 0.0f; }

struct Args {
    const float4 *accum;    // pitch_f4 per row
    const float4 *moments;  // pitch_f4 per row
    const float4 *guide;    // {n, t}, packed rows of `width`
    const float4 *albedo;   // {rgb, id}, packed
    float *v0;              // packed
    int pitch_f4, width, rows;
    float sigma_normal, sigma_depth;
    int demodulate;
};

constexpr int kHaloVar = 3, kSideVar = kTileDn + 2 * kHaloVar;

__global__ __launch_bounds__(256) void variance_estimate(const Args a) {
    __shared__ float4 sM[kSideVar * kSideVar], sG[kSideVar * kSideVar];
    const denoise::Tile16 t = denoise::tile16(a.width);
    const int x = t.x0 + t.tx, y = t.y0 + t.ty;
    for (int i = threadIdx.x; i < kSideVar * kSideVar; i += 256) {
        const int sy = i / kSideVar, sx = i - sy * kSideVar;
        const int gx = t.x0 - kHaloVar + sx, gy = t.y0 - kHaloVar + sy;
        float4 m = make_float4(0.f, 0.f, __int_as_float(kNoPixel), 0.f), g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (gx >= 0 && gx < a.width && gy >= 0 && gy < a.rows) {
            const size_t qa = (size_t)gy * a.pitch_f4 + gx, q = (size_t)gy * a.width + gx;
            const float4 s = a.accum[qa], mo = a.moments[qa], al = a.albedo[q];
            g = a.guide[q];
            if (!tiny(s.w) && __float_as_int(al.w) != kNoPixel) {
                m.z = al.w; m.w = mo.w;
                if (!tiny(mo.w)) { m.x = mo.x / mo.w; m.y = mo.y / mo.w; }
                else {
                    const float l = lum(s.x / s.w, s.y / s.w, s.z / s.w);
                    m.x = l; m.y = l * l;
                }
            }
        }
        sM[i] = m; sG[i] = g;
    }
    __syncthreads();
    if (x >= a.width || y >= a.rows) return;
    const int c = (t.ty + kHaloVar) * kSideVar + t.tx + kHaloVar;
    const float4 mp = sM[c];
    const int idp = __float_as_int(mp.z);
    float v = 0.0f;
    if (idp != kNoPixel) {
        if (mp.w >= 4.0f) v = max0(mp.y - mp.x * mp.x) / mp.w;
        else {
            const float4 gp = sG[c];
            const float tden = denoise::tden_of(gp);
            float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
            for (int dy = -3; dy <= 3; dy++) {
#pragma unroll
                for (int dx = -3; dx <= 3; dx++) {
                    const int i = c + dy * kSideVar + dx;
                    const float4 mq = sM[i];
                    if (__float_as_int(mq.z) == idp) {
                        const denoise::GeoTerm g = denoise::geometry_term(gp, tden, sG[i], a.sigma_normal, a.sigma_depth);
                        const float w = lp_exp(-(g.n + g.d));
                        sw = sw + w;
                        s1 = s1 + w * mq.x;
                        s2 = s2 + w * mq.y;
                    }
                }
            }
            const float den = denoise::weight_floor(sw);
            const float S1 = s1 / den, S2 = s2 / den;
            v = max0(S2 - S1 * S1);
        }
        if (a.demodulate) {
            const float4 al = a.albedo[(size_t)y * a.width + x];
            const float la = lum(albedo_of(al.x), albedo_of(al.y), albedo_of(al.z));
            v = v / (la * la);
        }
        v = canon(v);
    }
    a.v0[(size_t)y * a.width + x] = v;
}

}  // namespace variance

// (A namespace of its own: the kernels of the variance pass proper are counted by name.)
namespace adaptive_moments {

using variance::max0;

// The selection at the start of glrtx_render_adaptive_moments: which 8x8 tiles of the owned rows are still ACTIVE, from the moments plane as it stands.  Per pixel
// the temporal branch of the variance pass above, without demodulation, as a standard error of the mean luminance over the root of that mean:
//     force = !(M.w >= min_samples);   mu1 = M.x / M.w;   mu2 = M.y / M.w;   v = max(mu2 - mu1 * mu1, 0) / M.w;   d = sqrt(v) / sqrt(mu1 + kAdaptLumFloor)
// Lane k of the tile's wave holds pixel (k & 7, k >> 3) (0 outside the image); E is adaptive_select_kernel's tree sum over the in-image count.  A tile is active if a
// pixel forces, if threshold < 0 or if !(E <= threshold).  Writes the tile's mask byte and -- debug export only -- its E (a NaN as the canonical quiet NaN).
// host/variance.cpp (glrt_adaptive_select_moments) and tests/adaptive_moments_math.py state the same bit for bit.
__global__ __launch_bounds__(256) void select_kernel(const float4 *moments, int pitch_f4, int width, int rows, int tiles8_x, int n_tiles, float threshold, int min_samples,
                                                     unsigned char *mask, float *tile_err) {
    const int tile = blockIdx.x * 4 + (threadIdx.x >> 6), k = threadIdx.x & 63;
    if (tile >= n_tiles) return;  // (wave-uniform)
    const int x = (tile % tiles8_x) * 8 + (k & 7), y = (tile / tiles8_x) * 8 + (k >> 3);
    const bool in = x < width && y < rows;
    float d = 0.0f;
    bool force = false;
    if (in) {
        const float4 m = ld_stream(&moments[(size_t)y * pitch_f4 + x]);
        force = !(m.w >= (float)min_samples);
        const float mu1 = m.x / m.w, mu2 = m.y / m.w;
        const float v = max0(mu2 - mu1 * mu1) / m.w;
        d = __builtin_sqrtf(v) / __builtin_sqrtf(mu1 + kAdaptLumFloor);
    }
#pragma unroll
    for (int h = 32; h >= 1; h >>= 1) d = d + __shfl_xor(d, h, 64);  // (lane k adds lane k ^ h: lane 0 ends with the tree sum; addition commutes)
    const unsigned long long in_mask = __ballot(in), force_mask = __ballot(force);
    if (k == 0) {
        const float e = d / (float)__popcll(in_mask);
        mask[tile] = (force_mask != 0ull || threshold < 0.0f || !(e <= threshold)) ? 1 : 0;
        if (tile_err) tile_err[tile] = e != e ? __uint_as_float(0x7FC00000u) : e;
    }
}

}  // namespace adaptive_moments
}  // namespace glrtx
