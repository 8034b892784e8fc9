// denoise.hip.h -- the edge-avoiding a-trous wavelet filter (glrtx_denoise / glrtx_debug_denoise, include/glrtx.h "Denoising"; Dammertz et al. 2010) and its
// variance-guided form (glrtx_denoise_variance, include/glrtx.h "Variance guidance"; SVGF, Schied et al. 2017): one iteration, stated once.
//
// No reference counterpart.  The arithmetic is the header's text: host/denoise.cpp (glrt_denoise_atrous, glrt_denoise_variance) and tests/denoise_math.py /
// tests/variance_math.py state it again, and all three agree bit for bit -- every fp32 operation below is one correctly rounded operation in the order written
// (-ffp-contract=off; lp_exp carries the only fused ones), denormals flushed, a NaN that is stored is 0x7FC00000.
//
// Passes, all on the context's stream:  denoise_prep  accumulator + albedo plane -> image 0, {I or I / max(albedo, 1e-3), id}: the material id rides in the
// colour's fourth word, replaced by kNoPixel where the pixel has no samples, so that ONE compare per tap applies all three exclusions (outside the image: the
// staged halo carries kNoPixel too; no samples; another material) and a tap is two 16-byte loads -- {rgb, id} and the feature plane's {n, t}.
// atrous<S, LAST, VAR>, once per iteration, ping-pong between two images; the last one multiplies the albedo back and writes D {rgb, 1}.
//   S = 1, 2 (spacings 1 and 2): a workgroup owns a 16x16 tile and stages colour and normal/depth of tile + halo (20^2 / 24^2 pixels, 12.5 / 18 KiB) in LDS with
//       16-byte loads; the 25 taps are ds_read_b128 pairs.
//   S = 0 (spacing >= 4): the halo (16 + 4 x spacing)^2 outgrows the tile -- 32^2 pixels for 256 outputs at spacing 4 -- and the taps go to L2 directly.
//   VAR: the colour term is |lum(c_q) - lum(c_p)| / (sigma_lum * sqrt(g_p) + 1e-6), g_p the 3x3 Gaussian of the variance plane around p, and the variance is
//       filtered alongside with the squared weights.  The variance rides in a float plane that ping-pongs with the colour images; for S = 1, 2 it is staged
//       with tile + halo like colour and normal/depth (36 B per pixel: 14.1 / 20.3 KiB) -- the halo is 2 S >= 2 pixels, so the 3x3's one-pixel ring is inside
//       it; from spacing 4 everything goes to L2.  Everything of it sits behind `if constexpr (VAR)`: the plain form declares no LDS for the plane.
// Either way a wave is one 8x8 sub-tile (lane k at (k & 7, k >> 3), the wavefront kernel's tile order): a tap of a wave is 8 rows of 128 contiguous bytes.
// Groups are out of scope: a context filters the rows it owns, as one image in local row order.
// The kernels are denoise_atrous<S, LAST> and denoise_atrous_var<S, LAST>: two names for atrous<S, LAST, false / true>, one argument struct.
// The pieces variance_estimate (variance.hip.h) shares with the filter are here too: Tile16, geometry_term, lum, and canon / tiny (reproject.hip.h's as well).
#pragma once
#include "pt_kernel.hip.h"

namespace glrtx {
namespace denoise {

constexpr int kNoPixel = INT32_MIN;  // id of a pixel without samples (reserved: a feature plane that carries it marks the pixel as one)
constexpr float kAlbedoFloor = 1.0e-3f;
constexpr int kTileDn = 16;

struct Args {
    const float4 *src;   // {rgb, id}, packed rows of `width`
    const float4 *guide; // {n, t}
    const float4 *albedo;  // {rgb, id}: read by the last iteration when demodulating
    float4 *dst;
    const float *vsrc;   // VAR: the variance plane, packed rows of `width`
    float *vdst;         // VAR (not written by the last iteration)
    int width, rows, spacing;
    float sigma_c;       // the colour term's: sigma_color * 4^-i, a denormal flushed; VAR: sigma_lum
    float sigma_normal, sigma_depth;
    int demodulate;
};

DEV float canon(float x) { return x != x ? __uint_as_float(0x7FC00000u) : x; }
DEV bool tiny(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0u; }  // a zero or a denormal
DEV float albedo_of(float a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }
DEV float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// A workgroup's 16x16 tile (x0, y0) and a thread's pixel (tx, ty) in it: wave w is the 8x8 sub-tile (w & 1, w >> 1), lane k its pixel (k & 7, k >> 3).
struct Tile16 { int x0, y0, tx, ty; };
DEV Tile16 tile16(int width) {
    const int tiles_x = (width + kTileDn - 1) / kTileDn;
    const int tile = blockIdx.x, wv = threadIdx.x >> 6, k = threadIdx.x & 63;
    return {(tile % tiles_x) * kTileDn, (tile / tiles_x) * kTileDn, (wv & 1) * 8 + (k & 7), (wv >> 1) * 8 + (k >> 3)};
}

// The normal/depth terms of a tap's exponent: {dn / sigma_normal, min(dd / sigma_depth, 80)}, dd the squared depth difference relative to tden = max(t_p, 1e-6).
// (Two terms, not their sum: the filter adds its colour term to the first before the second.)
struct GeoTerm { float n, d; };
DEV float tden_of(float4 gp) { return gp.w > 1.0e-6f ? gp.w : 1.0e-6f; }
DEV GeoTerm geometry_term(float4 gp, float tden, float4 gq, float sigma_normal, float sigma_depth) {
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    const float dn = (nx * nx + ny * ny) + nz * nz;
    const float rt = (gq.w - gp.w) / tden;
    const float dd = (rt * rt) / sigma_depth;
    return {dn / sigma_normal, dd < 80.0f ? dd : 80.0f};
}
DEV float weight_floor(float sw) { return sw > 1.0e-20f ? sw : 1.0e-20f; }  // a sum of weights as a divisor

__global__ __launch_bounds__(256) void denoise_prep(const float4 *accum, int pitch_f4, const float4 *albedo, float4 *dst, int width, int rows, int demodulate) {
    const Tile16 t = tile16(width);
    const int x = t.x0 + t.tx, y = t.y0 + t.ty;
    if (x >= width || y >= rows) return;
    const float4 s = accum[(size_t)y * pitch_f4 + x];
    const float4 al = albedo[(size_t)y * width + x];
    float4 o = make_float4(0.f, 0.f, 0.f, __int_as_float(kNoPixel));
    if (!tiny(s.w) && __float_as_int(al.w) != kNoPixel) {
        float r = s.x / s.w, g = s.y / s.w, b = s.z / s.w;
        if (demodulate) { r = r / albedo_of(al.x); g = g / albedo_of(al.y); b = b / albedo_of(al.z); }
        o = make_float4(canon(r), canon(g), canon(b), al.w);
    }
    dst[(size_t)y * width + x] = o;
}

struct Centre { float4 c, g; float tden, lp, sdl; };  // p's colour and normal/depth; VAR: lum(c_p) and sigma_lum * sqrt(g_p) + 1e-6
struct Sum { float w, x, y, z, v; };                  // (v: VAR)

// One tap of the same material: w = k * lp_exp(-(colour term + dn / sn + min(dd / sd, 80))); the colour term is dc / sc, VAR: |lum(c_q) - lum(c_p)| / sdl
template <bool VAR>
DEV void tap(const Args &a, float kk, const Centre &p, float4 cq, float4 gq, float vq, Sum &s) {
    float dc, sc;  // the colour term dc / sc (divided where the exponent is summed, as the statements have it)
    if constexpr (VAR) { dc = __builtin_fabsf(lum(cq.x, cq.y, cq.z) - p.lp); sc = p.sdl; }
    else {
        const float cx = cq.x - p.c.x, cy = cq.y - p.c.y, cz = cq.z - p.c.z;
        dc = (cx * cx + cy * cy) + cz * cz;
        sc = a.sigma_c;
    }
    const GeoTerm t = geometry_term(p.g, p.tden, gq, a.sigma_normal, a.sigma_depth);
    const float e = (dc / sc + t.n) + t.d;
    const float w = kk * lp_exp(-e);
    s.w = s.w + w;
    s.x = s.x + w * cq.x; s.y = s.y + w * cq.y; s.z = s.z + w * cq.z;
    if constexpr (VAR) s.v = s.v + (w * w) * vq;
}

constexpr float kKern[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};
constexpr float kKern3[3] = {0.25f, 0.5f, 0.25f};

template <int S, bool LAST, bool VAR>
DEV void atrous(const Args &a) {
    constexpr int H = 2 * S, SIDE = kTileDn + 2 * H;
    __shared__ float4 sC[S > 0 ? SIDE * SIDE : 1], sG[S > 0 ? SIDE * SIDE : 1];
    __shared__ float sV[VAR && S > 0 ? SIDE * SIDE : 1];  // (referenced under `if constexpr (VAR)` alone: the plain form has none)
    const Tile16 t = tile16(a.width);
    const int x = t.x0 + t.tx, y = t.y0 + t.ty;
    if (S > 0) {
        for (int i = threadIdx.x; i < SIDE * SIDE; i += 256) {
            const int sy = i / SIDE, sx = i - sy * SIDE;
            const int gx = t.x0 - H + sx, gy = t.y0 - H + sy;
            const bool in = gx >= 0 && gx < a.width && gy >= 0 && gy < a.rows;
            const size_t q = (size_t)gy * a.width + gx;
            sC[i] = in ? a.src[q] : make_float4(0.f, 0.f, 0.f, __int_as_float(kNoPixel));
            sG[i] = in ? a.guide[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            if constexpr (VAR) sV[i] = in ? a.vsrc[q] : 0.f;
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.rows) return;
    const size_t p = (size_t)y * a.width + x;
    const int c = (t.ty + H) * SIDE + t.tx + H;
    Centre ctr;
    ctr.c = S > 0 ? sC[c] : a.src[p];
    const int idp = __float_as_int(ctr.c.w);
    float4 o = make_float4(0.f, 0.f, 0.f, LAST ? 1.0f : ctr.c.w);
    float vo = 0.0f;
    if (idp != kNoPixel) {
        if constexpr (VAR) {
            // g_p: the 3x3 Gaussian of the variance over the taps inside, alive and of p's id (the centre always is)
            float gs = 0.0f, gw = 0.0f;
#pragma unroll
            for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
                for (int dx = -1; dx <= 1; dx++) {
                    const float kw = kKern3[dy + 1] * kKern3[dx + 1];
                    if (S > 0) {
                        const int i = c + dy * SIDE + dx;
                        if (__float_as_int(sC[i].w) == idp) { gs = gs + kw * sV[i]; gw = gw + kw; }
                    } else {
                        const int qx = x + dx, qy = y + dy;
                        if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.rows) {
                            const size_t q = (size_t)qy * a.width + qx;
                            if (__float_as_int(a.src[q].w) == idp) { gs = gs + kw * a.vsrc[q]; gw = gw + kw; }
                        }
                    }
                }
            }
            ctr.sdl = a.sigma_c * __builtin_sqrtf(gs / gw) + 1.0e-6f;
            ctr.lp = lum(ctr.c.x, ctr.c.y, ctr.c.z);
        }
        ctr.g = S > 0 ? sG[c] : a.guide[p];
        ctr.tden = tden_of(ctr.g);
        Sum s = {0.f, 0.f, 0.f, 0.f, 0.f};
        const int sp = S > 0 ? S : a.spacing;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float kk = kKern[dy + 2] * kKern[dx + 2];
                float vq = 0.0f;
                if (S > 0) {
                    const int i = c + S * dy * SIDE + S * dx;
                    const float4 cq = sC[i];
                    if (__float_as_int(cq.w) == idp) {
                        if constexpr (VAR) vq = sV[i];
                        tap<VAR>(a, kk, ctr, cq, sG[i], vq, s);
                    }
                } else {
                    const int qx = x + sp * dx, qy = y + sp * dy;
                    if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.rows) {
                        const size_t q = (size_t)qy * a.width + qx;
                        const float4 cq = a.src[q];
                        if (__float_as_int(cq.w) == idp) {
                            if constexpr (VAR) vq = a.vsrc[q];
                            tap<VAR>(a, kk, ctr, cq, a.guide[q], vq, s);
                        }
                    }
                }
            }
        }
        const float den = weight_floor(s.w);
        o.x = canon(s.x / den); o.y = canon(s.y / den); o.z = canon(s.z / den);
        if constexpr (VAR) vo = canon(s.v / (den * den));
        if (LAST && a.demodulate) {
            const float4 al = a.albedo[p];
            o.x = canon(o.x * albedo_of(al.x)); o.y = canon(o.y * albedo_of(al.y)); o.z = canon(o.z * albedo_of(al.z));
        }
    }
    a.dst[p] = o;
    if constexpr (VAR && !LAST) a.vdst[p] = vo;
}

template <int S, bool LAST>
__global__ __launch_bounds__(256) void denoise_atrous(const Args a) { atrous<S, LAST, false>(a); }
template <int S, bool LAST>
__global__ __launch_bounds__(256) void denoise_atrous_var(const Args a) { atrous<S, LAST, true>(a); }

}  // namespace denoise
}  // namespace glrtx
