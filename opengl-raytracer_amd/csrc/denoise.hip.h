// denoise.hip.h -- the edge-avoiding a-trous wavelet filter (glrtx_denoise / glrtx_debug_denoise, include/glrtx.h "Denoising"; Dammertz et al. 2010).
//
// No reference counterpart.  The arithmetic is the header's text: host/denoise.cpp (glrt_denoise_atrous) and tests/denoise_math.py state it again, and all
// three agree bit for bit -- every fp32 operation below is one correctly rounded operation in the order written (-ffp-contract=off; lp_exp carries the only fused
// ones), denormals flushed, a NaN that is stored is 0x7FC00000.
//
// Passes, all on the context's stream:  denoise_prep  accumulator + albedo plane -> image 0, {I or I / max(albedo, 1e-3), id}: the material id rides in the
// colour's fourth word, replaced by kNoPixel where the pixel has no samples, so that ONE compare per tap applies all three exclusions (outside the image: the
// staged halo carries kNoPixel too; no samples; another material) and a tap is two 16-byte loads -- {rgb, id} and the feature plane's {n, t}.
// denoise_atrous<S, LAST>, once per iteration, ping-pong between two images; the last one multiplies the albedo back and writes D {rgb, 1}.
//   S = 1, 2 (spacings 1 and 2): a workgroup owns a 16x16 tile and stages colour and normal/depth of tile + halo (20^2 / 24^2 pixels, 12.5 / 18 KiB) in LDS with
//       16-byte loads; the 25 taps are ds_read_b128 pairs.
//   S = 0 (spacing >= 4): the halo (16 + 4 x spacing)^2 outgrows the tile -- 32^2 pixels for 256 outputs at spacing 4 -- and the taps go to L2 directly.
// Either way a wave is one 8x8 sub-tile (lane k at (k & 7, k >> 3), the wavefront kernel's tile order): a tap of a wave is 8 rows of 128 contiguous bytes.
// Groups are out of scope: a context filters the rows it owns, as one image in local row order.
// denoise_atrous_var<S, LAST>, at the end of the file, is the variance-guided form of the same iteration (glrtx_denoise_variance); denoise_atrous is not touched by it.
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
    int width, rows, spacing;
    float sigma_color_i, sigma_normal, sigma_depth;  // (sigma_color_i: sigma_color * 4^-i, a denormal flushed)
    int demodulate;
};

DEV float canon(float x) { return x != x ? __uint_as_float(0x7FC00000u) : x; }
DEV bool tiny(float x) { return (__float_as_uint(x) & 0x7F800000u) == 0u; }  // a zero or a denormal
DEV float albedo_of(float a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }

__global__ __launch_bounds__(256) void denoise_prep(const float4 *accum, int pitch_f4, const float4 *albedo, float4 *dst, int width, int rows, int demodulate) {
    const int tiles_x = (width + kTileDn - 1) / kTileDn;
    const int tile = blockIdx.x, w = threadIdx.x >> 6, k = threadIdx.x & 63;
    const int x = (tile % tiles_x) * kTileDn + (w & 1) * 8 + (k & 7), y = (tile / tiles_x) * kTileDn + (w >> 1) * 8 + (k >> 3);
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

struct Sum { float w, x, y, z; };

// One tap of the same material: w = k * lp_exp(-(dc / sc + dn / sn + min(dd / sd, 80)))
DEV void tap(const Args &a, float kk, float4 cp, float4 gp, float tden, float4 cq, float4 gq, Sum &s) {
    const float cx = cq.x - cp.x, cy = cq.y - cp.y, cz = cq.z - cp.z;
    const float dc = (cx * cx + cy * cy) + cz * cz;
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    const float dn = (nx * nx + ny * ny) + nz * nz;
    const float rt = (gq.w - gp.w) / tden;
    const float dd = (rt * rt) / a.sigma_depth;
    const float e = (dc / a.sigma_color_i + dn / a.sigma_normal) + (dd < 80.0f ? dd : 80.0f);
    const float w = kk * lp_exp(-e);
    s.w = s.w + w;
    s.x = s.x + w * cq.x; s.y = s.y + w * cq.y; s.z = s.z + w * cq.z;
}

constexpr float kKern[5] = {1.0f / 16, 4.0f / 16, 6.0f / 16, 4.0f / 16, 1.0f / 16};

template <int S, bool LAST>
__global__ __launch_bounds__(256) void denoise_atrous(const Args a) {
    constexpr int H = 2 * S, SIDE = kTileDn + 2 * H;
    __shared__ float4 sC[S > 0 ? SIDE * SIDE : 1], sG[S > 0 ? SIDE * SIDE : 1];
    const int tiles_x = (a.width + kTileDn - 1) / kTileDn;
    const int tile = blockIdx.x, wv = threadIdx.x >> 6, k = threadIdx.x & 63;
    const int x0 = (tile % tiles_x) * kTileDn, y0 = (tile / tiles_x) * kTileDn;
    const int tx = (wv & 1) * 8 + (k & 7), ty = (wv >> 1) * 8 + (k >> 3);
    const int x = x0 + tx, y = y0 + ty;
    if (S > 0) {
        for (int i = threadIdx.x; i < SIDE * SIDE; i += 256) {
            const int sy = i / SIDE, sx = i - sy * SIDE;
            const int gx = x0 - H + sx, gy = y0 - H + sy;
            const bool in = gx >= 0 && gx < a.width && gy >= 0 && gy < a.rows;
            const size_t q = (size_t)gy * a.width + gx;
            sC[i] = in ? a.src[q] : make_float4(0.f, 0.f, 0.f, __int_as_float(kNoPixel));
            sG[i] = in ? a.guide[q] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.rows) return;
    const size_t p = (size_t)y * a.width + x;
    const float4 cp = S > 0 ? sC[(ty + H) * SIDE + tx + H] : a.src[p];
    const int idp = __float_as_int(cp.w);
    float4 o = make_float4(0.f, 0.f, 0.f, LAST ? 1.0f : cp.w);
    if (idp != kNoPixel) {
        const float4 gp = S > 0 ? sG[(ty + H) * SIDE + tx + H] : a.guide[p];
        const float tden = gp.w > 1.0e-6f ? gp.w : 1.0e-6f;
        Sum s = {0.f, 0.f, 0.f, 0.f};
        const int sp = S > 0 ? S : a.spacing;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float kk = kKern[dy + 2] * kKern[dx + 2];
                if (S > 0) {
                    const int i = (ty + H + S * dy) * SIDE + tx + H + S * dx;
                    const float4 cq = sC[i];
                    if (__float_as_int(cq.w) == idp) tap(a, kk, cp, gp, tden, cq, sG[i], s);
                } else {
                    const int qx = x + sp * dx, qy = y + sp * dy;
                    if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.rows) {
                        const size_t q = (size_t)qy * a.width + qx;
                        const float4 cq = a.src[q];
                        if (__float_as_int(cq.w) == idp) tap(a, kk, cp, gp, tden, cq, a.guide[q], s);
                    }
                }
            }
        }
        const float den = s.w > 1.0e-20f ? s.w : 1.0e-20f;
        o.x = canon(s.x / den); o.y = canon(s.y / den); o.z = canon(s.z / den);
        if (LAST && a.demodulate) {
            const float4 al = a.albedo[p];
            o.x = canon(o.x * albedo_of(al.x)); o.y = canon(o.y * albedo_of(al.y)); o.z = canon(o.z * albedo_of(al.z));
        }
    }
    a.dst[p] = o;
}

// ---- the variance-guided form (glrtx_denoise_variance, include/glrtx.h "Variance guidance"; SVGF, Schied et al. 2017).  denoise_atrous's iteration with the colour
// term |lum(c_q) - lum(c_p)| / (sigma_lum * sqrt(g_p) + 1e-6), g_p the 3x3 Gaussian of the variance plane around p, and the variance filtered alongside with the
// squared weights.  The variance rides in a float plane that ping-pongs with the colour images; for S = 1, 2 it is staged with tile + halo like colour and
// normal/depth (36 B per pixel: 14.1 / 20.3 KiB) -- the halo is 2 S >= 2 pixels, so the 3x3's one-pixel ring is inside it; from spacing 4 everything goes to L2.
struct VarArgs {
    const float4 *src;   // {rgb, id}
    const float4 *guide; // {n, t}
    const float4 *albedo;
    float4 *dst;
    const float *vsrc;   // the variance plane, packed rows of `width`
    float *vdst;         // (not written by the last iteration)
    int width, rows, spacing;
    float sigma_lum, sigma_normal, sigma_depth;
    int demodulate;
};

struct VarSum { float w, x, y, z, v; };

DEV float lum_of(float4 c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }

DEV void tap_var(const VarArgs &a, float kk, float lp, float sdl, float4 gp, float tden, float4 cq, float4 gq, float vq, VarSum &s) {
    const float dl = __builtin_fabsf(lum_of(cq) - lp);
    const float nx = gq.x - gp.x, ny = gq.y - gp.y, nz = gq.z - gp.z;
    const float dn = (nx * nx + ny * ny) + nz * nz;
    const float rt = (gq.w - gp.w) / tden;
    const float dd = (rt * rt) / a.sigma_depth;
    const float e = (dl / sdl + dn / a.sigma_normal) + (dd < 80.0f ? dd : 80.0f);
    const float w = kk * lp_exp(-e);
    s.w = s.w + w;
    s.x = s.x + w * cq.x; s.y = s.y + w * cq.y; s.z = s.z + w * cq.z;
    s.v = s.v + (w * w) * vq;
}

constexpr float kKern3[3] = {0.25f, 0.5f, 0.25f};

template <int S, bool LAST>
__global__ __launch_bounds__(256) void denoise_atrous_var(const VarArgs a) {
    constexpr int H = 2 * S, SIDE = kTileDn + 2 * H;
    __shared__ float4 sC[S > 0 ? SIDE * SIDE : 1], sG[S > 0 ? SIDE * SIDE : 1];
    __shared__ float sV[S > 0 ? SIDE * SIDE : 1];
    const int tiles_x = (a.width + kTileDn - 1) / kTileDn;
    const int tile = blockIdx.x, wv = threadIdx.x >> 6, k = threadIdx.x & 63;
    const int x0 = (tile % tiles_x) * kTileDn, y0 = (tile / tiles_x) * kTileDn;
    const int tx = (wv & 1) * 8 + (k & 7), ty = (wv >> 1) * 8 + (k >> 3);
    const int x = x0 + tx, y = y0 + ty;
    if (S > 0) {
        for (int i = threadIdx.x; i < SIDE * SIDE; i += 256) {
            const int sy = i / SIDE, sx = i - sy * SIDE;
            const int gx = x0 - H + sx, gy = y0 - H + sy;
            const bool in = gx >= 0 && gx < a.width && gy >= 0 && gy < a.rows;
            const size_t q = (size_t)gy * a.width + gx;
            sC[i] = in ? a.src[q] : make_float4(0.f, 0.f, 0.f, __int_as_float(kNoPixel));
            sG[i] = in ? a.guide[q] : make_float4(0.f, 0.f, 0.f, 0.f);
            sV[i] = in ? a.vsrc[q] : 0.f;
        }
        __syncthreads();
    }
    if (x >= a.width || y >= a.rows) return;
    const size_t p = (size_t)y * a.width + x;
    const int c = (ty + H) * SIDE + tx + H;
    const float4 cp = S > 0 ? sC[c] : a.src[p];
    const int idp = __float_as_int(cp.w);
    float4 o = make_float4(0.f, 0.f, 0.f, LAST ? 1.0f : cp.w);
    float vo = 0.0f;
    if (idp != kNoPixel) {
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
        const float sdl = a.sigma_lum * __builtin_sqrtf(gs / gw) + 1.0e-6f;
        const float lp = lum_of(cp);
        const float4 gp = S > 0 ? sG[c] : a.guide[p];
        const float tden = gp.w > 1.0e-6f ? gp.w : 1.0e-6f;
        VarSum s = {0.f, 0.f, 0.f, 0.f, 0.f};
        const int sp = S > 0 ? S : a.spacing;
#pragma unroll
        for (int dy = -2; dy <= 2; dy++) {
#pragma unroll
            for (int dx = -2; dx <= 2; dx++) {
                const float kk = kKern[dy + 2] * kKern[dx + 2];
                if (S > 0) {
                    const int i = c + S * dy * SIDE + S * dx;
                    const float4 cq = sC[i];
                    if (__float_as_int(cq.w) == idp) tap_var(a, kk, lp, sdl, gp, tden, cq, sG[i], sV[i], s);
                } else {
                    const int qx = x + sp * dx, qy = y + sp * dy;
                    if (qx >= 0 && qx < a.width && qy >= 0 && qy < a.rows) {
                        const size_t q = (size_t)qy * a.width + qx;
                        const float4 cq = a.src[q];
                        if (__float_as_int(cq.w) == idp) tap_var(a, kk, lp, sdl, gp, tden, cq, a.guide[q], a.vsrc[q], s);
                    }
                }
            }
        }
        const float den = s.w > 1.0e-20f ? s.w : 1.0e-20f;
        o.x = canon(s.x / den); o.y = canon(s.y / den); o.z = canon(s.z / den);
        vo = canon(s.v / (den * den));
        if (LAST && a.demodulate) {
            const float4 al = a.albedo[p];
            o.x = canon(o.x * albedo_of(al.x)); o.y = canon(o.y * albedo_of(al.y)); o.z = canon(o.z * albedo_of(al.z));
        }
    }
    a.dst[p] = o;
    if (!LAST) a.vdst[p] = vo;
}

}  // namespace denoise
}  // namespace glrtx
