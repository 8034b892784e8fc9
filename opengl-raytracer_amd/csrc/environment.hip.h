// environment.hip.h -- environment lighting (include/glrtx.h "Environment"): one square octahedral HDR map, looked up where a path's ray misses (escape mode) or
// sampled as one more light through an importance grid (sampled mode).  The device statements of the rule: env_dir_to_st / env_st_to_dir (the mapping and its
// inverse), env_radiance, env_eval, env_sample -- used by the extension megakernel's environment instantiations (pt_kernel.hip.h: shade_core<true, TEX, true>,
// pt_render_persistent's ENV forms) and by the kernels behind the glrtx_debug_env_* hooks -- and env_weights_kernel, which sums the importance grid's cell weights.
//
// Why octahedral and not lat-long: the lookup sits on the shading path of a megakernel that is bound by instruction issue and vector memory.
// Direction -> (s, t) is three absolute values, one quotient and a few selects; lat-long needs atan2 and acos, neither of which has a bit-exact statement here.
// The map is read through tex_lookup (texture.hip.h) as it is: all three formats, nearest or bilinear, clamp on both axes.  Bilinear filtering across the fold
// seams is NOT corrected: at the square's edge a lookup reads what clamp gives it, not the texel on the other side of the fold.
//
// Every operation is one rounded fp32 operation in the order written (the file is compiled with -ffp-contract=off, denormals flushed); host/environment.cpp
// and tests/env_math.py state the same rule, bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "texture.hip.h"

namespace glrtx {

constexpr int ENV_ESCAPE = 0, ENV_SAMPLED = 1;
constexpr int kEnvGridMax = 1024;
constexpr int kEnvWeightThreads = 64;  // env_weights_kernel: one wave a cell

// What the kernels take of a bound environment; it travels in the kernarg block behind ExtArgs.  The tables are read in sampled mode only.
struct EnvArgs {
    TexDesc desc;                  // the map: square, clamp on both axes, offset 0
    const unsigned char *texels;
    const float *row_q;            // [G]      row alias table: thresholds ...
    const int *row_alias;          // [G]      ... and aliases
    const float *col_q;            // [G * G]  one alias table a row, over its columns
    const int *col_alias;          // [G * G]
    const float *cell_p;           // [G * G]  probability of cell (row j, column i) at j * G + i
    float R[9];                    // row-major rotation: map space = R * world
    float scale[3];
    int mode;                      // ENV_*
    float p_env;                   // light_pick (the launch forces 1 for a scene without lights)
    int G;
};

// abs / sign helpers: sgn(0) = sgn(-0) = +1
TEX_DEV float env_signed(float m, float of) { return of < 0.0f ? -m : m; }

// Direction (not normalised) -> (s, t).  false: the L1 norm is zero or not finite, the radiance is 0.  n1 = the L1 norm of the unit direction, from the
// direction scaled to L1 norm 1 (p = e / l, n1 = 1 / |p|: no overflow for a long direction, no underflow for a short one).
TEX_DEV bool env_dir_to_st(const float *R, float dx, float dy, float dz, float &s, float &t, float &n1) {
    const float ex = (R[0] * dx + R[1] * dy) + R[2] * dz;
    const float ey = (R[3] * dx + R[4] * dy) + R[5] * dz;
    const float ez = (R[6] * dx + R[7] * dy) + R[8] * dz;
    const float l = (__builtin_fabsf(ex) + __builtin_fabsf(ey)) + __builtin_fabsf(ez);
    s = t = n1 = 0.0f;
    if (!(l > 0.0f && l < __builtin_inff())) return false;
    float px = ex / l, pz = ez / l;
    const float py = ey / l;
    n1 = 1.0f / __builtin_sqrtf((pz * pz + py * py) + px * px);
    if (ey < 0.0f) {  // the lower half folds outward over the square's corners
        const float fx = env_signed(1.0f - __builtin_fabsf(pz), px);
        const float fz = env_signed(1.0f - __builtin_fabsf(px), pz);
        px = fx; pz = fz;
    }
    s = px * 0.5f + 0.5f;
    t = pz * 0.5f + 0.5f;
    return true;
}

// (s, t) -> unit direction in world space; n1 = the L1 norm of the unit direction (the solid-angle factor: dOmega = 4 n1^3 ds dt)
TEX_DEV void env_st_to_dir(const float *R, float s, float t, float &dx, float &dy, float &dz, float &n1) {
    const float u = s * 2.0f - 1.0f, v = t * 2.0f - 1.0f;
    const float au = __builtin_fabsf(u), av = __builtin_fabsf(v);
    const float y = (1.0f - au) - av;
    float x = u, z = v;
    if (y < 0.0f) {
        x = env_signed(1.0f - av, u);
        z = env_signed(1.0f - au, v);
    }
    const float r = 1.0f / __builtin_sqrtf((z * z + y * y) + x * x);
    const float qx = x * r, qy = y * r, qz = z * r;
    n1 = r * ((__builtin_fabsf(x) + __builtin_fabsf(y)) + __builtin_fabsf(z));
    dx = (R[0] * qx + R[3] * qy) + R[6] * qz;  // R^T
    dy = (R[1] * qx + R[4] * qy) + R[7] * qz;
    dz = (R[2] * qx + R[5] * qy) + R[8] * qz;
}
TEX_DEV float env_jacobian(float n1) { return 4.0f * ((n1 * n1) * n1); }

TEX_DEV float3 env_lookup(const EnvArgs &env, float s, float t) {
    TexSet ts;
    ts.desc = &env.desc; ts.texels = env.texels; ts.tri_st = nullptr; ts.mat_tex = nullptr; ts.n_tex = 1;
    const float3 c = tex_lookup(ts, 0, s, t);
    return make_float3(env.scale[0] * c.x, env.scale[1] * c.y, env.scale[2] * c.z);
}

// Le(d): what a ray that leaves the scene along d sees
TEX_DEV float3 env_radiance(const EnvArgs &env, float dx, float dy, float dz) {
    float s, t, n1;
    if (!env_dir_to_st(env.R, dx, dy, dz, s, t, n1)) return make_float3(0.f, 0.f, 0.f);
    return env_lookup(env, s, t);
}

// The grid cell of a coordinate along one axis: (int)(s * G) kept inside 0 .. G - 1 (a NaN: cell 0)
TEX_DEV int env_cell(float s, int G) {
    const float a = s * (float)G;
    return a >= 0.0f ? (a < (float)G ? (int)a : G - 1) : 0;
}
TEX_DEV float env_pdf(const EnvArgs &env, int ci, int cj, float n1) {
    const float g2 = (float)env.G * (float)env.G;
    return ((env.cell_p[cj * env.G + ci] * g2) / env_jacobian(n1)) * env.p_env;
}

// direction -> radiance and the solid-angle pdf sampled mode draws it with (0 where the direction has no (s, t))
TEX_DEV float3 env_eval(const EnvArgs &env, float dx, float dy, float dz, float &pdf) {
    float s, t, n1;
    pdf = 0.0f;
    if (!env_dir_to_st(env.R, dx, dy, dz, s, t, n1)) return make_float3(0.f, 0.f, 0.f);
    pdf = env_pdf(env, env_cell(s, env.G), env_cell(t, env.G), n1);
    return env_lookup(env, s, t);
}

// Six uniforms -> direction, pdf, radiance: a row through the row table (u0 entry, u1 threshold), a column through that row's table (u2, u3), a jittered point
// of the cell (u4, u5), the inverse mapping, the lookup at that (s, t).
TEX_DEV float3 env_sample(const EnvArgs &env, float u0, float u1, float u2, float u3, float u4, float u5, float &dx, float &dy, float &dz, float &pdf) {
    const int G = env.G;
    int cj = env_cell(u0, G);
    cj = u1 < env.row_q[cj] ? cj : env.row_alias[cj];
    int ci = env_cell(u2, G);
    const int k = cj * G + ci;
    ci = u3 < env.col_q[k] ? ci : env.col_alias[k];
    const float s = ((float)ci + u4) / (float)G, t = ((float)cj + u5) / (float)G;
    float n1;
    env_st_to_dir(env.R, s, t, dx, dy, dz, n1);
    pdf = env_pdf(env, ci, cj, n1);
    return env_lookup(env, s, t);
}

TEX_DEV float env_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// The texel block of cell index c along one axis: the texels that overlap [c / G, (c + 1) / G), widened by one on either side, clamped to the map
TEX_DEV void env_block(int c, int N, int G, int &lo, int &hi) {
    lo = (c * N) / G - 1;
    hi = ((c + 1) * N + G - 1) / G;  // (the last overlapping texel, + 1)
    lo = lo < 0 ? 0 : lo;
    hi = hi > N - 1 ? N - 1 : hi;
}

// Cell weights of the importance grid: out[j * G + i] = sum over the cell's texel block of max(luminance(scale * texel), 0) * 4 n1^3 at the texel centres.
// One wave a cell.  The order of the sum is fixed: lane k adds the block's texels k, k + 64, k + 128, .. (row-major inside the block) in that order, starting
// from 0; then the 64 partial sums are folded p[k] += p[k + h] for h = 32, 16, .. 1.  No atomics.
__global__ __launch_bounds__(kEnvWeightThreads) void env_weights_kernel(const EnvArgs env, float *out) {
    __shared__ float part[kEnvWeightThreads];
    const int G = env.G, N = env.desc.width;
    const int ci = blockIdx.x, cj = blockIdx.y;
    int x0, x1, y0, y1;
    env_block(ci, N, G, x0, x1);
    env_block(cj, N, G, y0, y1);
    const int bw = x1 - x0 + 1, n = bw * (y1 - y0 + 1);
    TexSet ts;
    ts.desc = &env.desc; ts.texels = env.texels; ts.tri_st = nullptr; ts.mat_tex = nullptr; ts.n_tex = 1;
    float sum = 0.0f;
    for (int k = threadIdx.x; k < n; k += kEnvWeightThreads) {
        const int x = x0 + k % bw, y = y0 + k / bw;
        const float3 c = tex_texel(ts, env.desc, x, y);
        const float s = ((float)x + 0.5f) / (float)N, t = ((float)y + 0.5f) / (float)N;
        float dx, dy, dz, n1;
        env_st_to_dir(env.R, s, t, dx, dy, dz, n1);
        const float w = env_lum(env.scale[0] * c.x, env.scale[1] * c.y, env.scale[2] * c.z) * env_jacobian(n1);
        sum = sum + ((w > 0.0f && w < __builtin_inff()) ? w : 0.0f);
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int h = kEnvWeightThreads / 2; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h) part[threadIdx.x] = part[threadIdx.x] + part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[cj * G + ci] = part[0];
}

// glrtx_debug_env_eval: out[4i..] = {Le.rgb, pdf} of dir[3i..]
__global__ __launch_bounds__(256) void env_eval_kernel(const EnvArgs env, const float *dir, unsigned n, float *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float pdf;
    const float3 c = env_eval(env, dir[3 * i], dir[3 * i + 1], dir[3 * i + 2], pdf);
    out[4 * i] = c.x; out[4 * i + 1] = c.y; out[4 * i + 2] = c.z; out[4 * i + 3] = pdf;
}

// glrtx_debug_env_sample: out[8i..] = {direction, pdf, Le.rgb, 0} of the six uniforms u[6i..]
__global__ __launch_bounds__(256) void env_sample_kernel(const EnvArgs env, const float *u, unsigned n, float *out) {
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float dx, dy, dz, pdf;
    const float3 c = env_sample(env, u[6 * i], u[6 * i + 1], u[6 * i + 2], u[6 * i + 3], u[6 * i + 4], u[6 * i + 5], dx, dy, dz, pdf);
    out[8 * i] = dx; out[8 * i + 1] = dy; out[8 * i + 2] = dz; out[8 * i + 3] = pdf;
    out[8 * i + 4] = c.x; out[8 * i + 5] = c.y; out[8 * i + 6] = c.z; out[8 * i + 7] = 0.0f;
}

}  // namespace glrtx
