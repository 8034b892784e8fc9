// statement_math.h -- what the CPU statements of the device's passes share (host/query.cpp, features.cpp, denoise.cpp, variance.cpp, reproject.cpp,
// reproject_motion.cpp, tonemap.cpp, bloom.cpp, reweight.cpp, normals.cpp, and the device-build statements in bvh.cpp; normal_topology.h, which the device
// library compiles as well, takes FlushDenormals and dot3 from here): the denormal mode they run under and the small fp32 helpers they are written in.  Internal
// to the host library; the kernels (csrc/) state the same helpers in their own source and share none of this.  Every operation is one correctly rounded IEEE
// operation in the order written (the callers are compiled with -ffp-contract=off; lp_exp's fmaf calls are the only fused ones).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#if defined(__SSE__)
#include <xmmintrin.h>
#endif

namespace glrt_detail {

// MXCSR FTZ | DAZ for the lifetime of the object: the device's arithmetic flushes fp32 denormals on input and output.  The caller's mode is restored.
struct FlushDenormals {
#if defined(__SSE__)
    unsigned csr = _mm_getcsr();
    FlushDenormals() { _mm_setcsr(csr | 0x8040u); }
    ~FlushDenormals() { _mm_setcsr(csr); }
#endif
};

inline uint32_t bits(float x) { uint32_t b; std::memcpy(&b, &x, 4); return b; }
inline float bits_f(uint32_t b) { float x; std::memcpy(&x, &b, 4); return x; }
// a NaN is stored as 0x7FC00000 on both sides (which NaN an operation yields is the one thing the two instruction sets do not share)
inline float canon(float x) { return x != x ? bits_f(0x7FC00000u) : x; }
inline bool tiny(float x) { return (bits(x) & 0x7F800000u) == 0u; }                     // a zero or a denormal
inline bool pos_finite(float x) { return (bits(x) - 0x00800000u) < 0x7F000000u; }       // sign clear, exponent neither 0 nor 255
inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return (az * bz + ay * by) + ax * bx; }
inline float lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// csrc/pt_kernel.hip.h: lp_exp.  (A NaN operand: the integer conversion is whatever it is, the result is NaN either way.)
inline float lp_exp(float x) {
    float t = x * bits_f(0x3fb8aa3bu);
    t = 128.0f < t ? 128.0f : t;
    t = bits_f(0xc2fdffffu) > t ? bits_f(0xc2fdffffu) : t;
    const float fl = std::floor(t);
    const float f = t - fl;
    const float p2 = bits_f((uint32_t)((fl == fl ? (int)fl : 0) + 127) << 23);
    const float z = f * f;
    const float a = std::fmaf(z, bits_f(0x3af61905u), bits_f(0x3d64aa23u));
    const float b = std::fmaf(z, bits_f(0x3c134806u), bits_f(0x3e75ead4u));
    const float c = std::fmaf(z, a, bits_f(0x3f31727bu));
    const float d = std::fmaf(z, b, 1.0f);
    return p2 * std::fmaf(c, f, d);
}

// The denoisers' planes (include/glrtx.h "Denoising")
constexpr int32_t kNoPixel = INT32_MIN;  // the id of a pixel without samples
constexpr float kAlbedoFloor = 1.0e-3f;
inline float albedo_of(float a) { return a > kAlbedoFloor ? a : kAlbedoFloor; }

// The normal/depth terms of a filter tap between p and q ({n, t} each): returns dn / sigma_normal, dd_out = min(dd / sigma_depth, 80); tden = max(t_p, 1e-6)
inline float geometry_terms(const float *gp, const float *gq, float tden, float sigma_normal, float sigma_depth, float &dd_out) {
    const float nx = gq[0] - gp[0], ny = gq[1] - gp[1], nz = gq[2] - gp[2];
    const float dn = (nx * nx + ny * ny) + nz * nz;
    const float rt = (gq[3] - gp[3]) / tden;
    const float dd = (rt * rt) / sigma_depth;
    dd_out = dd < 80.0f ? dd : 80.0f;
    return dn / sigma_normal;
}

}  // namespace glrt_detail
