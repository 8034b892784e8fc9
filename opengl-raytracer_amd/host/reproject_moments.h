// reproject_moments.h -- the moments plane M through the reprojection's taps (include/glrtx.h "Variance guidance": "Carrying M"), shared by glrt_reproject_moments
// and glrt_reproject_motion_moments as csrc/reproject.hip.h's moments_tap / moments_out are shared by the two kernels.  One correctly rounded fp32 operation
// at a time in the order written; the caller runs with denormals flushed.
#pragma once
#include <cmath>

#include "statement_math.h"

namespace glrt_detail {

struct MomSum { float sm = 0.0f, smc = 0.0f, s1 = 0.0f, s2 = 0.0f; };

// A tap that counts for the accumulator counts for M if M.w is neither a zero nor a denormal.
inline void moments_tap(MomSum &s, float w, const float *M) {
    if (tiny(M[3])) return;
    s.sm = s.sm + w;
    s.smc = s.smc + w * M[3];
    s.s1 = s.s1 + w * (M[0] / M[3]);
    s.s2 = s.s2 + w * (M[1] / M[3]);
}

// o = {(s1 / sm) * nm, (s2 / sm) * nm, 0, nm}, or zeros ("no moments").
inline void moments_out(const MomSum &s, float max_history, float *o) {
    o[0] = o[1] = o[2] = o[3] = 0.0f;
    if (!(s.sm > 1.0e-6f)) return;
    const float r = std::nearbyint(s.smc / s.sm);
    const float nm = r > max_history ? max_history : r;
    if (!(nm >= 1.0f)) return;
    o[0] = canon((s.s1 / s.sm) * nm); o[1] = canon((s.s2 / s.sm) * nm); o[3] = nm;
}

}  // namespace glrt_detail
