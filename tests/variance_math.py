"""numpy statement of the variance-guided denoiser (include/glrtx.h "Variance guidance"; csrc/variance.hip.h, csrc/denoise.hip.h; host/variance.cpp).

The rules are denoise_math's: every operation is one IEEE float32 operation, correctly rounded, in the kernel's order; lp_exp carries the only fused
operations; denormals count as zeros of their sign on the way into and out of every operation; a NaN that is STORED is 0x7FC00000.
"""
from __future__ import annotations

import numpy as np

import denoise_math as dm
from adaptive_math import _op, ftz
from denoise_math import ALBEDO_FLOOR, KERN, NO_PIXEL, add, canon, div, fmax_c, mul, sub, tiny
from volume_math import lp_exp

f32 = np.float32
LR, LG, LB = f32(0.2126), f32(0.7152), f32(0.0722)
KERN3 = np.array([0.25, 0.5, 0.25], np.float32)


def lum(r, g, b):
    return add(add(mul(LR, r), mul(LG, g)), mul(LB, b))


def max0(x):
    """x > 0 ? x : 0 (a NaN gives 0)."""
    x = ftz(x)
    with np.errstate(invalid="ignore"):
        return np.where(x > f32(0), x, f32(0)).astype(np.float32)


def fold_moments(moments, planes):
    """M after the sample planes (k, rows, width, 4) were folded into it, in order: M.x += l; M.y += l * l; M.w += 1."""
    m = np.array(moments, np.float32, copy=True)
    for p in np.asarray(planes, np.float32):
        l = lum(p[..., 0], p[..., 1], p[..., 2])
        m[..., 0] = add(m[..., 0], l)
        m[..., 1] = add(m[..., 1], mul(l, l))
        m[..., 3] = add(m[..., 3], f32(1))
    return m


def _shifts(rows, width, oy, ox):
    y0, y1 = max(0, -oy), min(rows, rows - oy)
    x0, x1 = max(0, -ox), min(width, width - ox)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))


def _geometry_terms(g, tden, sn, sd, P, Q):
    n = sub(g[Q][..., :3], g[P][..., :3])
    dn = add(add(mul(n[..., 0], n[..., 0]), mul(n[..., 1], n[..., 1])), mul(n[..., 2], n[..., 2]))
    rt = div(sub(g[Q][..., 3], g[P][..., 3]), tden[P])
    dd = div(mul(rt, rt), sd)
    with np.errstate(invalid="ignore"):
        dd = np.where(dd < f32(80), dd, f32(80)).astype(np.float32)
    return div(dn, sn), dd


def _prepare(accum, albedo_id):
    acc = np.ascontiguousarray(accum, np.float32)
    al = np.ascontiguousarray(albedo_id, np.float32)
    ids = al[..., 3].view(np.int32).copy()
    dead = tiny(acc[..., 3]) | (ids == NO_PIXEL)
    ids[dead] = NO_PIXEL
    return acc, al, ids, dead, fmax_c(al[..., :3], ALBEDO_FLOOR)


def variance_estimate(accum, moments, normal_depth, albedo_id, sigma_normal, sigma_depth, demodulate):
    """V0, (rows, width) float32: the variance of each pixel's mean luminance."""
    acc, al, ids, dead, alb = _prepare(accum, albedo_id)
    M = np.ascontiguousarray(moments, np.float32)
    g = np.ascontiguousarray(normal_depth, np.float32)
    rows, width = acc.shape[:2]
    sn, sd = f32(sigma_normal), f32(sigma_depth)
    own = ~tiny(M[..., 3])
    I = div(acc[..., :3], acc[..., 3:4])
    li = lum(I[..., 0], I[..., 1], I[..., 2])
    mu1 = np.where(own, div(M[..., 0], M[..., 3]), li).astype(np.float32)
    mu2 = np.where(own, div(M[..., 1], M[..., 3]), mul(li, li)).astype(np.float32)
    with np.errstate(invalid="ignore"):
        temporal = ftz(M[..., 3]) >= f32(4)
    vt = div(max0(sub(mu2, mul(mu1, mu1))), M[..., 3])
    tden = fmax_c(g[..., 3], f32(1e-6))
    sw = np.zeros((rows, width), np.float32)
    s1 = np.zeros((rows, width), np.float32)
    s2 = np.zeros((rows, width), np.float32)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            pq = _shifts(rows, width, dy, dx)
            if pq is None:
                continue
            P, Q = pq
            ok = (ids[Q] == ids[P]) & ~dead[P]
            tn, dd = _geometry_terms(g, tden, sn, sd, P, Q)
            w = ftz(lp_exp(-add(tn, dd)))
            sw[P] = np.where(ok, add(sw[P], w), sw[P])
            s1[P] = np.where(ok, add(s1[P], mul(w, mu1[Q])), s1[P])
            s2[P] = np.where(ok, add(s2[P], mul(w, mu2[Q])), s2[P])
    den = fmax_c(sw, f32(1e-20))
    S1, S2 = div(s1, den), div(s2, den)
    vs = max0(sub(S2, mul(S1, S1)))
    v = np.where(temporal, vt, vs).astype(np.float32)
    if demodulate:
        la = lum(alb[..., 0], alb[..., 1], alb[..., 2])
        v = div(v, mul(la, la))
    return canon(np.where(dead, f32(0), v))


def denoise_variance(accum, moments, normal_depth, albedo_id, iterations, sigma_lum, sigma_normal, sigma_depth, demodulate, return_v0=False):
    """D, (rows, width, 4) float32 {rgb, 1}: the variance-guided a-trous filter; with return_v0 also V0."""
    acc, al, ids, dead, alb = _prepare(accum, albedo_id)
    g = np.ascontiguousarray(normal_depth, np.float32)
    rows, width = acc.shape[:2]
    v0 = variance_estimate(accum, moments, normal_depth, albedo_id, sigma_normal, sigma_depth, demodulate)
    c = div(acc[..., :3], acc[..., 3:4])
    if demodulate:
        c = div(c, alb)
    c = canon(np.where(dead[..., None], f32(0), c))
    v = v0.copy()
    sl, sn, sd = f32(sigma_lum), f32(sigma_normal), f32(sigma_depth)
    tden = fmax_c(g[..., 3], f32(1e-6))
    for it in range(iterations):
        sp = 1 << it
        # g_p: the 3x3 Gaussian of the current variance, unit spacing, over the taps that are inside, alive and carry p's id
        gs = np.zeros((rows, width), np.float32)
        gw = np.zeros((rows, width), np.float32)
        for dy in range(-1, 2):
            for dx in range(-1, 2):
                pq = _shifts(rows, width, dy, dx)
                if pq is None:
                    continue
                P, Q = pq
                ok = (ids[Q] == ids[P]) & ~dead[P]
                kw = mul(KERN3[dy + 1], KERN3[dx + 1])
                gs[P] = np.where(ok, add(gs[P], mul(kw, v[Q])), gs[P])
                gw[P] = np.where(ok, add(gw[P], kw), gw[P])
        gp = div(gs, gw)
        sdl = add(mul(sl, _op(np.sqrt, gp)), f32(1e-6))
        l = lum(c[..., 0], c[..., 1], c[..., 2])
        sw = np.zeros((rows, width), np.float32)
        s = np.zeros((rows, width, 3), np.float32)
        sv = np.zeros((rows, width), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                pq = _shifts(rows, width, sp * dy, sp * dx)
                if pq is None:
                    continue
                P, Q = pq
                ok = (ids[Q] == ids[P]) & ~dead[P]
                dl = np.abs(sub(l[Q], l[P]))
                tn, dd = _geometry_terms(g, tden, sn, sd, P, Q)
                e = add(add(div(dl, sdl[P]), tn), dd)
                w = mul(mul(KERN[dy + 2], KERN[dx + 2]), ftz(lp_exp(-e)))
                sw[P] = np.where(ok, add(sw[P], w), sw[P])
                s[P] = np.where(ok[..., None], add(s[P], mul(w[..., None], c[Q])), s[P])
                sv[P] = np.where(ok, add(sv[P], mul(mul(w, w), v[Q])), sv[P])
        den = fmax_c(sw, f32(1e-20))
        c = canon(np.where(dead[..., None], f32(0), div(s, den[..., None])))
        v = canon(np.where(dead, f32(0), div(sv, mul(den, den))))
    out = np.ones((rows, width, 4), np.float32)
    if demodulate:
        c = np.where(dead[..., None], c, canon(mul(c, alb)))
    out[..., :3] = c
    return (out, v0) if return_v0 else out


def moments_of(accum, rng, spread=0.5):
    """A plausible M for an accumulator: count = acc.w, mean luminance that of the accumulator, second moment mean^2 * (1 + spread * u)."""
    acc = np.asarray(accum, np.float32)
    n = acc[..., 3]
    with np.errstate(all="ignore"):
        l = np.nan_to_num(lum(*[div(acc[..., k], n) for k in range(3)]), nan=0.0, posinf=1e30, neginf=-1e30).astype(np.float32)
    M = np.zeros_like(acc)
    M[..., 0] = l * n
    M[..., 1] = l * l * (1 + spread * rng.uniform(0, 1, n.shape)).astype(np.float32) * n
    M[..., 3] = n
    return np.nan_to_num(M, nan=0.0, posinf=3e38, neginf=-3e38).astype(np.float32)


def hostile_arrays(rows, width, seed):
    """denoise_math.hostile_arrays with a moments plane M: counts 0 .. 5 (0, 1, 3 take the spatial branch, 4, 5 the temporal one), then -- where the image has
    room -- M.w zero, denormal, 1, 3, 4, 5, NaN and Inf at fixed spots, moments with mu2 < mu1^2, and NaN / Inf / denormal sums."""
    acc, N, A = dm.hostile_arrays(rows, width, seed)
    rng = np.random.default_rng(seed + 7919)
    cnt = rng.integers(0, 6, (rows, width)).astype(np.float32)
    mean = rng.lognormal(0.0, 1.5, (rows, width)).astype(np.float32)
    M = np.zeros((rows, width, 4), np.float32)
    M[..., 0] = mean * cnt
    M[..., 1] = mean * mean * (1 + rng.uniform(0, 2, (rows, width))).astype(np.float32) * cnt
    M[..., 3] = cnt
    k = rng.integers(0, rows * width, 20)
    y, x = k // width, k % width
    for i, wv in enumerate([0.0, 1e-40, 1.0, 3.0, 4.0, 5.0, np.nan, np.inf, -0.0, -3.0]):
        M[y[i], x[i], 3] = f32(wv)
        if i in (2, 3, 4, 5):
            M[y[i], x[i], :2] = (f32(2.0) * f32(wv), f32(4.5) * f32(wv))
    M[y[10], x[10]] = (8.0, 12.0, 0.0, 4.0)     # mu1 = 2, mu2 = 3 < mu1^2: the temporal estimate clamps to 0
    M[y[11], x[11]] = (3.0, 1.0, 0.0, 1.0)      # the same on the spatial branch
    M[y[12], x[12], 0] = np.nan
    M[y[13], x[13], 1] = np.inf
    M[y[14], x[14], 0] = -np.inf
    M[y[15], x[15], :2] = f32(1e-40)
    M[y[16], x[16], 1] = f32(3e38)
    M[y[17], x[17]] = (3e38, 3e38, 0.0, 5.0)    # mu1^2 overflows
    return acc, M, N, A


# ---- M through the two reprojections (include/glrtx.h "Variance guidance": "Carrying M")
def _moments_as_accumulator(accum, moments):
    """The carry of M is steps 5-7 of "Reprojection" read with other names: over the taps that count, sm / smc / s1 / s2 are sw / sc / sI.r / sI.g of an
    accumulator {M.x, M.y, 0, M.w}, and nm and the output follow from them as n and out do.  A tap counts for M if it counts for the accumulator (acc.w neither
    a zero nor a denormal, the other tests do not read the accumulator) and M.w is neither: an M.w of 0 where acc.w is tiny says both."""
    acc, M = np.asarray(accum, np.float32), np.asarray(moments, np.float32)
    A = np.zeros_like(M)
    A[..., 0], A[..., 1] = M[..., 0], M[..., 1]
    A[..., 3] = np.where(tiny(acc[..., 3]), f32(0), M[..., 3])
    return A


def _carried_moments(out, mo):
    mo = mo.copy()
    mo[..., 2] = 0
    mo[out[..., 3] == 0] = 0  # a pixel with no accumulator history has no moments either (a carried count is >= 1)
    return mo


def reproject_moments(accum, moments, n0, a0, n1, a1, W, S, o_prev, cur, max_history, depth_tolerance, normal_tolerance):
    """reproject_math.reproject with the old view's M: returns (out, moments_out, carried, hit_pixels)."""
    import reproject_math as rm
    rest = (n0, a0, n1, a1, W, S, o_prev, cur, max_history, depth_tolerance, normal_tolerance)
    out, carried, hits = rm.reproject(accum, *rest)
    mo, _, _ = rm.reproject(_moments_as_accumulator(accum, moments), *rest)
    return out, _carried_moments(out, mo), carried, hits


def reproject_motion_moments(accum, moments, n0, a0, g1, a1, vert_prev, tri, W, S, o_prev, max_history, depth_tolerance, normal_tolerance):
    """reproject_motion_math.reproject_motion with the old view's M: returns (out, moments_out, carried, hit_pixels)."""
    import reproject_motion_math as mm
    rest = (n0, a0, g1, a1, vert_prev, tri, W, S, o_prev, max_history, depth_tolerance, normal_tolerance)
    out, carried, hits = mm.reproject_motion(accum, *rest)
    mo, _, _ = mm.reproject_motion(_moments_as_accumulator(accum, moments), *rest)
    return out, _carried_moments(out, mo), carried, hits


def hostile_moments(accum, seed):
    """An M plane for a hostile accumulator of any shape: hostile_arrays' M.w values and moments, at that shape."""
    rows, width = np.asarray(accum).shape[:2]
    return hostile_arrays(rows, width, seed)[1]
