"""numpy statement of the denoiser (include/glrtx.h "Denoising"; csrc/features.hip.h, csrc/denoise.hip.h; host/features.cpp, host/denoise.cpp).

Every operation is one IEEE float32 operation, correctly rounded, in the kernel's order; lp_exp (tests/volume_math.py) carries the only fused
operations.  Denormals count as zeros of their sign on the way into and out of every operation (ftz), and a NaN that is STORED is 0x7FC00000.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import _op, ftz
from volume_math import lp_exp

f32 = np.float32
NO_PIXEL = np.int32(-2 ** 31)  # the reserved id: a pixel without samples
ALBEDO_FLOOR = f32(1e-3)
KERN = (np.array([1, 4, 6, 4, 1], np.float32) / f32(16)).astype(np.float32)
EPS, INFTY = f32(1e-4), f32(1e8)


def add(a, b): return _op(np.add, a, b)
def sub(a, b): return _op(np.subtract, a, b)
def mul(a, b): return _op(np.multiply, a, b)
def div(a, b): return _op(np.divide, a, b)


def canon(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isnan(x), np.array([0x7FC00000], np.uint32).view(np.float32)[0], x).astype(np.float32)


def tiny(x):
    return (np.asarray(x, np.float32).view(np.uint32) & np.uint32(0x7F800000)) == 0


def fmax_c(x, c):
    x = ftz(x)
    with np.errstate(invalid="ignore"):
        return np.where(x > c, x, c).astype(np.float32)


def atrous(accum, normal_depth, albedo_id, iterations, sigma_color, sigma_normal, sigma_depth, demodulate):
    """accum, normal_depth, albedo_id: (rows, width, 4) float32 (albedo_id[..., 3] holds int32 bits).  Returns D, (rows, width, 4) float32."""
    acc = np.ascontiguousarray(accum, np.float32)
    g = np.ascontiguousarray(normal_depth, np.float32)
    al = np.ascontiguousarray(albedo_id, np.float32)
    rows, width = acc.shape[:2]
    ids = al[..., 3].view(np.int32).copy()
    dead = tiny(acc[..., 3]) | (ids == NO_PIXEL)
    ids[dead] = NO_PIXEL
    alb = fmax_c(al[..., :3], ALBEDO_FLOOR)
    c = div(acc[..., :3], acc[..., 3:4])
    if demodulate:
        c = div(c, alb)
    c = canon(np.where(dead[..., None], f32(0), c))
    sn, sd = f32(sigma_normal), f32(sigma_depth)
    tden = fmax_c(g[..., 3], f32(1e-6))
    for it in range(iterations):
        sp = 1 << it
        sc = ftz(f32(sigma_color) * f32(2.0 ** (-2 * it)))
        sw = np.zeros((rows, width), np.float32)
        s = np.zeros((rows, width, 3), np.float32)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                oy, ox = sp * dy, sp * dx
                # centre window [y0, y1) x [x0, x1) whose tap (y + oy, x + ox) lies inside the image
                y0, y1 = max(0, -oy), min(rows, rows - oy)
                x0, x1 = max(0, -ox), min(width, width - ox)
                if y0 >= y1 or x0 >= x1:
                    continue
                P = (slice(y0, y1), slice(x0, x1))
                Q = (slice(y0 + oy, y1 + oy), slice(x0 + ox, x1 + ox))
                ok = (ids[Q] == ids[P]) & ~dead[P]
                d = sub(c[Q], c[P])
                dc = add(add(mul(d[..., 0], d[..., 0]), mul(d[..., 1], d[..., 1])), mul(d[..., 2], d[..., 2]))
                n = sub(g[Q][..., :3], g[P][..., :3])
                dn = add(add(mul(n[..., 0], n[..., 0]), mul(n[..., 1], n[..., 1])), mul(n[..., 2], n[..., 2]))
                rt = div(sub(g[Q][..., 3], g[P][..., 3]), tden[P])
                dd = div(mul(rt, rt), sd)
                with np.errstate(invalid="ignore"):
                    dd = np.where(dd < f32(80), dd, f32(80)).astype(np.float32)
                e = add(add(div(dc, sc), div(dn, sn)), dd)
                w = mul(mul(KERN[dy + 2], KERN[dx + 2]), ftz(lp_exp(-e)))
                sw[P] = np.where(ok, add(sw[P], w), sw[P])
                s[P] = np.where(ok[..., None], add(s[P], mul(w[..., None], c[Q])), s[P])
        den = fmax_c(sw, f32(1e-20))
        c = canon(np.where(dead[..., None], f32(0), div(s, den[..., None])))
    out = np.ones((rows, width, 4), np.float32)
    if demodulate:
        c = np.where(dead[..., None], c, canon(mul(c, alb)))
    out[..., :3] = c
    return out


def centre_rays(params, width, height, rows_y=None):
    """The feature pass's rays: camera_ray (csrc/pt_kernel.hip.h) with r0 = r1 = 0.5 and no thin lens, in float32, for the image rows rows_y
    (default: all).  (n, 8) {o, tmin = 1e-4, d, tmax = 1e8}, row-major."""
    C = np.asarray(params["c2w"], np.float32).reshape(16)
    S = np.asarray(params["s2c"], np.float32).reshape(16)
    ys = np.arange(height) if rows_y is None else np.asarray(rows_y)
    y, x = np.meshgrid(ys, np.arange(width), indexing="ij")
    fcx, fcy = add(x.astype(np.float32), f32(0.5)), add(y.astype(np.float32), f32(0.5))
    nx = add(mul(div(add(fcx, f32(0.5)), f32(width)), f32(2)), f32(-1))
    ny = add(mul(div(add(fcy, f32(0.5)), f32(height)), f32(2)), f32(-1))
    t = [add(add(mul(S[k], nx), S[12 + k]), mul(S[4 + k], ny)) for k in range(4)]
    cx, cy, cz = div(t[0], t[3]), div(t[1], t[3]), div(t[2], t[3])
    rn = div(f32(1), _op(np.sqrt, add(add(mul(cz, cz), mul(cy, cy)), mul(cx, cx))))
    dx, dy, dz = mul(cx, rn), mul(cy, rn), mul(cz, rn)
    z = f32(0)
    w = [add(add(mul(C[k], z), C[12 + k]), mul(C[4 + k], z)) for k in range(4)]
    e = [add(add(mul(C[k], dx), mul(C[4 + k], dy)), mul(C[8 + k], dz)) for k in range(3)]
    re = div(f32(1), _op(np.sqrt, add(add(mul(e[2], e[2]), mul(e[1], e[1])), mul(e[0], e[0]))))
    r = np.zeros((ys.size, width, 8), np.float32)
    for k in range(3):
        r[..., k] = div(w[k], w[3])
        r[..., 4 + k] = mul(e[k], re)
    r[..., 3] = EPS
    r[..., 7] = INFTY
    return r.reshape(-1, 8)


def features_from_hits(scene, hits, rows, width):
    """The two planes from glrt_trace_rays' hits of centre_rays: surf_tri's normal, t, albedo and material id."""
    t, tri_i, u, v = hits
    vert = np.asarray(scene["vert"], np.float32).reshape(-1, 15)
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    mat = np.asarray(scene["mat"], np.float32).reshape(-1, 18)
    hit = tri_i >= 0
    k = np.where(hit, tri_i, 0)
    idx = tri[k, :3].astype(np.int64)
    n0, n1, n2 = vert[idx[:, 0], 3:6], vert[idx[:, 1], 3:6], vert[idx[:, 2], 3:6]
    w0 = sub(sub(f32(1), u), v)[:, None]
    tv = add(add(mul(w0, n0), mul(u[:, None], n1)), mul(v[:, None], n2))
    r = div(f32(1), _op(np.sqrt, add(add(mul(tv[:, 2], tv[:, 2]), mul(tv[:, 1], tv[:, 1])), mul(tv[:, 0], tv[:, 0]))))
    N = np.zeros((hits[0].size, 4), np.float32)
    N[:, :3] = canon(mul(tv, r[:, None]))
    N[:, 3] = t
    N[~hit] = 0
    m = tri[k, 3].astype(np.int32)
    A = np.ones((hits[0].size, 4), np.float32)
    diffuse = hit & (mat[m, 0].astype(np.int32) == 2)
    A[diffuse, :3] = mat[m[diffuse], 6:9]
    A[:, 3] = np.where(hit, m, np.int32(-1)).astype(np.int32).view(np.float32)
    return N.reshape(rows, width, 4), A.reshape(rows, width, 4)


def hostile_arrays(rows, width, seed):
    """A random HDR accumulator with NaN, Inf, zero-count, denormal and reserved-id pixels, and feature planes with three materials, misses, depth steps and
    a few NaN normals: inputs for the bit-for-bit comparisons of the three statements of the filter."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(0, 5, (rows, width)).astype(np.float32)
    acc = np.zeros((rows, width, 4), np.float32)
    acc[..., :3] = (rng.lognormal(0.0, 2.5, (rows, width, 3)) * cnt[..., None]).astype(np.float32)
    acc[..., 3] = cnt
    n = rng.normal(size=(rows, width, 3))
    n = np.where(rng.uniform(size=(rows, width, 1)) < 0.6, np.array([0.0, 0.0, 1.0]), n / np.linalg.norm(n, axis=2, keepdims=True))
    N = np.zeros((rows, width, 4), np.float32)
    N[..., :3] = n
    N[..., 3] = np.where(rng.uniform(size=(rows, width)) < 0.5, 3.0, 3.0 + rng.uniform(0, 2, (rows, width))) + 0.01 * np.arange(width)
    ids = rng.integers(-1, 3, (rows, width)).astype(np.int32)
    ids[rows // 2:, : width // 2] = 1  # one larger region of one material
    A = np.ones((rows, width, 4), np.float32)
    A[..., :3] = rng.uniform(0, 1, (rows, width, 3))
    A[ids < 0, :3] = 1
    N[ids < 0] = 0
    k = rng.integers(0, rows * width, 24)
    y, x = k // width, k % width
    acc[y[0], x[0], 0] = np.nan
    acc[y[1], x[1], 1] = np.inf
    acc[y[2], x[2], 2] = -np.inf
    acc[y[3], x[3], 3] = np.nan
    acc[y[4], x[4], 3] = np.inf
    acc[y[5], x[5], 3] = f32(1e-40)       # a denormal count: dead
    acc[y[6], x[6], :3] = f32(1e-40)      # denormal sums
    acc[y[7], x[7], 3] = f32(-0.0)
    acc[y[8], x[8], :3] = f32(3e38)
    acc[y[9], x[9], 3] = f32(-2.0)
    N[y[10], x[10], 0] = np.nan
    N[y[11], x[11], 3] = np.inf
    N[y[12], x[12], 3] = f32(1e-40)
    N[y[13], x[13], 3] = np.nan
    A[y[14], x[14], 0] = f32(0.0)
    A[y[15], x[15], 1] = f32(1e-40)
    A[y[16], x[16], 2] = np.nan
    A[y[17], x[17], 0] = np.inf
    ids[y[18], x[18]] = NO_PIXEL
    ids[y[19], x[19]] = 2 ** 31 - 1
    A[..., 3] = ids.view(np.float32)
    return acc, N, A
