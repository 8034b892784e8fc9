"""numpy statement of the temporal reprojection (include/glrtx.h "Reprojection"; csrc/reproject.hip.h; host/reproject.cpp).

Every operation is one IEEE float32 operation, correctly rounded, in the kernel's order.  Denormals count as zeros of their sign on the way into and out of
every operation (ftz), and a NaN that is STORED is 0x7FC00000.  The inverses of the previous camera's matrices are INPUTS (W, S): what is stated here is fp32
arithmetic only; the tests form them with glrt_mat4_inverse, the routine both libraries compile.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import _op, ftz
from denoise_math import add, canon, centre_rays, div, mul, sub, tiny

f32 = np.float32
MIN_WEIGHT = f32(1e-6)


def pos_finite(x):
    """Sign bit clear, exponent field neither 0 nor 255."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return (b - np.uint32(0x00800000)) < np.uint32(0x7F000000)


def origin(c2w):
    """centre_ray's origin for a camera: (C[k] * 0 + C[12 + k]) + C[4 + k] * 0 per row, divided by the w row."""
    C = np.asarray(c2w, np.float32).reshape(16)
    w = [add(add(mul(C[k], f32(0)), C[12 + k]), mul(C[4 + k], f32(0))) for k in range(4)]
    return np.array([div(w[k], w[3]) for k in range(3)], np.float32)


def reproject(accum, n0, a0, n1, a1, W, S, o_prev, cur, max_history, depth_tolerance, normal_tolerance):
    """accum, n0, a0: the old view; n1, a1: the new view's planes; all (rows, width, 4) float32.  W, S: inverse(c2w_prev), inverse(s2c_prev); o_prev: origin(c2w_prev);
    cur: the new camera (c2w, s2c).  Returns (out, carried, hit_pixels)."""
    acc, N0, A0, N1, A1 = (np.ascontiguousarray(v, np.float32) for v in (accum, n0, a0, n1, a1))
    rows, width = acc.shape[:2]
    W, S = np.asarray(W, np.float32).reshape(16), np.asarray(S, np.float32).reshape(16)
    o_prev = np.asarray(o_prev, np.float32)
    mh, dt, nt = f32(max_history), ftz(f32(depth_tolerance)), ftz(f32(normal_tolerance))
    id1 = A1[..., 3].view(np.int32)
    id0 = A0[..., 3].view(np.int32)
    t = N1[..., 3]
    hit = id1 >= 0
    live = hit & pos_finite(t)
    ray = centre_rays(cur, width, rows).reshape(rows, width, 8)
    P = [add(ray[..., k], mul(t, ray[..., 4 + k])) for k in range(3)]
    q = [add(add(add(mul(W[k], P[0]), mul(W[4 + k], P[1])), mul(W[8 + k], P[2])), W[12 + k]) for k in range(4)]
    s = {k: add(add(add(mul(S[k], q[0]), mul(S[4 + k], q[1])), mul(S[8 + k], q[2])), mul(S[12 + k], q[3])) for k in (0, 1, 3)}
    Wf, Hf = f32(width), f32(rows)
    u = add(mul(mul(add(div(s[0], s[3]), f32(1)), f32(0.5)), Wf), f32(-1))
    v = add(mul(mul(add(div(s[1], s[3]), f32(1)), f32(0.5)), Hf), f32(-1))
    with np.errstate(invalid="ignore"):
        live &= pos_finite(s[3]) & (u >= f32(-1)) & (u < Wf) & (v >= f32(-1)) & (v < Hf)
    u, v = np.where(live, u, f32(0)), np.where(live, v, f32(0))  # (dead pixels: any in-range value, masked out below)
    d = [sub(P[k], o_prev[k]) for k in range(3)]
    e = _op(np.sqrt, add(add(mul(d[2], d[2]), mul(d[1], d[1])), mul(d[0], d[0])))
    lim = mul(dt, e)
    fx0, fy0 = np.floor(u).astype(np.float32), np.floor(v).astype(np.float32)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    fx, fy = sub(u, fx0), sub(v, fy0)
    wx, wy = (sub(f32(1), fx), fx), (sub(f32(1), fy), fy)
    sw = np.zeros((rows, width), np.float32)
    sc = np.zeros((rows, width), np.float32)
    sI = np.zeros((rows, width, 3), np.float32)
    for j in range(2):
        for i in range(2):
            tx, ty = x0 + i, y0 + j
            inside = (tx >= 0) & (tx < width) & (ty >= 0) & (ty < rows)
            cx, cy = np.clip(tx, 0, width - 1), np.clip(ty, 0, rows - 1)
            C, n0q = acc[cy, cx], N0[cy, cx]
            dot = add(add(mul(N1[..., 2], n0q[..., 2]), mul(N1[..., 1], n0q[..., 1])), mul(N1[..., 0], n0q[..., 0]))
            with np.errstate(invalid="ignore"):
                ok = live & inside & (id0[cy, cx] == id1) & ~tiny(C[..., 3]) & (dot >= nt) & (np.abs(sub(n0q[..., 3], e)) <= lim)
            w = mul(wx[i], wy[j])
            sw = np.where(ok, add(sw, w), sw)
            sc = np.where(ok, add(sc, mul(w, C[..., 3])), sc)
            sI = np.where(ok[..., None], add(sI, mul(w[..., None], div(C[..., :3], C[..., 3:4]))), sI)
    with np.errstate(invalid="ignore"):
        r = np.rint(div(sc, sw)).astype(np.float32)
        n = np.where(r > mh, mh, r).astype(np.float32)
        carried = live & (sw > MIN_WEIGHT) & (n >= f32(1))
    out = np.zeros((rows, width, 4), np.float32)
    out[..., :3] = canon(mul(div(sI, sw[..., None]), n[..., None]))
    out[..., 3] = n
    out[~carried] = 0
    return out, int(carried.sum()), int(hit.sum())


def move_camera(params, kind, amount):
    """A camera moved from params' (c2w column-major float32[16]): 'pan' turns it by `amount` degrees about its own up axis, 'dolly' moves it `amount` units
    along its viewing direction, 'orbit' turns it by `amount` degrees about the world's y axis through the origin.  Returns params with the new c2w."""
    C = np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    a = np.deg2rad(amount)
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    if kind == "pan":
        M = C @ R
    elif kind == "orbit":
        M = R @ C
    elif kind == "dolly":
        T = np.eye(4)
        T[2, 3] = -amount
        M = C @ T
    else:
        raise ValueError(kind)
    return dict(params, c2w=np.ascontiguousarray(M.T.reshape(16), np.float32))


def hostile_arrays(rows, width, seed):
    """Old and new views for the bit-for-bit comparisons of the three statements: tests/denoise_math.py's hostile accumulator and planes as the old view (NaN, Inf,
    zero, negative and denormal counts, reserved ids, NaN normals, misses), and as the new view's planes a copy of them with depths that fit a plane in front of
    the camera -- so that many taps pass the tests -- plus hostile depths, ids and normals of its own.  Returns (accum, N0, A0, N1, A1)."""
    from denoise_math import NO_PIXEL, hostile_arrays as dn_hostile
    acc, N0, A0 = dn_hostile(rows, width, seed)
    rng = np.random.default_rng(seed + 1)
    N1, A1 = N0.copy(), A0.copy()
    k = rng.integers(0, rows * width, 16)
    y, x = k // width, k % width
    N1[y[0], x[0], 3] = np.nan
    N1[y[1], x[1], 3] = np.inf
    N1[y[2], x[2], 3] = f32(1e-40)
    N1[y[3], x[3], 3] = f32(-3.0)
    N1[y[4], x[4], 3] = f32(0.0)
    N1[y[5], x[5], 3] = f32(3e38)
    N1[y[6], x[6], 1] = np.nan
    N1[y[7], x[7], 0] = np.inf
    ids = A1[..., 3].view(np.int32).copy()
    ids[y[8], x[8]] = NO_PIXEL
    ids[y[9], x[9]] = -1
    ids[y[10], x[10]] = 2 ** 31 - 1
    A1[..., 3] = ids.view(np.float32)
    return acc, N0, A0, N1, A1
