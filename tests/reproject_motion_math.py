"""numpy statement of the reprojection across a geometry move (include/glrtx.h "Reprojection across a geometry move"; csrc/reproject_motion.hip.h;
host/reproject_motion.cpp).

tests/reproject_math.py's rules hold: every operation is one IEEE float32 operation, correctly rounded, in the kernel's order, denormals count as zeros of
their sign on the way into and out of every operation (ftz), a NaN that is STORED is 0x7FC00000, and W, S, o_prev are inputs.  One exception, as in the
contract: the previous triangles' edges p1 - p0 and p2 - p0 are formed with denormals KEPT (the scene upload's subtraction), and flushed only when the
per-pixel arithmetic reads them.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import _op, ftz
from denoise_math import add, canon, div, mul, sub, tiny
from reproject_math import MIN_WEIGHT, pos_finite

f32 = np.float32


def previous_records(vert_prev, tri):
    """Per wire triangle: p0, e1, e2 (n, 3) and the three vertex normals (n, 3, 3).  The edges are plain IEEE subtractions, denormals kept."""
    vert = np.ascontiguousarray(vert_prev, np.float32).reshape(-1, 15)
    tr = np.ascontiguousarray(tri, np.float32).reshape(-1, 4)
    idx = tr[:, :3].astype(np.int64)
    p = vert[idx, 0:3]  # (n, 3 corners, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        e1, e2 = (p[:, 1] - p[:, 0]).astype(np.float32), (p[:, 2] - p[:, 0]).astype(np.float32)
    return p[:, 0], e1, e2, vert[idx, 3:6]


def reproject_motion(accum, n0, a0, g1, a1, vert_prev, tri, W, S, o_prev, max_history, depth_tolerance, normal_tolerance):
    """accum, n0, a0: the old view; g1, a1: the new view's geometry and albedo planes; all (rows, width, 4) float32.  vert_prev: the vertices as they stood at
    the old view; tri: the wire triangles.  W, S: inverse(c2w_prev), inverse(s2c_prev); o_prev: origin(c2w_prev).  Returns (out, carried, hit_pixels)."""
    acc, N0, A0, G1, A1 = (np.ascontiguousarray(v, np.float32) for v in (accum, n0, a0, g1, a1))
    rows, width = acc.shape[:2]
    W, S = np.asarray(W, np.float32).reshape(16), np.asarray(S, np.float32).reshape(16)
    o_prev = np.asarray(o_prev, np.float32)
    mh, dt, nt = f32(max_history), ftz(f32(depth_tolerance)), ftz(f32(normal_tolerance))
    p0, e1, e2, nr = previous_records(vert_prev, tri)
    n_tri = p0.shape[0]
    id1 = A1[..., 3].view(np.int32)
    id0 = A0[..., 3].view(np.int32)
    t1 = G1[..., 0].view(np.int32)
    hit = id1 >= 0
    live = hit & (t1 >= 0) & (t1 < n_tri)
    k = np.where(live, t1, 0) if n_tri else np.zeros_like(t1)
    if n_tri == 0:
        return np.zeros((rows, width, 4), np.float32), 0, int(hit.sum())
    u, v = G1[..., 1], G1[..., 2]
    # 2'  the point and the normal the old view should have seen
    P = [add(add(p0[k, c], mul(u, e1[k, c])), mul(v, e2[k, c])) for c in range(3)]
    w0 = sub(sub(f32(1), u), v)
    tv = [add(add(mul(w0, nr[k, 0, c]), mul(u, nr[k, 1, c])), mul(v, nr[k, 2, c])) for c in range(3)]
    rn = div(f32(1), _op(np.sqrt, add(add(mul(tv[2], tv[2]), mul(tv[1], tv[1])), mul(tv[0], tv[0]))))
    m = [mul(tv[c], rn) for c in range(3)]
    # 3, 4
    q = [add(add(add(mul(W[c], P[0]), mul(W[4 + c], P[1])), mul(W[8 + c], P[2])), W[12 + c]) for c in range(4)]
    s = {c: add(add(add(mul(S[c], q[0]), mul(S[4 + c], q[1])), mul(S[8 + c], q[2])), mul(S[12 + c], q[3])) for c in (0, 1, 3)}
    Wf, Hf = f32(width), f32(rows)
    ui = add(mul(mul(add(div(s[0], s[3]), f32(1)), f32(0.5)), Wf), f32(-1))
    vi = add(mul(mul(add(div(s[1], s[3]), f32(1)), f32(0.5)), Hf), f32(-1))
    with np.errstate(invalid="ignore"):
        live &= pos_finite(s[3]) & (ui >= f32(-1)) & (ui < Wf) & (vi >= f32(-1)) & (vi < Hf)
    ui, vi = np.where(live, ui, f32(0)), np.where(live, vi, f32(0))  # (dead pixels: any in-range value, masked out below)
    d = [sub(P[c], o_prev[c]) for c in range(3)]
    e = _op(np.sqrt, add(add(mul(d[2], d[2]), mul(d[1], d[1])), mul(d[0], d[0])))
    lim = mul(dt, e)
    # 5 .. 7
    fx0, fy0 = np.floor(ui).astype(np.float32), np.floor(vi).astype(np.float32)
    x0, y0 = fx0.astype(np.int64), fy0.astype(np.int64)
    fx, fy = sub(ui, fx0), sub(vi, fy0)
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
            dot = add(add(mul(m[2], n0q[..., 2]), mul(m[1], n0q[..., 1])), mul(m[0], n0q[..., 0]))
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


def rotate_vertices(vert, degrees):
    """Every vertex's position and normal turned by `degrees` about the world's y axis through the origin (reproject_math.move_camera's 'orbit' matrix), in
    float64, rounded once to float32.  Returns (n, 15) float32."""
    v = np.array(np.asarray(vert, np.float32).reshape(-1, 15), np.float64)
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    v[:, 0:3] = v[:, 0:3] @ R.T
    v[:, 3:6] = v[:, 3:6] @ R.T
    return np.ascontiguousarray(v, np.float32)


def vertices_of_material(scene, material):
    """The indices of the vertices that triangles of `material` use (and no triangle of another material: asserted)."""
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    own = tri[:, 3].astype(np.int64) == material
    idx = np.unique(tri[own, :3].astype(np.int64))
    assert idx.size and not np.isin(tri[~own, :3].astype(np.int64), idx).any()
    return idx


def hostile_arrays(rows, width, seed):
    """reproject_math.hostile_arrays' old view and albedo plane, a geometry plane G1 that puts most pixels on a plane of triangles in front of the camera at the
    hostile depths (so that many taps pass), and previous vertices with hostile records: triangle indices out of range on both sides, NaN / Inf / denormal
    barycentrics, triangles with zero edges, denormal edges, NaN and zero normals, NaN and Inf positions.  Needs the camera of scenes.config_c1(width, rows):
    the triangles lie where that camera's centre rays reach the depths of N0.  Returns (accum, N0, A0, G1, A1, vert_prev, tri)."""
    import reproject_math as rm
    from denoise_math import centre_rays
    from glrt_amd import scenes
    acc, N0, A0, _, A1 = rm.hostile_arrays(rows, width, seed)
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    rng = np.random.default_rng(seed + 2)
    ray = centre_rays(params, width, rows).reshape(rows, width, 8).astype(np.float64)
    t = np.where(np.isfinite(N0[..., 3]) & (N0[..., 3] > 0), N0[..., 3], 3.0).astype(np.float64)
    P = ray[..., 0:3] + t[..., None] * ray[..., 4:7]
    # a triangle per pixel around its point, the point at barycentrics (u, v); normals the old view's, slightly turned per corner
    u, v = rng.uniform(0.05, 0.45, (rows, width)), rng.uniform(0.05, 0.45, (rows, width))
    e1, e2 = rng.normal(size=(rows, width, 3)) * 0.1, rng.normal(size=(rows, width, 3)) * 0.1
    p0 = P - u[..., None] * e1 - v[..., None] * e2
    n_px = rows * width
    vert = np.zeros((3 * n_px + 12, 15), np.float32)
    vert[0:3 * n_px:3, 0:3] = p0.reshape(-1, 3)
    vert[1:3 * n_px:3, 0:3] = (p0 + e1).reshape(-1, 3)
    vert[2:3 * n_px:3, 0:3] = (p0 + e2).reshape(-1, 3)
    for c in range(3):
        vert[c:3 * n_px:3, 3:6] = (N0[..., :3] + rng.normal(size=(rows, width, 3)) * 0.05).reshape(-1, 3)
    tri = np.zeros((n_px + 6, 4), np.float32)
    tri[:n_px, 0:3] = 3 * np.arange(n_px)[:, None] + np.arange(3)
    b = 3 * n_px
    vert[b + 0, 0:3] = vert[b + 1, 0:3] = vert[b + 2, 0:3] = (0.0, 0.0, -3.0)        # zero edges
    vert[b:b + 3, 3:6] = (0.0, 0.0, 1.0)
    vert[b + 3:b + 6, 0:3] = [(0, 0, -3), (1e-40, 0, -3), (0, 1e-39, -3)]             # denormal edges
    vert[b + 3:b + 6, 3:6] = 0.0                                                      # a zero normal: rsq(0) = inf, 0 * inf = NaN
    vert[b + 6:b + 9, 0:3] = [(0, 0, -3), (np.nan, 0, -3), (0, np.inf, -3)]
    vert[b + 6:b + 9, 3:6] = (0.0, 1.0, 0.0)
    vert[b + 9:b + 12, 0:3] = [(0, 0, -3), (1, 0, -3), (0, 1, -3)]
    vert[b + 9:b + 12, 3:6] = [(np.nan, 0, 1), (0, np.inf, 1), (0, 0, 1e-40)]          # NaN / Inf / denormal normals
    for j in range(4):
        tri[n_px + j, 0:3] = b + 3 * j + np.arange(3)
    tri[n_px + 4, 0:3] = (b, b, b)          # one vertex three times
    tri[n_px + 5, 0:3] = (0, 4, 8)          # corners far apart
    G1 = np.zeros((rows, width, 4), np.float32)
    ids = np.arange(n_px, dtype=np.int32).reshape(rows, width).copy()
    G1[..., 1], G1[..., 2] = u, v
    k = rng.integers(0, n_px, 24)
    y, x = k // width, k % width
    for j in range(6):
        ids[y[j], x[j]] = n_px + j
    ids[y[6], x[6]] = n_px + 6               # the first index past the triangles
    ids[y[7], x[7]] = 2 ** 31 - 1
    ids[y[8], x[8]] = -1
    ids[y[9], x[9]] = -(2 ** 31)
    G1[y[10], x[10], 1] = np.nan
    G1[y[11], x[11], 2] = np.inf
    G1[y[12], x[12], 1] = f32(1e-40)
    G1[y[13], x[13], 2] = f32(-0.25)
    G1[y[14], x[14], 1] = f32(3e38)
    G1[y[15], x[15], 1:3] = 0.0
    G1[y[16], x[16], 3] = np.nan             # (the fourth word is not read)
    ids[A1[..., 3].view(np.int32) < 0] = -1  # misses of the albedo plane are misses here (a few hostile ids above stay as they are)
    G1[..., 0] = ids.view(np.float32)
    return acc, N0, A0, G1, A1, vert, tri
