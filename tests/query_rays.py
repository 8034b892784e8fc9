"""Ray sets and a brute-force statement for the ray-query tests (glrt_trace_rays / glrtx_trace_rays)."""
import numpy as np

F32 = np.float32


def _pos(scene):
    return np.asarray(scene["vert"], F32).reshape(-1, 15)[:, :3]


def _tris(scene):
    t = np.asarray(scene["tri"], F32).reshape(-1, 4)[:, :3].astype(np.int64)
    p = _pos(scene)
    return p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]


def pack(o, d, tmin, tmax):
    n = o.shape[0]
    r = np.zeros((n, 8), F32)
    r[:, 0:3] = o
    r[:, 3] = tmin
    r[:, 4:7] = d
    r[:, 7] = tmax
    return r


def camera_rays(params, width=None, height=None, tmin=1e-4, tmax=1e8):
    """Pinhole rays through pixel centres, from the renderer's camera matrices (c2w, s2c: column-major float[16])."""
    w = width or params["width"]
    h = height or params["height"]
    c2w = np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    s2c = np.asarray(params["s2c"], np.float64).reshape(4, 4).T
    y, x = np.mgrid[0:h, 0:w]
    ndc = np.stack([(x.ravel() + 0.5) / w * 2 - 1, (y.ravel() + 0.5) / h * 2 - 1, np.ones(w * h), np.ones(w * h)], 1)
    p = ndc @ s2c.T
    p = p[:, :3] / p[:, 3:4]
    d = p @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return pack(o.astype(F32), d.astype(F32), tmin, tmax)


def surface_points(scene, n, rng):
    v0, v1, v2 = _tris(scene)
    k = rng.integers(0, v0.shape[0], n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    p = v0[k] + a[:, None] * (v1[k] - v0[k]) + b[:, None] * (v2[k] - v0[k])
    nrm = np.cross(v1[k] - v0[k], v2[k] - v0[k]).astype(np.float64)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-30), np.array([0.0, 0.0, 1.0]))
    return p.astype(F32), nrm


def incoherent_rays(scene, n, seed=1, tmin=1e-4, tmax=1e8):
    """Cosine-distributed directions about the surface normal (either side at random), from random points on the surfaces."""
    rng = np.random.default_rng(seed)
    p, nrm = surface_points(scene, n, rng)
    nrm = nrm * np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)[:, None]
    u1, u2 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1 - u1))], 1)
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(a, nrm)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    d = local[:, :1] * t + local[:, 1:2] * b + local[:, 2:3] * nrm
    return pack(p, d.astype(F32), tmin, tmax)


def shadow_rays(scene, n, seed=2):
    """From random surface points to random points on the light triangles (all triangles when the scene has none): direction = the unnormalised
    difference, tmin = 1e-4, tmax = 1 - 1e-4."""
    rng = np.random.default_rng(seed)
    p, _ = surface_points(scene, n, rng)
    light = np.asarray(scene["light"], F32).reshape(-1, 4)
    pos = _pos(scene)
    if light.shape[0]:
        lt = light[:, :3].astype(np.int64)
        k = rng.integers(0, lt.shape[0], n)
        l0, l1, l2 = pos[lt[k, 0]], pos[lt[k, 1]], pos[lt[k, 2]]
    else:
        v0, v1, v2 = _tris(scene)
        k = rng.integers(0, v0.shape[0], n)
        l0, l1, l2 = v0[k], v1[k], v2[k]
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    q = (l0 + a[:, None] * (l1 - l0) + b[:, None] * (l2 - l0)).astype(F32)
    return pack(p, (q - p).astype(F32), 1e-4, 1.0 - 1e-4)


def special_rays():
    """Rays that need no search: NaN / infinite components, zero directions, tmax <= tmin; plus a denormal tmin."""
    nan, inf = F32(np.nan), F32(np.inf)
    rows = []
    base = [0.0, 0.0, 5.0, 1e-4, 0.0, 0.0, -1.0, 1e8]
    for i in range(8):
        for bad in (nan, inf, -inf):
            r = list(base)
            r[i] = bad
            rows.append(r)
    rows.append([0.0, 0.0, 5.0, 1e-4, 0.0, 0.0, 0.0, 1e8])       # zero direction
    rows.append([0.0, 0.0, 5.0, 1e-4, -0.0, 0.0, -0.0, 1e8])     # signed zeros
    rows.append([0.0, 0.0, 5.0, 2.0, 0.0, 0.0, -1.0, 2.0])       # tmax == tmin
    rows.append([0.0, 0.0, 5.0, 3.0, 0.0, 0.0, -1.0, 1.0])       # tmax < tmin
    rows.append([0.0, 0.0, 5.0, -1e8, 0.0, 0.0, -1.0, -2e8])     # both negative, reversed
    return np.asarray(rows, F32)


def brute_force(scene, rays):
    """Every triangle against every ray, in float32 with the device's operation order and no fused multiply-adds.  Returns (hit mask (n, T), t (n, T),
    u, v): hit[i, k] when triangle k passes the renderer's test with tmin < t < tmax."""
    v0, v1, v2 = _tris(scene)
    e1, e2 = (v1 - v0).astype(F32), (v2 - v0).astype(F32)
    o, d = rays[:, None, 0:3], rays[:, None, 4:7]
    tmin, tmax = rays[:, 3:4], rays[:, 7:8]

    def dot3(a, b):
        return (a[..., 2] * b[..., 2] + a[..., 1] * b[..., 1]) + a[..., 0] * b[..., 0]

    with np.errstate(all="ignore"):
        px = d[..., 1] * e2[None, :, 2] - d[..., 2] * e2[None, :, 1]
        py = d[..., 2] * e2[None, :, 0] - d[..., 0] * e2[None, :, 2]
        pz = d[..., 0] * e2[None, :, 1] - d[..., 1] * e2[None, :, 0]
        p = np.stack([px, py, pz], -1)
        det = dot3(np.broadcast_to(e1[None], p.shape), p)
        inv = np.where(np.isinf(det), F32(np.nan), F32(1.0) / det).astype(F32)
        tv = o - v0[None]
        U = dot3(tv, p)
        u = U * inv
        q = np.stack([tv[..., 1] * e1[None, :, 2] - tv[..., 2] * e1[None, :, 1], tv[..., 2] * e1[None, :, 0] - tv[..., 0] * e1[None, :, 2],
                      tv[..., 0] * e1[None, :, 1] - tv[..., 1] * e1[None, :, 0]], -1)
        V = dot3(np.broadcast_to(d, q.shape), q)
        v = V * inv
        t = dot3(np.broadcast_to(e2[None], q.shape), q) * inv
        hit = ~((F32(-1e-4) < det) & (det < F32(1e-4))) & ~((u < 0) | (1 < u)) & ~((v < 0) | (1 < inv * (U + V))) & (t > tmin) & (t < tmax)
    return hit, t.astype(F32), u.astype(F32), v.astype(F32)
