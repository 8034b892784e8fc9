"""The environment lighting of include/glrtx.h "Environment" in numpy: the third statement beside csrc/environment.hip.h and host/environment.cpp, bit for bit.

Every operation is one float32 operation in the order the header writes it (add / sub / mul / div of tests/texture_math.py flush denormal operands and
results); the map is looked up through texture_math.  An environment map is given as glrt_amd.host.pack_environment takes it -- (array, format, filter) -- and a
configuration as a dict(mode, grid, light_pick, scale (3,), rotation (9,)).
"""
from __future__ import annotations

import numpy as np

import texture_math as tm
from texture_math import F, add, div, ftz, mul, sub

IDENTITY = (1, 0, 0, 0, 1, 0, 0, 0, 1)
LANES = 64  # env_weights_kernel: one wave a cell


def cfg(mode=0, grid=0, light_pick=0.5, scale=1.0, rotation=IDENTITY):
    return dict(mode=int(mode), grid=int(grid), light_pick=F(light_pick), scale=np.broadcast_to(np.asarray(scale, F), (3,)).copy(),
                rotation=np.asarray(rotation, F).reshape(9).copy())


def _sqrt(a):
    with np.errstate(all="ignore"):
        return ftz(np.sqrt(ftz(a)))


def _abs(a):
    return np.abs(ftz(a)).astype(F)


def _signed(m, of):
    return np.where(ftz(of) < 0, -ftz(m), ftz(m)).astype(F)


def _rot(R, x, y, z, transpose=False):
    k = (lambda r, c: R[3 * c + r]) if transpose else (lambda r, c: R[3 * r + c])
    return [add(add(mul(k(r, 0), x), mul(k(r, 1), y)), mul(k(r, 2), z)) for r in range(3)]


def dir_to_st(R, d):
    """d (n, 3) -> (ok (n,), s, t, n1)."""
    d = np.asarray(d, F).reshape(-1, 3)
    ex, ey, ez = _rot(np.asarray(R, F), d[:, 0], d[:, 1], d[:, 2])
    l = add(add(_abs(ex), _abs(ey)), _abs(ez))
    with np.errstate(all="ignore"):
        ok = (l > 0) & (l < np.inf)
    px, py, pz = div(ex, l), div(ey, l), div(ez, l)
    n1 = div(F(1), _sqrt(add(add(mul(pz, pz), mul(py, py)), mul(px, px))))
    fold = ey < 0
    fx = _signed(sub(F(1), _abs(pz)), px)
    fz = _signed(sub(F(1), _abs(px)), pz)
    px, pz = np.where(fold, fx, px).astype(F), np.where(fold, fz, pz).astype(F)
    s = add(mul(px, F(0.5)), F(0.5))
    t = add(mul(pz, F(0.5)), F(0.5))
    return ok, np.where(ok, s, F(0)).astype(F), np.where(ok, t, F(0)).astype(F), np.where(ok, n1, F(0)).astype(F)


def st_to_dir(R, s, t):
    """(s, t) arrays -> (direction (n, 3), n1 (n,))."""
    s, t = np.asarray(s, F).reshape(-1), np.asarray(t, F).reshape(-1)
    u, v = sub(mul(s, F(2)), F(1)), sub(mul(t, F(2)), F(1))
    au, av = _abs(u), _abs(v)
    y = sub(sub(F(1), au), av)
    fold = y < 0
    x = np.where(fold, _signed(sub(F(1), av), u), u).astype(F)
    z = np.where(fold, _signed(sub(F(1), au), v), v).astype(F)
    r = div(F(1), _sqrt(add(add(mul(z, z), mul(y, y)), mul(x, x))))
    qx, qy, qz = mul(x, r), mul(y, r), mul(z, r)
    n1 = mul(r, add(add(_abs(x), _abs(y)), _abs(z)))
    return np.stack(_rot(np.asarray(R, F), qx, qy, qz, transpose=True), 1), n1


def jacobian(n1):
    return mul(F(4), mul(mul(n1, n1), n1))


def lookup(env_map, c, s, t):
    arr, fmt, filt = env_map
    rgb = tm.lookup([(arr, fmt, "clamp", filt)], np.zeros(np.size(s), np.int64), np.stack([s, t], 1))
    return mul(c["scale"][None, :], rgb)


def grid_of(env_map, c):
    n = np.asarray(env_map[0]).shape[0]
    return c["grid"] if c["grid"] > 0 else min(n, 256)


def cell(s, G):
    a = mul(s, F(G))
    with np.errstate(all="ignore"):
        ok = a >= 0  # (a NaN: cell 0)
        inside = ok & (a < F(G))
        i = np.where(inside, a, F(0)).astype(np.int64)
    return np.where(ok & ~inside, G - 1, i)


def block(c, N, G):
    lo = (c * N) // G - 1
    hi = ((c + 1) * N + G - 1) // G
    return max(lo, 0), min(hi, N - 1)


def weights(env_map, c):
    """(G, G) float32 cell weights in the device's summation order."""
    arr, fmt, _ = env_map
    tex = tm.decode(arr, tm._code(fmt))
    N = tex.shape[0]
    G = grid_of(env_map, c)
    centre = div(add(np.arange(N, dtype=F), F(0.5)), F(N))
    ss, tt = np.meshgrid(centre, centre)  # [y, x]
    _, n1 = st_to_dir(c["rotation"], ss.reshape(-1), tt.reshape(-1))
    sc = mul(c["scale"][None, None, :], tex)
    lum = add(add(mul(F(0.2126), sc[..., 0]), mul(F(0.7152), sc[..., 1])), mul(F(0.0722), sc[..., 2]))
    w = mul(lum, jacobian(n1).reshape(N, N))
    with np.errstate(all="ignore"):
        w = np.where((w > 0) & (w < np.inf), w, F(0)).astype(F)
    out = np.zeros((G, G), F)
    for cj in range(G):
        y0, y1 = block(cj, N, G)
        for ci in range(G):
            x0, x1 = block(ci, N, G)
            flat = w[y0:y1 + 1, x0:x1 + 1].reshape(-1)
            pad = np.zeros(-(-flat.size // LANES) * LANES, F)
            pad[:flat.size] = flat
            rows = pad.reshape(-1, LANES)
            part = np.zeros(LANES, F)
            for r in rows:  # lane k adds texels k, k + 64, .. in order
                part = add(part, r)
            h = LANES // 2
            while h >= 1:
                part[:h] = add(part[:h], part[h:2 * h])
                h //= 2
            out[cj, ci] = part[0]
    return out


def alias(w):
    """Vose's method in float64 in the order host/env_tables.h states: (thresholds float32, aliases int32)."""
    w = np.asarray(w, np.float64).reshape(-1)
    n = w.size
    total = 0.0
    for v in w:
        total += float(v)
    q, al = np.ones(n, F), np.arange(n, dtype=np.int32)
    if not (total > 0.0) or not np.isfinite(total):
        return q, al
    p = [float(v) * float(n) / total for v in w]
    small = [i for i in range(n) if p[i] < 1.0]
    large = [i for i in range(n) if not p[i] < 1.0]
    while small and large:
        s, l = small.pop(), large.pop()
        q[s] = F(p[s])
        al[s] = l
        p[l] = (p[l] + p[s]) - 1.0
        (small if p[l] < 1.0 else large).append(l)
    return q, al


def tables(w):
    w = np.asarray(w, F)
    G = w.shape[0]
    rows = np.zeros(G, np.float64)
    for j in range(G):
        for i in range(G):
            rows[j] += float(w[j, i])
    total = 0.0
    for j in range(G):
        total += rows[j]
    row_q, row_alias = alias(rows)
    col = [alias(w[j].astype(np.float64)) for j in range(G)]
    cell_p = np.zeros((G, G), F)
    if total > 0.0 and np.isfinite(total):
        cell_p = (w.astype(np.float64) / total).astype(F)
    return dict(row_q=row_q, row_alias=row_alias, col_q=np.stack([c[0] for c in col]), col_alias=np.stack([c[1] for c in col]), cell_p=cell_p)


def realised(t):
    """The probability of every cell that the tables realise, exactly in float64: (G, G)."""
    def one(q, al):
        n = q.size
        p = np.zeros(n, np.float64)
        for i in range(n):
            p[i] += float(q[i]) / n
            p[al[i]] += (1.0 - float(q[i])) / n
        return p
    rows = one(t["row_q"], t["row_alias"])
    return np.stack([rows[j] * one(t["col_q"][j], t["col_alias"][j]) for j in range(rows.size)])


def pdf(t, c, G, ci, cj, n1):
    g2 = mul(F(G), F(G))
    return mul(div(mul(t["cell_p"][cj, ci], g2), jacobian(n1)), c["light_pick"])


def sample(env_map, c, u, t=None):
    """u (n, 6) -> (n, 8) {direction, pdf, Le.rgb, 0}."""
    u = np.asarray(u, F).reshape(-1, 6)
    G = grid_of(env_map, c)
    t = tables(weights(env_map, c)) if t is None else t
    cj = cell(u[:, 0], G)
    cj = np.where(ftz(u[:, 1]) < t["row_q"][cj], cj, t["row_alias"][cj])
    ci = cell(u[:, 2], G)
    ci = np.where(ftz(u[:, 3]) < t["col_q"][cj, ci], ci, t["col_alias"][cj, ci])
    s = div(add(ci.astype(F), u[:, 4]), F(G))
    tt = div(add(cj.astype(F), u[:, 5]), F(G))
    d, n1 = st_to_dir(c["rotation"], s, tt)
    out = np.zeros((u.shape[0], 8), F)
    out[:, :3] = d
    out[:, 3] = pdf(t, c, G, ci, cj, n1)
    out[:, 4:7] = lookup(env_map, c, s, tt)
    return out


def evaluate(env_map, c, dirs, t=None):
    """dirs (n, 3) -> (n, 4) {Le.rgb, pdf}."""
    d = np.asarray(dirs, F).reshape(-1, 3)
    G = grid_of(env_map, c)
    t = tables(weights(env_map, c)) if t is None else t
    ok, s, tt, n1 = dir_to_st(c["rotation"], d)
    out = np.zeros((d.shape[0], 4), F)
    out[:, :3] = lookup(env_map, c, s, tt)
    out[:, 3] = pdf(t, c, G, cell(s, G), cell(tt, G), n1)
    out[~ok] = 0
    return out
