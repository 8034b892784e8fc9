"""numpy statement of the bloom pass (include/glrtx.h "Bloom"; csrc/bloom.hip.h; host/bloom.cpp).

Every fp32 operation is one IEEE float32 operation, correctly rounded, in the order the header writes it; nothing is fused.  Denormals count as zeros of
their sign on the way into and out of every operation (ftz), as in tonemap_math.py.  Selects are selects: a NaN on the way in becomes 0.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import _op, ftz
from tonemap_math import dead_of, hostile_array, lum, mean_of

f32 = np.float32
DEFAULTS = dict(source=0, threshold=1.0, strength=0.25, levels=5)
SIZES = [(1, 1), (2, 3), (13, 67), (9, 131), (37, 70), (5, 300)]  # (rows, width): 1x1, 3x2, 67x13, 131x9, 70x37, 300x5 as width x height
LEVELS = (1, 2, 5, 8)


def add(a, b): return _op(np.add, a, b)
def sub(a, b): return _op(np.subtract, a, b)
def mul(a, b): return _op(np.multiply, a, b)
def div(a, b): return _op(np.divide, a, b)


def level_sizes(width, rows, levels):
    """[(w_0, h_0), .., (w_levels, h_levels)]: w_{k+1} = (w_k + 1) >> 1."""
    out = [(int(width), int(rows))]
    for _ in range(levels):
        w, h = out[-1]
        out.append(((w + 1) >> 1, (h + 1) >> 1))
    return out


def pixel_value(src):
    """x: I = src.rgb / src.w clamped to [0, 65504] by selects (a NaN: 0); a dead pixel: zeros."""
    src = np.ascontiguousarray(src, np.float32)
    I = mean_of(src)
    with np.errstate(invalid="ignore"):
        x = np.where(I > 0, I, f32(0)).astype(np.float32)
        x = np.where(x < f32(65504), x, f32(65504)).astype(np.float32)
    return np.where(dead_of(src)[..., None], f32(0), x).astype(np.float32)


def bright(x, threshold):
    """D_0 = x * g, g = max(l - threshold, 0) / max(l, 1e-4)."""
    l = lum(x)
    n = sub(l, f32(threshold))
    n = np.where(n > 0, n, f32(0)).astype(np.float32)
    m = np.where(l > f32(1e-4), l, f32(1e-4)).astype(np.float32)
    return mul(x, div(n, m)[..., None])


def c5(a, b, c, d, e):
    return add(add(add(a, e), mul(f32(4), add(b, d))), mul(f32(6), c))


def down(D):
    """One level of the down chain on a (h, w, 3) plane: the binomial kernel, horizontal first, clamp to edge, times 2^-8."""
    h, w = D.shape[:2]
    wn, hn = (w + 1) >> 1, (h + 1) >> 1
    X = [np.clip(2 * np.arange(wn) + i, 0, w - 1) for i in range(-2, 3)]
    Y = [np.clip(2 * np.arange(hn) + j, 0, h - 1) for j in range(-2, 3)]
    r = c5(*[D[:, X[i]] for i in range(5)])  # (r_j depends on the source row alone: one horizontal pass over all of them)
    return mul(c5(*[r[Y[j]] for j in range(5)]), f32(2.0 ** -8))


def _near_far(n, nc):
    x = np.arange(n)
    near = x >> 1
    far = np.where(x & 1, near + 1, near - 1)
    return np.clip(near, 0, nc - 1), np.clip(far, 0, nc - 1)


def up(C, w, h):
    """The (h, w, 3) interpolation of the (hc, wc, 3) plane C: 3/4 of the near texel and 1/4 of the far one, horizontally, then vertically."""
    hc, wc = C.shape[:2]
    nx, fx = _near_far(w, wc)
    ny, fy = _near_far(h, hc)
    hz = add(mul(f32(0.75), C[:, nx]), mul(f32(0.25), C[:, fx]))
    return add(mul(f32(0.75), hz[ny]), mul(f32(0.25), hz[fy]))


def bloom(src, threshold=DEFAULTS["threshold"], strength=DEFAULTS["strength"], levels=DEFAULTS["levels"], **_):
    """(d, B): d the planes D_1 .. D_levels packed back to back as (n, 4) float32 with w = 0; B (rows, width, 4) float32 {x + strength * glow, 1}."""
    src = np.ascontiguousarray(src, np.float32)
    rows, width = src.shape[:2]
    x = pixel_value(src)
    D = [bright(x, threshold)]
    for _k in range(levels):
        D.append(down(D[-1]))
    d = np.zeros((sum(p.shape[0] * p.shape[1] for p in D[1:]), 4), np.float32)
    at = 0
    for p in D[1:]:
        n = p.shape[0] * p.shape[1]
        d[at:at + n, :3] = p.reshape(n, 3)
        at += n
    U = D[levels]
    for k in range(levels - 1, 0, -1):
        U = add(D[k], up(U, D[k].shape[1], D[k].shape[0]))
    glow = mul(up(U, width, rows), div(f32(1), f32(levels)))
    B = np.ones(src.shape, np.float32)
    B[..., :3] = add(x, mul(ftz(f32(strength)), glow))
    return d, B


def hostile(rows, width, seed, threshold=1.0):
    """tonemap_math.hostile_array plus what the bright pass has rules for: grey pixels whose luminance sits on and around the threshold and 1e-4."""
    a = hostile_array(max(rows, 13), max(width, 67), seed)[:rows, :width].copy() if rows * width < 64 else hostile_array(rows, width, seed)
    rng = np.random.default_rng(seed + 1000)
    k = rng.permutation(rows * width)[:min(12, rows * width)]
    vals = []
    for centre in (threshold, 1e-4):
        for ulp in (-2, -1, 0, 1, 2, 64):
            vals.append((np.array([centre], np.float32).view(np.uint32) + np.uint32(ulp & 0xFFFFFFFF)).view(np.float32)[0])
    for i, kk in enumerate(k):
        a[kk // width, kk % width] = (vals[i], vals[i], vals[i], 1.0)
    return a
