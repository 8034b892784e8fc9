"""numpy statement of firefly re-weighting by luminance cascades (include/glrtx.h "Firefly re-weighting"; csrc/reweight.hip.h; host/reweight.cpp).

The rules are variance_math's: every operation is one IEEE float32 operation, correctly rounded, in the kernel's order; denormals count as zeros of their
sign on the way into and out of every operation; selects are as written; a NaN that the resolve STORES is 0x7FC00000.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import ftz
from denoise_math import add, canon, div, mul, sub, tiny
from variance_math import lum

f32 = np.float32
N_CASCADES = 6
DEFAULTS = dict(kappa=4.0, start=1.0)


def bounds(start):
    """b_k = start * 8^k, k = 0 .. 5 (exact scalings)."""
    b = [f32(start)]
    for _ in range(1, N_CASCADES):
        b.append(f32(b[-1] * f32(8)))
    return b


def fold_cascades(cascades, accum, planes, start=DEFAULTS["start"]):
    """(C, accumulator) after the sample planes (k, rows, width, 4) were folded, in order, into copies of C (6, rows, width, 4) and of the accumulator
    (rows, width, 4): the sample is split between C_j and C_{j+1} linearly in 1 / luminance, its count goes to one of them, and it is added to the accumulator."""
    C = np.array(cascades, np.float32, copy=True)
    acc = np.array(accum, np.float32, copy=True)
    b = bounds(start)
    with np.errstate(invalid="ignore"):
        for v in np.asarray(planes, np.float32):
            l = lum(v[..., 0], v[..., 1], v[..., 2])
            j = np.zeros(l.shape, np.int64)
            for k in range(1, 5):
                j = np.where(l >= b[k], k, j)
            lower = np.choose(j, b[:5]).astype(np.float32)
            upper = np.choose(j, b[1:6]).astype(np.float32)
            low = ~(l > lower)
            top = ~low & (l >= upper)
            q = div(lower, l)
            w = div(sub(q, f32(0.125)), f32(0.875))
            w = np.where(w > 0, w, f32(0)).astype(np.float32)
            w = np.where(w < 1, w, f32(1)).astype(np.float32)
            wl = np.where(low, f32(1), np.where(top, f32(0), w)).astype(np.float32)
            wu = np.where(low, f32(0), np.where(top, f32(1), sub(f32(1), w))).astype(np.float32)
            jc = np.where(top, 5, j)
            for k in range(N_CASCADES):
                for ch in range(3):
                    C[k, ..., ch] = np.where(j == k, add(C[k, ..., ch], mul(wl, v[..., ch])), C[k, ..., ch])
                    C[k, ..., ch] = np.where(j + 1 == k, add(C[k, ..., ch], mul(wu, v[..., ch])), C[k, ..., ch])
                C[k, ..., 3] = np.where(jc == k, add(C[k, ..., 3], f32(1)), C[k, ..., 3])
            for ch in range(3):
                acc[..., ch] = add(acc[..., ch], v[..., ch])
            acc[..., 3] = add(acc[..., 3], f32(1))
    return C, acc


def counts_above(cascades):
    """T (5, rows, width): T_k = samples at level k or brighter, T_5 = C_5.w, T_k = T_{k+1} + C_k.w."""
    C = np.asarray(cascades, np.float32)
    t = C[5, ..., 3]
    T = [None] * 5
    for k in range(4, -1, -1):
        t = add(t, C[k, ..., 3])
        T[k] = t
    return np.stack(T)


def reweight(cascades, kappa=DEFAULTS["kappa"]):
    """D (rows, width, 4) {rgb, 1}: cascade 0 in full, cascade j as far as the 3x3 neighbourhood holds kappa samples at level j - 1 or brighter besides one."""
    C = np.ascontiguousarray(cascades, np.float32)
    rows, width = C.shape[1:3]
    T = counts_above(C)
    n = T[0]
    dead = tiny(n) | np.isnan(n)
    a = [C[0, ..., ch].copy() for ch in range(3)]
    with np.errstate(invalid="ignore"):
        for j in range(1, N_CASCADES):
            pad = np.zeros((rows + 2, width + 2), np.float32)  # (+0 outside the image: adding it equals skipping it)
            pad[1:-1, 1:-1] = T[j - 1]
            s = np.zeros((rows, width), np.float32)
            for dy in range(3):
                for dx in range(3):
                    s = add(s, pad[dy:dy + rows, dx:dx + width])
            s = sub(s, f32(1))
            s = np.where(s > 0, s, f32(0)).astype(np.float32)
            r = div(s, f32(kappa))
            r = np.where(r < 1, r, f32(1)).astype(np.float32)
            for ch in range(3):
                a[ch] = add(a[ch], mul(r, C[j, ..., ch]))
    D = np.zeros((rows, width, 4), np.float32)
    for ch in range(3):
        D[..., ch] = np.where(dead, f32(0), canon(div(a[ch], n)))
    D[..., 3] = f32(1)
    return D


def hostile_samples(n, rows, width, seed, start=DEFAULTS["start"]):
    """n sample planes (n, rows, width, 4): log-normal HDR samples over every cascade, with grey samples exactly at each bound b_k and one ulp either side of
    it, zeros, negatives, denormals, 1e30, +inf and NaN scattered in."""
    rng = np.random.default_rng(seed)
    v = np.zeros((n, rows, width, 4), np.float32)
    v[..., :3] = (rng.lognormal(0.0, 3.5, (n, rows, width, 1)) * rng.uniform(0.2, 1.8, (n, rows, width, 3))).astype(np.float32)
    v[..., 3] = 1
    b = bounds(start)
    special = []
    for bk in b:
        # a grey sample {g, g, g} has luminance close to g; solve for the g whose fp32 luminance is bk and bk's neighbours
        for target in (np.nextafter(bk, f32(0)), bk, np.nextafter(bk, f32(np.inf))):
            g = f32(target)
            for _ in range(8):
                got = lum(g, g, g)
                if got == target:
                    break
                g = np.nextafter(g, f32(np.inf) if got < target else f32(0))
            special.append((g, g, g))
    special += [(0, 0, 0), (-1, -2, -3), (-0.0, 0.5, -0.25), (1e-40, 1e-41, 1e-39), (1e30, 1e30, 1e30), (np.inf, 1, 1), (1, np.inf, 0), (np.nan, 1, 1),
                (1, 2, np.nan), (3e38, 3e38, 3e38), (1e-30, 0, 0)]
    flat = v.reshape(-1, 4)
    at = rng.choice(flat.shape[0], size=min(flat.shape[0], 4 * len(special)), replace=False)
    for i, p in enumerate(at):
        flat[p, :3] = np.array(special[i % len(special)], np.float32)
    return v


def hostile_cascades(rows, width, seed):
    """Six incoming planes (6, rows, width, 4) for the resolve: integer counts with holes, and fractional, zero, denormal, negative, infinite and NaN counts and
    colours scattered in."""
    rng = np.random.default_rng(seed)
    C = np.zeros((6, rows, width, 4), np.float32)
    fall = np.array([6, 2, 1, 0.5, 0.25, 0.1])[:, None, None]
    C[..., 3] = rng.poisson(fall * np.ones((6, rows, width))).astype(np.float32)
    C[..., :3] = (rng.lognormal(0.0, 2.0, (6, rows, width, 3)) * C[..., 3:4] * (8.0 ** np.arange(6))[:, None, None, None]).astype(np.float32)
    hole = rng.random((rows, width)) < 0.08
    C[:, hole] = 0
    cnt = C[..., 3].reshape(-1)
    odd = [0.5, 2.75, 0.0, -0.0, 1e-40, -1e-41, np.nan, np.inf, -3.0, 1e30]
    at = rng.choice(cnt.shape[0], size=min(cnt.shape[0], max(6, cnt.shape[0] // 25)), replace=False)
    for i, p in enumerate(at):
        cnt[p] = f32(odd[i % len(odd)])
    col = C[..., :3].reshape(-1)
    oddc = [np.nan, np.inf, -np.inf, 1e-40, -5.0, 3e38]
    at = rng.choice(col.shape[0], size=min(col.shape[0], max(6, col.shape[0] // 60)), replace=False)
    for i, p in enumerate(at):
        col[p] = f32(oddc[i % len(oddc)])
    return C
