"""Moments planes for the selection's tests (CPU and GPU): plausible planes, and the hostile pixels the contract names, alone and sprinkled over a plane."""
from __future__ import annotations

import numpy as np

f32 = np.float32
SIZES = [(1, 1), (3, 5), (8, 8), (50, 38), (241, 135)]  # (width, rows): a single pixel, one partial tile, one whole tile, partial tiles on both edges
MIN_SAMPLES = 4


def plausible(width, rows, seed, n_lo=MIN_SAMPLES, n_hi=64):
    """M of pixels with n in [n_lo, n_hi] samples of mean m and spread s: {n m, n (m^2 + s^2), 0, n}, noisier towards the right."""
    rng = np.random.default_rng(seed)
    n = rng.integers(n_lo, n_hi + 1, (rows, width)).astype(np.float32)
    m = rng.uniform(0.02, 2.0, (rows, width)).astype(np.float32)
    s = (rng.uniform(0.0, 1.0, (rows, width)) * np.linspace(0.05, 1.0, width)[None, :]).astype(np.float32)
    M = np.zeros((rows, width, 4), np.float32)
    M[..., 0] = n * m
    M[..., 1] = n * (m * m + s * s)
    M[..., 3] = n
    return M


def hostile_pixels(min_samples=MIN_SAMPLES):
    """[(name, float4)]: the counts and sums the contract names."""
    nan, inf = f32(np.nan), f32(np.inf)
    out = []
    for name, w in [("w_zero", 0.0), ("w_negzero", -0.0), ("w_denormal", 1e-40), ("w_negative", -3.0), ("w_nan", nan), ("w_inf", inf), ("w_one", 1.0),
                    ("w_min_minus_1", min_samples - 1), ("w_min", min_samples), ("w_2p24", 2.0 ** 24)]:
        w = f32(w)
        out.append((name, np.array([f32(0.7) * (w if np.isfinite(w) else f32(1)), f32(0.6) * (w if np.isfinite(w) else f32(1)), 0, w], np.float32)))
    # sum l^2 below (sum l)^2 / n by one ulp: n a power of two, so both divisions are exact and mu2 - mu1 * mu1 is one ulp below zero
    mu1 = f32(0.3)
    sq = f32(mu1 * mu1)
    for name, mu2 in [("v_minus_ulp", np.nextafter(sq, f32(0))), ("v_zero", sq), ("v_plus_ulp", np.nextafter(sq, f32(1)))]:
        out.append((name, np.array([mu1 * f32(8), f32(mu2) * f32(8), 0, 8], np.float32)))
    for name, x, y in [("x_nan", nan, 1.0), ("x_inf", inf, 1.0), ("x_neginf", -inf, 1.0), ("y_nan", 1.0, nan), ("y_inf", 1.0, inf), ("xy_inf", inf, inf),
                       ("x_denormal", 1e-39, 1e-39)]:
        out.append((name, np.array([x, y, 0, 8], np.float32)))
    # mu1 at and around -1e-3: mu1 + floor is 0 (d = sqrt(v) / 0), just below (the root of a negative number) and just above
    floor = f32(1e-3)
    for name, m in [("mu1_at_minus_floor", -floor), ("mu1_below_minus_floor", np.nextafter(-floor, f32(-1))), ("mu1_above_minus_floor", np.nextafter(-floor, f32(0)))]:
        for tag, y in [("", 1.0), ("_v0", 0.0)]:
            out.append((name + tag, np.array([f32(m) * f32(8), y, 0, 8], np.float32)))
    return out


def sprinkled(width, rows, seed, min_samples=MIN_SAMPLES):
    """A plausible plane with every hostile pixel placed once (where the plane has room), at positions drawn from the seed."""
    M = plausible(width, rows, seed)
    rng = np.random.default_rng(seed + 1)
    px = hostile_pixels(min_samples)
    at = rng.permutation(width * rows)[:len(px)]
    for i, q in zip(at, px):
        M[i // width, i % width] = q[1]
    return M


def planes():
    """[(id, M)]: per size a plausible plane and a sprinkled one; for the sizes of a single tile, every hostile pixel on its own as well."""
    out = []
    for i, (w, h) in enumerate(SIZES):
        out.append((f"{w}x{h}-plausible", plausible(w, h, 10 + i)))
        out.append((f"{w}x{h}-sprinkled", sprinkled(w, h, 20 + i)))
        if w * h <= 64:
            for name, q in hostile_pixels():
                M = plausible(w, h, 30 + i)
                M[h // 2, w // 2] = q
                out.append((f"{w}x{h}-{name}", M))
    return out


def thresholds(e):
    """-1, 0, a value that falls between two tiles' E (the two middle ones of the finite, distinct E; 0.5 where there are not two), +Inf."""
    v = np.unique(np.asarray(e, np.float32)[np.isfinite(e)])
    mid = float((np.float64(v[len(v) // 2 - 1]) + np.float64(v[len(v) // 2])) / 2) if len(v) >= 2 else 0.5
    return [-1.0, 0.0, mid, float("inf")]
