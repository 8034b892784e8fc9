"""numpy statement of the adaptive selection made from the moments plane M (include/glrtx.h "Adaptive sampling by variance"; csrc/variance.hip.h:
adaptive_moments::select_kernel; host/variance.cpp: glrt_adaptive_select_moments) and of the masked accumulation that folds M (accumulate.hip.h: the
MomentsMasked sink).

The rules are variance_math's: every operation is one IEEE float32 operation, correctly rounded, in the kernel's order; denormals count as zeros of their
sign on the way into and out of every operation; a NaN that is STORED is 0x7FC00000.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import CANONICAL_NAN, LUM_FLOOR, _op, expand_mask, ftz, tiles_of, to_tiles  # noqa: F401  (tiles_of: for the callers)
from variance_math import lum, max0

f32 = np.float32


def pixel_error(M):
    """d per pixel: sqrt(max(mu2 - mu1 * mu1, 0) / M.w) / sqrt(mu1 + kAdaptLumFloor), mu1 = M.x / M.w, mu2 = M.y / M.w."""
    M = np.asarray(M, np.float32)
    n = M[..., 3]
    mu1, mu2 = _op(np.divide, M[..., 0], n), _op(np.divide, M[..., 1], n)
    v = _op(np.divide, max0(_op(np.subtract, mu2, _op(np.multiply, mu1, mu1))), n)
    return _op(np.divide, _op(np.sqrt, v), _op(np.sqrt, _op(np.add, mu1, LUM_FLOOR)))


def tile_error(M):
    """E per tile (tiles_y, tiles_x) float32: the 64 lanes (0 outside the image) summed as a tree, s[k] += s[k ^ h] for h = 32 .. 1, divided by the
    number of in-image pixels.  A NaN is returned as the canonical quiet NaN 0x7FC00000, as the debug export writes it."""
    M = np.asarray(M, np.float32)
    rows, width = M.shape[:2]
    inside = to_tiles(np.ones((rows, width), bool), False)
    d = np.where(inside, to_tiles(pixel_error(M), f32(0)), f32(0)).astype(np.float32)
    h = 32
    while h >= 1:
        d = _op(np.add, d[..., :h], d[..., h:2 * h])
        h //= 2
    e = _op(np.divide, d[..., 0], inside.sum(-1).astype(np.float32))
    return np.where(np.isnan(e), CANONICAL_NAN.view(np.float32), e).astype(np.float32)


def select(M, threshold, min_samples):
    """(mask (tiles_y, tiles_x) uint8, E (tiles_y, tiles_x) float32, ascending list of active tile ids (row-major)) of glrtx_render_adaptive_moments'
    selection: a tile is active if a pixel has !(M.w >= min_samples), if threshold < 0 or if !(E <= threshold)."""
    M = np.asarray(M, np.float32)
    e = tile_error(M)
    with np.errstate(invalid="ignore"):
        force_px = ~(ftz(M[..., 3]) >= f32(min_samples))
        active = to_tiles(force_px, False).any(-1) | (f32(threshold) < 0) | ~(e <= f32(threshold))
    mask = active.astype(np.uint8)
    return mask, e, np.flatnonzero(mask.reshape(-1)).astype(np.int32)


def accumulate(acc, M, samples, mask):
    """The MomentsMasked pass: the samples (n, rows, width, 4) -- {min(L, 100), 1} per frame and sample, in order -- go to the pixels of active tiles only:
    M.x += l; M.y += l * l; M.w += 1, then acc.rgb += v.rgb; acc.w += 1.  Returns new (acc, M)."""
    acc, M = np.array(acc, np.float32), np.array(M, np.float32)
    on = expand_mask(mask, acc.shape[0], acc.shape[1])
    for v in np.asarray(samples, np.float32):
        l = lum(v[..., 0], v[..., 1], v[..., 2])
        M[..., 0] = np.where(on, _op(np.add, M[..., 0], l), M[..., 0])
        M[..., 1] = np.where(on, _op(np.add, M[..., 1], _op(np.multiply, l, l)), M[..., 1])
        M[..., 3] = np.where(on, _op(np.add, M[..., 3], f32(1)), M[..., 3])
        for c in range(3):
            acc[..., c] = np.where(on, _op(np.add, acc[..., c], v[..., c]), acc[..., c])
        acc[..., 3] = np.where(on, acc[..., 3] + f32(1), acc[..., 3])
    return acc, M
