"""numpy statement of the adaptive-sampling selection (csrc/pt_kernel.hip.h: adaptive_select_kernel, adaptive_compact_kernel) and of the
masked accumulation with its half buffer (accumulate_adaptive_kernel).

Every operation is one IEEE float32 operation, correctly rounded, in the kernel's order.  The device library is built with denormals
flushed (-fgpu-flush-denormals-to-zero): inputs and results of each operation that are subnormal count as zero of the same sign (ftz).
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
LUM_FLOOR = f32(1e-3)  # kAdaptLumFloor
CANONICAL_NAN = np.uint32(0x7FC00000)
_TINY = np.float32(2.0 ** -126)


def ftz(x):
    x = np.asarray(x, np.float32)
    return np.where(np.abs(x) < _TINY, np.copysign(f32(0), x), x).astype(np.float32)


def _op(fn, *args):
    with np.errstate(all="ignore"):
        return ftz(fn(*[ftz(a) for a in args]))


def tiles_of(rows: int, width: int):
    return (rows + 7) // 8, (width + 7) // 8


def to_tiles(a, fill):
    """(rows, width, ...) -> (tiles_y, tiles_x, 64, ...): lane k of a tile is pixel (k & 7, k >> 3) of it; pixels outside the image get `fill`."""
    a = np.asarray(a)
    rows, width = a.shape[:2]
    ty, tx = tiles_of(rows, width)
    pad = np.full((ty * 8, tx * 8) + a.shape[2:], fill, a.dtype)
    pad[:rows, :width] = a
    t = pad.reshape((ty, 8, tx, 8) + a.shape[2:]).swapaxes(1, 2)
    return t.reshape((ty, tx, 64) + a.shape[2:])


def pixel_error(acc, half):
    """d per pixel: (|I.r - A.r| + |I.g - A.g| + |I.b - A.b|) / sqrt(I.r + I.g + I.b + kAdaptLumFloor), I = acc.rgb / acc.w, A = half.rgb / half.w."""
    acc, half = np.asarray(acc, np.float32), np.asarray(half, np.float32)
    div, add, sub = np.divide, np.add, np.subtract
    i = [_op(div, acc[..., c], acc[..., 3]) for c in range(3)]
    a = [_op(div, half[..., c], half[..., 3]) for c in range(3)]
    e = [np.abs(_op(sub, i[c], a[c])) for c in range(3)]
    num = _op(add, _op(add, e[0], e[1]), e[2])
    den = _op(np.sqrt, _op(add, _op(add, _op(add, i[0], i[1]), i[2]), LUM_FLOOR))
    return _op(div, num, den)


def tile_error(acc, half):
    """E per tile (tiles_y, tiles_x) float32: the 64 lanes (0 outside the image) summed as a tree, s[k] += s[k + h] for h = 32 .. 1, divided by
    the number of in-image pixels.  A NaN is returned as the canonical quiet NaN 0x7FC00000, as the debug export writes it."""
    acc = np.asarray(acc, np.float32)
    rows, width = acc.shape[:2]
    d = to_tiles(pixel_error(acc, half), f32(0))
    inside = to_tiles(np.ones((rows, width), bool), False)
    d = np.where(inside, d, f32(0)).astype(np.float32)
    h = 32
    while h >= 1:
        d = _op(np.add, d[..., :h], d[..., h:2 * h])
        h //= 2
    e = _op(np.divide, d[..., 0], inside.sum(-1).astype(np.float32))
    return np.where(np.isnan(e), CANONICAL_NAN.view(np.float32), e).astype(np.float32)


def select(acc, half, threshold, min_samples):
    """(mask (tiles_y, tiles_x) uint8, E (tiles_y, tiles_x) float32, ascending list of active tile ids (row-major)) of glrtx_render_adaptive's selection."""
    acc, half = np.asarray(acc, np.float32), np.asarray(half, np.float32)
    e = tile_error(acc, half)
    with np.errstate(invalid="ignore"):
        force_px = (ftz(acc[..., 3]) < f32(min_samples)) | (ftz(half[..., 3]) == f32(0))
    force = to_tiles(force_px, False).any(-1)
    with np.errstate(invalid="ignore"):
        active = force | (f32(threshold) < 0) | ~(e <= f32(threshold))
    mask = active.astype(np.uint8)
    return mask, e, np.flatnonzero(mask.reshape(-1)).astype(np.int32)


def expand_mask(mask, rows, width):
    """Tile mask -> per-pixel bool (rows, width)."""
    return np.repeat(np.repeat(np.asarray(mask, bool), 8, 0), 8, 1)[:rows, :width]


def accumulate(acc, half, samples, mask):
    """accumulate_adaptive_kernel: add samples (n, rows, width, 4) -- {min(L, 100), 1} per frame and sample, in order -- to the pixels of active tiles;
    a sample also goes into half when the pixel's count before the add is odd.  Returns new (acc, half)."""
    acc, half = np.array(acc, np.float32), np.array(half, np.float32)
    on = expand_mask(mask, acc.shape[0], acc.shape[1])
    for v in np.asarray(samples, np.float32):
        odd = on & ((acc[..., 3].astype(np.int64) & 1) == 1)
        for c in range(3):
            half[..., c] = np.where(odd, _op(np.add, half[..., c], v[..., c]), half[..., c])
            acc[..., c] = np.where(on, _op(np.add, acc[..., c], v[..., c]), acc[..., c])
        half[..., 3] = np.where(odd, half[..., 3] + f32(1), half[..., 3])
        acc[..., 3] = np.where(on, acc[..., 3] + f32(1), acc[..., 3])
    return acc, half
