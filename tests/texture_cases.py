"""The lookup cases tests/test_texture_host.py (CPU) and tests/test_gpu_texture.py (GPU) share: textures of 1x1, 1x7, 2x3, 5x4 and 64x64 texels in all three
formats, both filters and both wrap modes per axis, and the coordinates they are looked up at."""
import functools

import numpy as np

SIZES = ((1, 1), (1, 7), (2, 3), (5, 4), (64, 64))  # (width, height)
FORMATS = ("rgba32f", "rgba8_unorm", "rgba8_srgb")
FILTERS = ("nearest", "bilinear")
WRAPS = (("repeat", "repeat"), ("clamp", "clamp"), ("repeat", "clamp"), ("clamp", "repeat"))


def texels(width, height, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == "rgba32f":
        return rng.uniform(0.0, 1.0, (height, width, 4)).astype(np.float32)
    return rng.integers(0, 256, (height, width, 4), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def textures():
    """Every (size, format, filter, wrap pair): 5 x 3 x 2 x 4 = 120 textures, as host.pack_textures takes them."""
    out = []
    for k, (w, h) in enumerate(SIZES):
        for f, fmt in enumerate(FORMATS):
            arr = texels(w, h, fmt, 100 * k + f)
            for filt in FILTERS:
                for wrap in WRAPS:
                    out.append((arr, fmt, wrap, filt))
    return out


def _neighbours(x):
    x = np.asarray(x, np.float32)
    return np.concatenate([np.nextafter(x, np.float32(-np.inf)), x, np.nextafter(x, np.float32(np.inf))])


@functools.lru_cache(maxsize=None)
def axis_values(n):
    """One axis of size n: every k / n for k in -n .. 2n and its two float neighbours, then the special values (and two denormals)."""
    grid = (np.arange(-n, 2 * n + 1, dtype=np.float32) / np.float32(n)).astype(np.float32)
    special = np.array([0.0, 1.0, -0.0, 1e-30, -1e-30, 1e30, -1e30, np.inf, -np.inf, np.nan, 1e-40, -1e-40], np.float32)  # (the last two are denormals: zeros)
    return np.concatenate([_neighbours(grid), special])


def coordinates(width, height, seed):
    """(n, 2): 4096 uniform in [-3, 3]^2; the grid and special values of each axis against a few values of the other."""
    rng = np.random.default_rng(seed)
    parts = [rng.uniform(-3.0, 3.0, (4096, 2)).astype(np.float32)]
    sx, sy = axis_values(width), axis_values(height)
    other = np.array([0.3, -0.0, 1.0, np.nan, 0.999], np.float32)
    parts.append(np.stack([np.repeat(sx, other.size), np.tile(other, sx.size)], 1))
    parts.append(np.stack([np.tile(other, sy.size), np.repeat(sy, other.size)], 1))
    m = min(sx.size, sy.size)
    parts.append(np.stack([sx[:m], sy[:m][::-1]], 1))
    return np.concatenate(parts, 0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def batch():
    """(textures, which (n,), st (n, 2)): every texture at its size's coordinates, in one batch."""
    tex = textures()
    which, st = [], []
    for k, (arr, _, _, _) in enumerate(tex):
        c = coordinates(arr.shape[1], arr.shape[0], 7 + k)
        which.append(np.full(c.shape[0], k, np.int32))
        st.append(c)
    return tex, np.concatenate(which), np.concatenate(st, 0)
