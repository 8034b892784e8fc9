"""The environment cases tests/test_env_host.py (CPU) and tests/test_gpu_env.py (GPU) share: hostile maps with their configurations, hostile directions and the
uniforms sampling is driven with."""
import functools

import numpy as np

F = np.float32
QUARTER_TURN = (0, 0, -1, 0, 1, 0, 1, 0, 0)  # about +y: what the map holds along +z is seen along world +x


def _rot(seed):
    """A rotation with no special structure, rounded to float32 (the statements take it as given)."""
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return tuple(float(v) for v in q.astype(F).reshape(9))


@functools.lru_cache(maxsize=None)
def maps():
    """[(name, env_map (array, format, filter), cfg keywords)]: a single non-zero texel, all zero, 2 x 2, N no multiple of G (both ways round), G > N, the three
    formats with both filters, a scale and a rotation."""
    rng = np.random.default_rng(5)
    one = np.zeros((8, 8, 4), F)
    one[5, 2, :3] = (3.0, 7.0, 1.0)
    out = [("one texel", (one, "rgba32f", "bilinear"), dict(grid=4, light_pick=1.0)),
           ("one texel nearest", (one, "rgba32f", "nearest"), dict(grid=8, light_pick=0.25)),
           ("all zero", (np.zeros((4, 4, 4), F), "rgba32f", "bilinear"), dict(grid=2, light_pick=0.5)),
           ("2 x 2", (rng.uniform(0, 4, (2, 2, 4)).astype(F), "rgba32f", "bilinear"), dict(grid=0, light_pick=1.0)),
           ("10 over 4", (rng.uniform(0, 2, (10, 10, 4)).astype(F), "rgba32f", "bilinear"), dict(grid=4, light_pick=0.75, scale=(0.5, 2.0, 1.5))),
           ("7 over 3", (rng.uniform(0, 2, (7, 7, 4)).astype(F), "rgba32f", "nearest"), dict(grid=3, light_pick=1.0, rotation=_rot(1))),
           ("4 over 6", (rng.uniform(0, 2, (4, 4, 4)).astype(F), "rgba32f", "bilinear"), dict(grid=6, light_pick=1.0, rotation=QUARTER_TURN))]
    for fmt in ("rgba32f", "rgba8_unorm", "rgba8_srgb"):
        arr = rng.uniform(0, 1, (16, 16, 4)).astype(F) if fmt == "rgba32f" else rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
        for filt in ("nearest", "bilinear"):
            out.append((f"{fmt} {filt}", (arr, fmt, filt), dict(grid=8, light_pick=0.5, scale=(1.0, 0.5, 2.0), rotation=_rot(2))))
    return out


def axes():
    return np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float64)


def edge_midpoints():
    out = []
    for a in range(3):
        for b in range(a + 1, 3):
            for sa in (1, -1):
                for sb in (1, -1):
                    v = np.zeros(3)
                    v[a], v[b] = sa, sb
                    out.append(v)
    return np.array(out)


def face_centres():
    return np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float64)


@functools.lru_cache(maxsize=None)
def unit_directions(n=10_000, seed=3):
    """The six axes, the twelve edge midpoints, the eight face centres and n random directions, normalised in float64: (26 + n, 3)."""
    rng = np.random.default_rng(seed)
    d = np.concatenate([axes(), edge_midpoints(), face_centres(), rng.normal(size=(n, 3))], 0)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def directions():
    """(n, 3) float32: hostile directions (zero, denormal, inf, NaN, axis-aligned, ey = -0), the symmetric ones and 2000 random of every length."""
    hostile = np.array([[0, 0, 0], [-0.0, -0.0, -0.0], [1e-40, 0, 0], [0, -1e-40, 1e-41], [1e-40, 1e-40, 1e-40], [np.inf, 0, 0], [0, -np.inf, 0], [1, np.inf, 1],
                        [np.nan, 0, 0], [0, 1, np.nan], [np.inf, np.nan, -np.inf], [1, -0.0, 0], [0, -0.0, 1], [0.5, -0.0, -0.5], [-1, -0.0, -1], [1, 1e-40, 0],
                        [1, -1e-40, 0.25], [1e30, 1e30, 1e30], [3e38, 3e38, 3e38], [1e-20, -1e-20, 1e-20], [1e-30, 0, 0]], F)
    rng = np.random.default_rng(4)
    rand = rng.normal(size=(2000, 3)) * 10.0 ** rng.uniform(-3, 3, (2000, 1))
    return np.concatenate([hostile, axes().astype(F), -2.5 * axes().astype(F), edge_midpoints().astype(F), face_centres().astype(F), rand.astype(F)], 0)


@functools.lru_cache(maxsize=None)
def uniforms(n=3000, seed=6):
    """(m, 6) float32 in [0, 1): random rows, then rows of edge values (0, the largest float below 1, cell boundaries of grids 2 .. 8)."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(0, 1, (n, 6)).astype(F)
    u[u >= 1] = np.nextafter(F(1), F(0))
    edge = np.array([0.0, np.nextafter(F(1), F(0)), 0.5, 0.25, 0.75, 1 / 3, 2 / 3, 0.125, 0.375, np.nextafter(F(0.5), F(0)), 1e-40], F)
    grid = np.stack(np.meshgrid(edge, edge, indexing="ij"), -1).reshape(-1, 2)
    rows = [np.concatenate([g, rng.uniform(0, 1, 4).astype(F)])[[0, 2, 1, 3, 4, 5]] for g in grid]          # entries of both tables
    rows += [np.concatenate([rng.uniform(0, 1, 4).astype(F), g]) for g in grid]                              # the jitter
    rows += [np.concatenate([rng.uniform(0, 1, 1).astype(F), g[:1], rng.uniform(0, 1, 1).astype(F), g[1:], rng.uniform(0, 1, 2).astype(F)]) for g in grid]  # thresholds
    return np.concatenate([u, np.array(rows, F)], 0)
