"""The cases of the normal rebuild (include/glrtx.h "Rebuilding normals"): the smallest shapes at which each rule can go wrong.  The host test walks them
through glrt_normal_topology / glrt_rebuild_normals against tests/normals_math.py, the GPU test through glrtx_debug_rebuild_normals against glrt_rebuild_normals.

A case is (name, rest (n, 15) float32, tri (n_tri, 4) float32, moved (n, 15) float32, class map or None).  `rest` makes the topology, `moved` is what gets
rebuilt.  A class map that is given replaces the weld's (with flips from the rest pose all the same): classes no weld would make, for the debug hook.
"""
from __future__ import annotations

import numpy as np

from glrt_amd import scenes


def _bits_f(u):
    return np.array(u, np.uint32).view(np.float32)


def mesh(pos, nrm):
    """Unindexed wire arrays from (n_tri, 3, 3) positions and normals: three vertices a triangle, as scenes.SceneBuilder lays them out."""
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    nrm = np.asarray(nrm, np.float32).reshape(-1, 3)
    v = np.zeros((pos.shape[0], 15), np.float32)
    v[:, 0:3], v[:, 3:6] = pos, nrm
    v[:, 6:9] = np.arange(pos.shape[0] * 3, dtype=np.float32).reshape(-1, 3) * 0.25  # uv, tangent and binormal: words that must come through untouched
    v[:, 9:15] = np.linspace(-1, 1, pos.shape[0] * 6, dtype=np.float32).reshape(-1, 6)
    t = np.zeros((pos.shape[0] // 3, 4), np.float32)
    t[:, 0:3] = np.arange(pos.shape[0], dtype=np.float32).reshape(-1, 3)
    return v, t


def wobble(v, seed, amount=0.05):
    """The moved surface: welded vertices move together (the offset is a function of the rest position), so classes stay coincident."""
    out = np.array(v, np.float32)
    p = out[:, 0:3].astype(np.float64)
    rng = np.random.default_rng(seed)
    a, ph = rng.uniform(1.0, 3.0, (3, 3)), rng.uniform(0, 6.28, 3)
    out[:, 0:3] = (p + amount * np.sin(p @ a + ph)).astype(np.float32)
    return out


def fan(n):
    """n triangles around one hub: the hub's class lists all n, every rim class two (a closed fan, slightly domed so that nothing cancels)."""
    ang = 2 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(ang), np.sin(ang), np.full(n, -0.1)], -1)
    rim_n = np.stack([np.cos(ang), np.sin(ang), np.ones(n)], -1)
    k, k1 = np.arange(n), (np.arange(n) + 1) % n
    pos = np.stack([np.zeros((n, 3)), rim[k], rim[k1]], 1)
    nrm = np.stack([np.broadcast_to([0.0, 0.0, 1.0], (n, 3)), rim_n[k], rim_n[k1]], 1)
    return mesh(pos, nrm)


def grid(nx, ny):
    """A welded height field of (nx - 1) (ny - 1) quads: nx * ny classes, interior ones of six members."""
    x, y = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64), indexing="ij")
    p = np.stack([x, y, 0.3 * np.sin(x * 0.7) * np.cos(y * 0.9)], -1)
    q = [p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]]
    pos = np.concatenate([np.stack([q[0], q[1], q[2]], -2).reshape(-1, 3, 3), np.stack([q[0], q[2], q[3]], -2).reshape(-1, 3, 3)])
    nrm = np.broadcast_to([0.0, 0.0, 1.0], pos.shape)
    return mesh(pos, nrm)


def strip(n_classes):
    """Exactly n_classes classes: a welded strip of n_classes - 2 triangles over n_classes points (one triangle for three, a lone vertex pair below)."""
    k = np.arange(n_classes, dtype=np.float64)
    p = np.stack([k * 0.5, (k % 2) * 1.0, 0.05 * k * (k % 3)], -1)
    if n_classes < 3:  # 1 or 2 classes: a degenerate triangle over them -- every corner in range, the classes keep their words
        idx = np.array([[0, n_classes - 1, 0]])
    else:
        idx = np.stack([np.arange(n_classes - 2), np.arange(1, n_classes - 1), np.arange(2, n_classes)], -1)
        idx[1::2] = idx[1::2][:, [1, 0, 2]]  # keep the winding
    pos = p[idx]
    nrm = np.broadcast_to([0.0, 0.0, 1.0], pos.shape)
    return mesh(pos, nrm)


def _one_triangle():
    return mesh([[[0, 0, 0], [1, 0, 0], [0, 1, 0]]], [[[0, 0, 1]] * 3])


def _quad(crease=False):
    pos = [[[0, 0, 0], [1, 0, 0], [1, 1, 0.2]], [[0, 0, 0], [1, 1, 0.2], [0, 1, 0]]]
    nrm = np.broadcast_to([0.0, 0.0, 1.0], (2, 3, 3)).copy()
    if crease:
        nrm[1] = [0.0, 0.6, 0.8]
    return mesh(pos, nrm)


def _hostile_positions(v):
    """Positions holding NaN, +-Inf, denormals and -0, one kind a vertex, on a welded grid (so every kind meets ordinary neighbours in a sum)."""
    out = wobble(v, 11)
    kinds = _bits_f([0x7FC00000, 0xFFC12345, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF, 0x80000000, 0x00400000, 0x7F7FFFFF, 0xFF7FFFFF])
    keys = {}
    for i, p in enumerate(map(bytes, np.ascontiguousarray(v[:, 0:3]))):
        keys.setdefault(p, []).append(i)
    for j, members in enumerate(list(keys.values())[::3]):
        out[members, j % 3] = kinds[j % kinds.size]
    return out


def cases():
    out = []
    v, t = _one_triangle()
    out.append(("1 one triangle", v, t, wobble(v, 1, 0.3), None))
    v, t = _quad()
    out.append(("2 quad, two welded corners", v, t, wobble(v, 2, 0.3), None))
    v, t = _quad(crease=True)
    out.append(("3 quad with a crease", v, t, wobble(v, 3, 0.3), None))
    for n in (256, 257, 1000):
        v, t = fan(n)
        out.append((f"4 fan of {n}", v, t, wobble(v, 4), None))
    v, t = mesh([[[0, 0, 0], [1, 1, 1], [2, 2, 2]]], [[[0, 0, 1], [0, 1, 0], [1, 0, 0]]])
    out.append(("5 zero-area triangle", v, t, v.copy(), None))
    pos = [[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 0], [0, 1, 0], [1, 0, 0]]]
    v, t = mesh(pos, [[[0, 0, 1]] * 3, [[0, 0, -1]] * 3])  # each face agrees with its own normals: neither is flipped, and welded by position they cancel
    m = v.copy()
    m[:, 0:3] *= np.float32(1.5)  # scaled by an exact factor: the two face vectors still cancel exactly
    out.append(("6 coincident opposite faces", v, t, m, np.array([0, 1, 2, 0, 2, 1], np.uint32)))  # (the map GLRTX_NORMALS_WELD_POSITIONS makes)
    v, t = _quad()
    v = np.concatenate([v, v[:1] + np.float32(5.0)])  # vertex 6: no triangle names it
    out.append(("7 unnamed vertex", v, t, wobble(v, 7, 0.3), None))
    v, t = mesh([[[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[1, 0, 0], [1, 1, 0.5], [0, 1, 0]]], np.broadcast_to([0.0, 0.0, 1.0], (2, 3, 3)))
    out.append(("8 two corners in one class", v, t, wobble(v, 8, 0.3), np.array([0, 0, 1, 0, 2, 1], np.uint32)))
    v, t = grid(5, 4)
    w = v.copy(); w[:, 3:6] = [0.0, 0.0, -1.0]
    out.append(("9 wound against its normals", w, t, wobble(w, 9), None))
    tm = t.copy(); tm[1::2, 0:3] = tm[1::2][:, [0, 2, 1]]
    out.append(("10 mixed winding", v, tm, wobble(v, 10), None))
    v, t = grid(6, 5)
    out.append(("11 hostile positions", v, t, _hostile_positions(v), None))
    v, t = _quad()
    v[3, 0:3] = _bits_f([0x80000000, 0, 0])  # triangle 1's first corner: -0 where triangle 0's has +0
    out.append(("12 +0 and -0 are not welded", v, t, wobble(v, 12, 0.3), None))
    for n in (1, 63, 64, 65, 255, 256, 257):
        v, t = strip(n)
        out.append((f"13 {n} classes", v, t, wobble(v, 13), None))
    pos, nrm = scenes.icosphere(2, 1.0, (0.0, 0.0, 0.0))
    v, t = mesh(pos, nrm)
    out.append(("14 icosphere(2)", v, t, wobble(v, 14), None))
    pos, nrm, _ = scenes.random_triangles(1000, 15, 4.0)
    v, t = mesh(pos, nrm)
    out.append(("15 random_triangles(1000)", v, t, wobble(v, 15), None))
    v, t = grid(7, 6)
    rng = np.random.default_rng(16)
    out.append(("16 caller-made classes", v, t, wobble(v, 16), rng.integers(0, v.shape[0], v.shape[0]).astype(np.uint32)))
    return out
