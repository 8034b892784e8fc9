"""numpy statement of the skinning pass (include/glrtx.h "Posing"; csrc/skin.hip.h: skin_kernel; host/deform.cpp: glrt_skin_vertices), and the hostile rigs the
tests pose.

Every operation is one IEEE float32 operation, correctly rounded, in the contract's order, with denormals read and written as zeros of their sign
(adaptive_math._op / ftz).  A NaN that is stored is 0x7FC00000.  (Like every statement built on _op, this one rounds a product on the denormal grid before it
flushes; a product whose exact value lies less than half a denormal step below 2^-126 is the one place where that can differ from hardware that flushes before
it rounds, and the hostile rigs hold no 2^-126 to aim at it.)
"""
from __future__ import annotations

import numpy as np

from adaptive_math import CANONICAL_NAN, _op, f32

mul, add, sub, div = np.multiply, np.add, np.subtract, np.divide


def dot(a0, a1, a2, vx, vy, vz):
    """(a2 v.z + a1 v.y) + a0 v.x"""
    return _op(add, _op(add, _op(mul, a2, vz), _op(mul, a1, vy)), _op(mul, a0, vx))


def canon(x):
    x = np.asarray(x, np.float32)
    return np.where(np.isnan(x), CANONICAL_NAN.view(np.float32), x).astype(np.float32)


def blend(bones, weights, matrices):
    """B (n, 3, 4): ((w0 M_b0 + w1 M_b1) + w2 M_b2) + w3 M_b3, entry by entry."""
    m = np.asarray(matrices, np.float32).reshape(-1, 3, 4)
    b = np.asarray(bones, np.int32).reshape(-1, 4)
    w = np.asarray(weights, np.float32).reshape(-1, 4)
    t = [_op(mul, w[:, k, None, None], m[b[:, k]]) for k in range(4)]
    return _op(add, _op(add, _op(add, t[0], t[1]), t[2]), t[3])


def cofactor(L):
    """C (n, 3, 3) of L (n, 3, 3): C[i][j] = L[i+1][j+1] L[i+2][j+2] - L[i+1][j+2] L[i+2][j+1], indices mod 3."""
    C = np.zeros_like(L)
    for i in range(3):
        x, y = L[:, (i + 1) % 3], L[:, (i + 2) % 3]
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            C[:, i, j] = _op(sub, _op(mul, x[:, j1], y[:, j2]), _op(mul, x[:, j2], y[:, j1]))
    return C


def skin(rest, bones, weights, matrices):
    """The posed vertices (n, 15) float32 of rest (n, 15), bones (n, 4) int32, weights (n, 4), matrices (n_bones, 12)."""
    r = np.ascontiguousarray(rest, np.float32).reshape(-1, 15)
    B = blend(bones, weights, matrices)
    L = B[:, :, :3]
    out = r.copy()  # uv: the words as they are
    p, n, t, bn = r[:, 0:3], r[:, 3:6], r[:, 9:12], r[:, 12:15]
    C = cofactor(L)
    v = np.zeros((r.shape[0], 3), np.float32)
    for i in range(3):
        out[:, i] = canon(_op(add, dot(L[:, i, 0], L[:, i, 1], L[:, i, 2], p[:, 0], p[:, 1], p[:, 2]), B[:, i, 3]))
        v[:, i] = dot(C[:, i, 0], C[:, i, 1], C[:, i, 2], n[:, 0], n[:, 1], n[:, 2])
        out[:, 9 + i] = canon(dot(L[:, i, 0], L[:, i, 1], L[:, i, 2], t[:, 0], t[:, 1], t[:, 2]))
        out[:, 12 + i] = canon(dot(L[:, i, 0], L[:, i, 1], L[:, i, 2], bn[:, 0], bn[:, 1], bn[:, 2]))
    s = dot(v[:, 0], v[:, 1], v[:, 2], v[:, 0], v[:, 1], v[:, 2])
    l = _op(np.sqrt, s)
    with np.errstate(invalid="ignore"):
        unit = l > f32(0)
    for i in range(3):
        out[:, 3 + i] = canon(np.where(unit, _op(div, v[:, i], l), v[:, i]))
    return out


SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1e30, -1e30, np.nan, np.inf, -np.inf, 1.0, -1.0, 1e-30, 3e38], np.float32)


def hostile_rig(n_vert, n_bones, seed):
    """(rest (n, 15), bones (n, 4) int32, weights (n, 4), matrices (n_bones, 12)) float32: a rig meant to break a careless statement.
    Vertices cycle through eight kinds -- ordinary convex weights; weights that do not sum to one; negative weights; zero weights; denormal weights; all four
    bones the same; special rest positions (0, -0, denormal, 1e30, NaN, Inf); zero and denormal normals (the other arm of l > 0).  Matrices cycle through a
    rotation with translation, zero scale, a reflection, a shear, 1e20 entries and plain random ones."""
    rng = np.random.default_rng(seed)
    rest = rng.standard_normal((n_vert, 15)).astype(np.float32)
    nrm = rest[:, 3:6]
    rest[:, 3:6] = nrm / np.maximum(np.linalg.norm(nrm, axis=1, keepdims=True), 1e-6).astype(np.float32)
    bones = rng.integers(0, n_bones, (n_vert, 4)).astype(np.int32)
    w = rng.random((n_vert, 4)).astype(np.float32)
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    kind = (np.arange(n_vert) + seed) % 8
    k = kind == 1
    w[k] = (rng.random((int(k.sum()), 4)) * 3.0).astype(np.float32)
    k = kind == 2
    w[k] = rng.standard_normal((int(k.sum()), 4)).astype(np.float32)
    k = kind == 3
    w[k] = np.where(rng.random((int(k.sum()), 4)) < 0.6, 0.0, w[k]).astype(np.float32)
    k = np.flatnonzero(kind == 3)[::2]
    w[k] = 0.0
    k = kind == 4
    w[k] = (rng.choice(np.array([1e-40, -1e-40, 1e-45, 0.5], np.float32), (int(k.sum()), 4))).astype(np.float32)
    k = kind == 5
    bones[k] = bones[k][:, :1]
    k = np.flatnonzero(kind == 6)
    rest[k[:, None], rng.integers(0, 3, (k.size, 1))] = rng.choice(SPECIAL, (k.size, 1))
    rest[k[::3], 0:3] = rng.choice(SPECIAL, (k[::3].size, 3))
    rest[k[1::3], 9:15] = rng.choice(SPECIAL, (k[1::3].size, 6))
    rest[k[2::3], 6:9] = rng.choice(SPECIAL, (k[2::3].size, 3))  # uv: moved as words, denormals and NaN payloads kept
    k = np.flatnonzero(kind == 7)
    rest[k, 3:6] = rng.choice(np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30], np.float32), (k.size, 3))
    if n_vert > 2:
        rest[n_vert // 2, 6] = np.uint32(0x7FA00001).view(np.float32)  # a signalling NaN with a payload in uv
    mats = np.zeros((n_bones, 3, 4), np.float32)
    for b in range(n_bones):
        form = (b + seed) % 6
        a = rng.standard_normal((3, 4)).astype(np.float32)
        if form == 0:
            th = rng.random() * 6.28
            c, s = np.cos(th), np.sin(th)
            a[:, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64).astype(np.float32)
        elif form == 1:
            a[:, :3] = 0.0
            if b % 2:
                a[:, :3] = np.diag([1.0, 0.0, 1.0]).astype(np.float32)
        elif form == 2:
            a[:, :3] = np.diag([1.0, -1.0, 1.0]).astype(np.float32)
        elif form == 3:
            a[:, :3] = np.array([[1, 2.5, 0], [0, 1, 0], [0.25, 0, 1]], np.float32)
        elif form == 4:
            a = (a * np.float32(1e20)).astype(np.float32)
        mats[b] = a
    return rest, bones, np.ascontiguousarray(w, np.float32), mats.reshape(n_bones, 12)
