"""numpy statement of the deform pass (include/glrtx.h "Deforming"; csrc/skin.hip.h: deform_kernel; host/deform.cpp: glrt_deform_vertices), and the hostile
cases the tests deform.

The rules are skin_math's: every operation is one IEEE float32 operation, correctly rounded, in the contract's order, with denormals read and written as zeros
of their sign (adaptive_math._op); a stored NaN is 0x7FC00000.  From B = [L | t] on the vertex is Posing's, so the tail is skin_math's own functions.  (As
there, a product is rounded on the denormal grid before it is flushed; the hostile cases hold no 2^-126 and no weight times delta that lands just below it.)
"""
from __future__ import annotations

import numpy as np

import skin_math as sm
from adaptive_math import _op, f32
from skin_math import add, canon, div, dot, mul, sub

MAX_TARGETS = 64
_TINY = np.float32(2.0 ** -126)


def active_targets(morph_weights):
    """Indices of the active targets, ascending: |w| >= 2^-126."""
    w = np.asarray(morph_weights, np.float32).reshape(-1)
    return [int(k) for k in np.flatnonzero(np.abs(w) >= _TINY)]


def morph(rest, deltas, morph_weights):
    """(p, n) (n, 3) each: the rest position and normal plus w_k * delta_k over the active targets, a rounded product and a rounded sum a component.  An
    inactive target's deltas are not read."""
    r = np.ascontiguousarray(rest, np.float32).reshape(-1, 15)
    pn = r[:, 0:6].copy()
    if morph_weights is None:
        return pn[:, 0:3], pn[:, 3:6]
    w = np.asarray(morph_weights, np.float32).reshape(-1)
    for k in active_targets(w):
        pn = _op(add, pn, _op(mul, w[k], np.asarray(deltas[k], np.float32).reshape(-1, 6)))
    return pn[:, 0:3], pn[:, 3:6]


def dot4(a, b):
    """((a.w b.w + a.z b.z) + a.y b.y) + a.x b.x over the last axis {x, y, z, w}"""
    return _op(add, _op(add, _op(add, _op(mul, a[..., 3], b[..., 3]), _op(mul, a[..., 2], b[..., 2])), _op(mul, a[..., 1], b[..., 1])),
               _op(mul, a[..., 0], b[..., 0]))


def signs(bones, weights, dualquats):
    """(s (n, 4), h (n, 3)): the weights with the sign of every bone outside bone 0's hemisphere flipped, and the three dot products that decide."""
    q = np.asarray(dualquats, np.float32).reshape(-1, 8)
    b = np.asarray(bones, np.int32).reshape(-1, 4)
    s = np.array(np.asarray(weights, np.float32).reshape(-1, 4), np.float32)
    h = np.zeros((b.shape[0], 3), np.float32)
    for k in range(1, 4):
        h[:, k - 1] = dot4(q[b[:, 0], 0:4], q[b[:, k], 0:4])
        with np.errstate(invalid="ignore"):
            flip = h[:, k - 1] < f32(0)
        s[:, k] = np.where(flip, np.negative(s[:, k]), s[:, k])  # the sign bit, whatever the value
    return s, h


def dualquat_matrix(bones, weights, dualquats):
    """B (n, 3, 4) = [L | t] of the blended, normalised dual quaternion of every vertex."""
    q = np.asarray(dualquats, np.float32).reshape(-1, 8)
    b = np.asarray(bones, np.int32).reshape(-1, 4)
    s, _ = signs(b, weights, q)
    t = [_op(mul, s[:, k, None], q[b[:, k]]) for k in range(4)]
    Q = _op(add, _op(add, _op(add, t[0], t[1]), t[2]), t[3])
    l = _op(np.sqrt, dot4(Q[:, 0:4], Q[:, 0:4]))
    with np.errstate(invalid="ignore"):
        unit = l > f32(0)
    Q = np.where(unit[:, None], _op(div, Q, l[:, None]), Q).astype(np.float32)
    x, y, z, w = Q[:, 0], Q[:, 1], Q[:, 2], Q[:, 3]
    D = Q[:, 4:8]
    xx, yy, zz, xy, xz, yz = _op(mul, x, x), _op(mul, y, y), _op(mul, z, z), _op(mul, x, y), _op(mul, x, z), _op(mul, y, z)
    wx, wy, wz = _op(mul, w, x), _op(mul, w, y), _op(mul, w, z)
    one, two = f32(1), f32(2)
    diag = lambda a, c: _op(sub, one, _op(mul, two, _op(add, a, c)))
    off = lambda fn, a, c: _op(mul, two, _op(fn, a, c))
    B = np.zeros((Q.shape[0], 3, 4), np.float32)
    B[:, 0, 0], B[:, 0, 1], B[:, 0, 2] = diag(yy, zz), off(sub, xy, wz), off(add, xz, wy)
    B[:, 1, 0], B[:, 1, 1], B[:, 1, 2] = off(add, xy, wz), diag(xx, zz), off(sub, yz, wx)
    B[:, 2, 0], B[:, 2, 1], B[:, 2, 2] = off(sub, xz, wy), off(add, yz, wx), diag(xx, yy)
    R = Q[:, 0:4]
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        B[:, i, 3] = _op(mul, two, _op(sub, _op(add, _op(sub, _op(mul, R[:, 3], D[:, i]), _op(mul, D[:, 3], R[:, i])), _op(mul, R[:, j], D[:, k])),
                                       _op(mul, R[:, k], D[:, j])))
    return B


def transform(rest, p, n, B):
    """Posing from B on (skin_math.skin's body), with the morphed position and normal in the rest ones' place."""
    r = np.ascontiguousarray(rest, np.float32).reshape(-1, 15)
    L = B[:, :, :3]
    out = r.copy()  # uv: the words as they are
    t, bn = r[:, 9:12], r[:, 12:15]
    C = sm.cofactor(L)
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


def deform(rest, bones, weights, bone_data, mode=0, deltas=None, morph_weights=None):
    """The deformed vertices (n, 15) float32: morph, then the skinning stage with matrices (mode 0, (n_bones, 12)) or dual quaternions (mode 1, (n_bones, 8))."""
    p, n = morph(rest, deltas, morph_weights)
    B = dualquat_matrix(bones, weights, bone_data) if mode else sm.blend(bones, weights, bone_data)
    return transform(rest, p, n, B)


# ---- the hostile cases
def hostile_dualquats(n_bones, seed):
    """(dualquats (n_bones, 8) float32, form (n_bones,)): bones cycle through six forms -- 0 unit; 1 non-unit; 2 all-zero (the other arm of l > 0); 3 1e20-scaled;
    4 the negative of the previous bone (an antipodal pair); 5 a rotation along one axis of the 4-space of quaternions, so that two such bones along
    different axes have h exactly 0.  Bone 0 is the identity (form 5 along w)."""
    rng = np.random.default_rng(seed)
    q = np.zeros((n_bones, 8), np.float32)
    form = (np.arange(n_bones) + seed) % 6
    form[0] = 5
    for b in range(n_bones):
        r = rng.standard_normal(4)
        r /= np.linalg.norm(r)
        t = rng.standard_normal(3)
        if form[b] == 5:
            r = np.zeros(4)
            r[3 if b == 0 else b % 4] = 1.0
        d = 0.5 * np.array([r[3] * t[0] + t[1] * r[2] - t[2] * r[1], r[3] * t[1] + t[2] * r[0] - t[0] * r[2], r[3] * t[2] + t[0] * r[1] - t[1] * r[0],
                            -(t @ r[:3])])
        a = np.concatenate([r, d]).astype(np.float32)
        if form[b] == 1:
            a = (a * np.float32(rng.uniform(0.3, 3.0))).astype(np.float32)
        elif form[b] == 2:
            a[:] = 0.0
        elif form[b] == 3:
            a = (a * np.float32(1e20)).astype(np.float32)
        elif form[b] == 4:
            a = np.negative(q[b - 1])
        q[b] = a
    return q, form


def hostile_dq_bones(bones, form):
    """The rig's bone indices with every fifth vertex hung on an antipodal pair {b - 1, b} and every fifth on two axis bones (h exactly 0 where the axes
    differ), where the pose has such bones."""
    b = np.array(bones, np.int32)
    anti, axis = np.flatnonzero(form == 4), np.flatnonzero(form == 5)
    for i in range(b.shape[0]):
        if i % 5 == 0 and anti.size:
            a = anti[(i // 5) % anti.size]
            b[i, 0], b[i, 1] = a - 1, a
        elif i % 5 == 1 and axis.size > 1:
            b[i, 0], b[i, 2] = axis[(i // 5) % axis.size], axis[(i // 5 + 1) % axis.size]
    return b


def hostile_morph(n_vert, n_targets, seed):
    """(deltas (n_targets, n_vert, 6), morph_weights (n_targets,)) float32.  Weights cycle through zero, +-denormal (all three inactive), negative, above one and
    ordinary; deltas are small random numbers with a fifth of the entries drawn from skin_math.SPECIAL; every inactive target holds NaN and Inf deltas."""
    rng = np.random.default_rng(seed + 77)
    d = (rng.standard_normal((n_targets, n_vert, 6)) * 0.25).astype(np.float32)
    sp = rng.random(d.shape) < 0.2
    d[sp] = rng.choice(sm.SPECIAL, int(sp.sum()))
    pool = np.array([0.0, 1e-40, -1e-40, -0.75, 1.5, 0.3, -0.0, 2.5], np.float32)
    w = pool[(np.arange(n_targets) + seed) % pool.size].copy()
    if n_targets == 1:
        w[0] = -0.75 if seed % 2 else 0.0
    for k in range(n_targets):
        if abs(w[k]) < _TINY:
            d[k, ::2, :] = np.nan
            d[k, 1::2, :] = np.inf
    return d, w


def hostile_case(n_vert, n_bones, mode, n_targets, seed):
    """(rest, bones, weights, bone_data, deltas, morph_weights) for one point of the grid; deltas and morph_weights are None without targets."""
    rest, bones, weights, mats = sm.hostile_rig(n_vert, n_bones, seed)
    if mode:
        mats, form = hostile_dualquats(n_bones, seed)
        bones = hostile_dq_bones(bones, form)
    data = mats
    if n_targets == 0:
        return rest, bones, weights, data, None, None
    d, w = hostile_morph(n_vert, n_targets, seed)
    return rest, bones, weights, data, d, w
