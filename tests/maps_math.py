"""numpy statement of the material maps (include/glrtx.h "Material maps"; csrc/maps.hip.h; host/maps.cpp: glrt_map_decode, glrt_map_normal, glrt_map_alpha), in
tests/adaptive_math.py's _op / ftz: one rounded fp32 operation at a time, denormals as zeros of their sign into and out of every operation.  Kept words and
inverted sign bits are integer moves.

Records are (k, 18) float32: {n, e1, e2, (s0, t0), (s1, t1), (s2, t2), m}, m the decoded texel.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import _op, ftz

ALPHA_MIN = np.float32(1e-3)  # GLRTX_MAP_ALPHA_MIN
RECORD_FLOATS = 18
add, sub, mul, div = np.add, np.subtract, np.multiply, np.divide
_SIGN = np.uint32(0x80000000)
_EXP = np.uint32(0x7F800000)


def _u(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def dot(a, b):
    """(a.x b.x + a.y b.y) + a.z b.z over the last axis."""
    return _op(add, _op(add, _op(mul, a[..., 0], b[..., 0]), _op(mul, a[..., 1], b[..., 1])), _op(mul, a[..., 2], b[..., 2]))


def rsq(x):
    return _op(div, np.float32(1), _op(np.sqrt, x))


def tiny(x):
    return (_u(x) & _EXP) == 0


def finite(x):
    return (_u(x) & _EXP) != _EXP


def pos_finite(x):
    return (_u(x) - np.uint32(0x00800000)) < np.uint32(0x7F000000)


def neg_where(x, flip):
    """x with its sign bits inverted where flip (k,) holds."""
    return (_u(x) ^ np.where(flip[:, None], _SIGN, np.uint32(0))).view(np.float32)


def decode(rgb):
    c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)
    return _op(add, _op(mul, c, np.float32(2)), np.float32(-1))


def alpha(rgb):
    c = np.ascontiguousarray(rgb, np.float32).reshape(-1, 3)[:, 0:2]
    with np.errstate(invalid="ignore"):
        return np.where(ftz(c) > ALPHA_MIN, c, ALPHA_MIN).astype(np.float32)


def normal(records, scale=1.0):
    r = np.ascontiguousarray(records, np.float32).reshape(-1, RECORD_FLOATS)
    n, e1, e2, st0, st1, st2, m = r[:, 0:3], r[:, 3:6], r[:, 6:9], r[:, 9:11], r[:, 11:13], r[:, 13:15], r[:, 15:18]
    scale = np.float32(scale)
    col = lambda v: v[:, None]
    with np.errstate(all="ignore"):
        a, b = _op(mul, m[:, 0], scale), _op(mul, m[:, 1], scale)
        keep = tiny(a) & tiny(b)
        ds1, ds2 = _op(sub, st1[:, 0], st0[:, 0]), _op(sub, st2[:, 0], st0[:, 0])
        dt1, dt2 = _op(sub, st1[:, 1], st0[:, 1]), _op(sub, st2[:, 1], st0[:, 1])
        det = _op(sub, _op(mul, ds1, dt2), _op(mul, ds2, dt1))
        keep |= tiny(det) | ~finite(det)
        Tr = _op(sub, _op(mul, e1, col(dt2)), _op(mul, e2, col(dt1)))
        Br = _op(sub, _op(mul, e2, col(ds1)), _op(mul, e1, col(ds2)))
        Tr, Br = neg_where(Tr, det < 0), neg_where(Br, det < 0)
        k = dot(n, Tr)
        Tp = _op(sub, Tr, _op(mul, col(k), n))
        l2 = dot(Tp, Tp)
        keep |= ~pos_finite(l2)
        T = _op(mul, Tp, col(rsq(l2)))
        x, y, z = 0, 1, 2
        C = np.stack([_op(sub, _op(mul, n[:, y], T[:, z]), _op(mul, n[:, z], T[:, y])),
                      _op(sub, _op(mul, n[:, z], T[:, x]), _op(mul, n[:, x], T[:, z])),
                      _op(sub, _op(mul, n[:, x], T[:, y]), _op(mul, n[:, y], T[:, x]))], -1).astype(np.float32)
        B = neg_where(C, dot(C, Br) < 0)
        p = _op(add, _op(add, _op(mul, col(a), T), _op(mul, col(b), B)), _op(mul, col(m[:, 2]), n))
        q = dot(p, p)
        keep |= ~pos_finite(q)
        out = _op(mul, p, col(rsq(q)))
    return np.where(keep[:, None], _u(n), _u(out)).view(np.float32)
