"""numpy statement of the normal rebuild (include/glrtx.h "Rebuilding normals"; csrc/normals.hip.h; host/normals.cpp: glrt_normal_topology,
glrt_rebuild_normals, glrt_positions_to_vertices), in tests/adaptive_math.py's _op / ftz: one rounded fp32 operation at a time, denormals as zeros of their sign
into and out of every operation, a stored NaN as 0x7FC00000.

Vertices are (n, 15) float32 wire records {pos, normal, uv, tangent, binormal}; triangles (n_tri, 4) float32 {i0, i1, i2, material}.
"""
from __future__ import annotations

import numpy as np

from adaptive_math import CANONICAL_NAN, _op

WELD_POSITIONS = 1  # GLRTX_NORMALS_WELD_POSITIONS
CHUNK = 256  # GLRTX_NORMAL_CHUNK

add, sub, mul, div = np.add, np.subtract, np.multiply, np.divide


def _verts(v):
    return np.ascontiguousarray(v, np.float32).reshape(-1, 15)


def _corners(tri):
    return np.ascontiguousarray(tri, np.float32).reshape(-1, 4)[:, 0:3].astype(np.int64)


def dot(a, b):
    """(a.z b.z + a.y b.y) + a.x b.x over the last axis."""
    return _op(add, _op(add, _op(mul, a[..., 2], b[..., 2]), _op(mul, a[..., 1], b[..., 1])), _op(mul, a[..., 0], b[..., 0]))


def face_vectors(pos, corners):
    """f = e1 x e2 with e1 = p[i1] - p[i0], e2 = p[i2] - p[i0]: two rounded products and one subtraction a component.  (n_tri, 3) float32."""
    p0, p1, p2 = pos[corners[:, 0]], pos[corners[:, 1]], pos[corners[:, 2]]
    e1, e2 = _op(sub, p1, p0), _op(sub, p2, p0)
    x, y, z = 0, 1, 2
    return np.stack([_op(sub, _op(mul, e1[:, y], e2[:, z]), _op(mul, e1[:, z], e2[:, y])),
                     _op(sub, _op(mul, e1[:, z], e2[:, x]), _op(mul, e1[:, x], e2[:, z])),
                     _op(sub, _op(mul, e1[:, x], e2[:, y]), _op(mul, e1[:, y], e2[:, x]))], -1).astype(np.float32).reshape(-1, 3)


def weld(rest, flags=0):
    """(class_of_vertex (n,) uint32, n_classes): equal 32-bit patterns of the six position and normal words (three with WELD_POSITIONS); ids ascend with each
    class's smallest member."""
    w = _verts(rest).view(np.uint32)[:, 0:(3 if flags & WELD_POSITIONS else 6)]
    seen, cls = {}, np.zeros(w.shape[0], np.uint32)
    for i, key in enumerate(map(bytes, w)):
        cls[i] = seen.setdefault(key, len(seen))
    return cls, len(seen)


def flips(rest, tri):
    """(n_tri,) uint8: 1 iff dot(f, m) < 0 in the rest pose, m = (n0 + n1) + n2 over the corners' rest normals.  A NaN or a zero does not flip."""
    r, c = _verts(rest), _corners(tri)
    f = face_vectors(r[:, 0:3], c)
    n = r[:, 3:6]
    m = _op(add, _op(add, n[c[:, 0]], n[c[:, 1]]), n[c[:, 2]]).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        return (dot(f, m) < 0).astype(np.uint8)


def topology(rest, tri, flags=0):
    """glrt_normal_topology: (class_of_vertex, flip, n_classes)."""
    cls, n = weld(rest, flags)
    return cls, flips(rest, tri), n


def face_lists(tri, class_of_vertex):
    """Per class id (0 .. max id), the triangles with at least one corner in the class, each once, ascending."""
    c = _corners(tri)
    cls = np.asarray(class_of_vertex, np.int64)
    lists = [[] for _ in range(int(cls.max()) + 1 if cls.size else 0)]
    for t in range(c.shape[0]):
        for k in sorted(set(cls[c[t]].tolist())):
            lists[k].append(t)
    return lists


def rebuild(vert, tri, class_of_vertex, flip):
    """glrt_rebuild_normals: a copy of vert with the normal words rebuilt.  The sum of a class runs over its list in chunks of CHUNK entries: inside a chunk
    c = f_first, c = c + f_next; across chunks s = c_0, s = s + c_k.  l = sqrt(dot(s, s)); l == 0 keeps the words; else n = s / l, a NaN as 0x7FC00000."""
    v = _verts(vert).copy()
    fv = face_vectors(v[:, 0:3], _corners(tri)).view(np.uint32)
    fv = (fv ^ np.where(np.asarray(flip, np.uint8).reshape(-1, 1) != 0, np.uint32(0x80000000), np.uint32(0))).view(np.float32)
    cls = np.asarray(class_of_vertex, np.int64)
    for k, faces in enumerate(face_lists(tri, cls)):
        s = np.zeros(3, np.float32)
        for e0 in range(0, len(faces), CHUNK):
            c = fv[faces[e0]].copy()
            for t in faces[e0 + 1:e0 + CHUNK]:
                c = _op(add, c, fv[t])
            s = c if e0 == 0 else _op(add, s, c)
        l = _op(np.sqrt, dot(s, s))
        if l == 0:  # (a NaN is not: it goes through)
            continue
        n = _op(div, s, l).astype(np.float32).view(np.uint32)
        n = np.where(np.isnan(n.view(np.float32)), CANONICAL_NAN, n)
        v.view(np.uint32)[cls == k, 3:6] = n
    return v


def positions_to_vertices(rest, pos):
    """glrt_positions_to_vertices: the rest records with their position words replaced, moved as integers."""
    v = _verts(rest).copy()
    v.view(np.uint32)[:, 0:3] = np.ascontiguousarray(pos, np.float32).reshape(-1, 3).view(np.uint32)
    return v
