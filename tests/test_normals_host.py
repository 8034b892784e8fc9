"""The normal rebuild's CPU statements (libglrt_host.so: glrt_normal_topology, glrt_rebuild_normals, glrt_positions_to_vertices; include/glrtx.h "Rebuilding
normals") without a GPU: against the numpy statement (tests/normals_math.py) word for word on every case of tests/normals_cases.py; the class map against a
dictionary-built one; the weld rule on the headline's rest pose; weld-by-position on a box; and every refusal."""
import ctypes as C

import numpy as np
import pytest

import normals_cases as nc
import normals_math as nm
from glrt_amd import host, scenes

CASES = nc.cases()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _verts(scene):
    return np.ascontiguousarray(np.asarray(scene["vert"], np.float32).reshape(-1, 15))


def _tris(scene):
    return np.ascontiguousarray(np.asarray(scene["tri"], np.float32).reshape(-1, 4))


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_statements_equal_numpy_word_for_word(case):
    name, rest, tri, moved, class_map = case
    cls, flip, n = host.normal_topology(rest, tri)
    cls2, flip2, n2 = nm.topology(rest, tri)
    assert cls.dtype == np.uint32 and flip.dtype == np.uint8
    assert cls.tolist() == cls2.tolist() and flip.tolist() == flip2.tolist() and n == n2 == len(set(cls.tolist())), name
    if class_map is not None:
        cls = class_map
    got = host.rebuild_normals(moved, tri, cls, flip)
    ref = nm.rebuild(moved, tri, cls, flip)
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{name}: {int(bad.any(1).sum())} vertices differ; first {np.argwhere(bad)[0].tolist()}"
    keep = np.r_[0:3, 6:15]
    assert (_bits(got)[:, keep] == _bits(moved)[:, keep]).all(), f"{name}: a word other than a normal's changed"
    # every member of a class holds the same three words, unless the class kept its own
    changed = (_bits(got)[:, 3:6] != _bits(moved)[:, 3:6]).any(1)
    for k in np.unique(np.asarray(cls)[changed]):
        words = _bits(got)[np.asarray(cls) == k, 3:6]
        assert (words == words[0]).all(), (name, int(k))


def _case(prefix):
    return next(c for c in CASES if c[0].startswith(prefix))


def test_what_each_case_is_there_for():
    # 2 / 3: the quad welds two corners, the crease none
    assert host.normal_topology(*_case("2 ")[1:3])[2] == 4 and host.normal_topology(*_case("3 ")[1:3])[2] == 6
    # 4: the hub's list is the whole fan, and the chunk rule is visible: a plain sequential sum over 1000 faces gives other bits
    for n in (256, 257, 1000):
        _, rest, tri, moved, _ = _case(f"4 fan of {n}")
        cls, flip, _ = host.normal_topology(rest, tri)
        lists = nm.face_lists(tri, cls)
        assert len(lists[0]) == n and max(map(len, lists[1:])) == 2
    fv = nm.face_vectors(moved[:, 0:3], tri[:, 0:3].astype(np.int64))
    s = fv[0].copy()
    for f in fv[1:]:
        s = nm._op(nm.add, s, f)
    plain = nm._op(nm.div, s, nm._op(np.sqrt, nm.dot(s, s)))
    got = host.rebuild_normals(moved, tri, cls, flip)
    assert (_bits(plain) != _bits(got[0, 3:6])).any(), "the 1000-face fan does not tell the chunked sum from a sequential one"
    # 5, 6, 7: kept words
    for prefix in ("5 ", "6 "):
        _, rest, tri, moved, class_map = _case(prefix)
        cls, flip, _ = host.normal_topology(rest, tri)
        assert not flip.any()
        out = host.rebuild_normals(moved, tri, cls if class_map is None else class_map, flip)
        assert (_bits(out) == _bits(moved)).all(), prefix
    _, rest, tri, moved, class_map = _case("6 ")
    assert host.normal_topology(rest, tri, host.NORMALS_WELD_POSITIONS)[0].tolist() == class_map.tolist()
    assert host.normal_topology(rest, tri)[2] == 6  # by position and normal the two faces share nothing
    _, rest, tri, moved, _ = _case("7 ")
    cls, flip, _ = host.normal_topology(rest, tri)
    out = host.rebuild_normals(moved, tri, cls, flip)
    assert (_bits(out[6]) == _bits(moved[6])).all() and (_bits(out[:6, 3:6]) != _bits(moved[:6, 3:6])).any()
    # 8: triangle 0 has two corners in class 0 and is listed there once
    _, rest, tri, moved, class_map = _case("8 ")
    assert nm.face_lists(tri, class_map)[0] == [0, 1]
    # 9 / 10: flipped faces; the rebuilt normals stay on the authored side
    _, rest, tri, moved, _ = _case("9 ")
    cls, flip, _ = host.normal_topology(rest, tri)
    assert flip.all() and (host.rebuild_normals(moved, tri, cls, flip)[:, 5] < -0.5).all()
    _, rest, tri, moved, _ = _case("10 ")
    cls, flip, _ = host.normal_topology(rest, tri)
    assert 0 < flip.sum() < flip.size and (host.rebuild_normals(moved, tri, cls, flip)[:, 5] > 0.5).all()
    # 11: NaN goes through as the canonical NaN, and the case holds some
    _, rest, tri, moved, _ = _case("11 ")
    cls, flip, _ = host.normal_topology(rest, tri)
    out = host.rebuild_normals(moved, tri, cls, flip)
    nan = np.isnan(out[:, 3:6])
    assert nan.any() and not nan.all() and (_bits(out[:, 3:6])[nan] == 0x7FC00000).all()
    # 12: +0 and -0
    _, rest, tri, _, _ = _case("12 ")
    cls, _, n = host.normal_topology(rest, tri)
    assert n == 5 and cls[3] != cls[0] and cls[4] == cls[2]
    # 13: the class counts; 14: classes of 5 and of 6 members; 15: singletons
    for k in (1, 63, 64, 65, 255, 256, 257):
        assert host.normal_topology(*_case(f"13 {k} classes")[1:3])[2] == k
    cls, _, n = host.normal_topology(*_case("14 ")[1:3])
    assert n == 162 and np.bincount(np.bincount(cls)).tolist() == [0, 0, 0, 0, 0, 12, 150]
    cls, _, n = host.normal_topology(*_case("15 ")[1:3])
    assert n == 3000 and cls.tolist() == list(range(3000))


def test_class_map_equals_a_dictionary_built_one():
    scene, _ = scenes.config_c1(64, 48, max_depth=4, subdiv=2)
    rest, tri = _verts(scene), _tris(scene)
    for flags, words in ((0, 6), (host.NORMALS_WELD_POSITIONS, 3)):
        cls, _, n = host.normal_topology(rest, tri, flags)
        seen = {}
        ref = [seen.setdefault(tuple(w), len(seen)) for w in _bits(rest)[:, :words].tolist()]
        assert cls.tolist() == ref and n == len(seen)
        first = [int(np.flatnonzero(cls == k)[0]) for k in range(n)]
        assert first == sorted(first)  # ids ascend with each class's smallest member


def test_headline_rest_pose():
    scene, _ = scenes.config_headline(64, 36)
    rest, tri = _verts(scene), _tris(scene)
    cls, flip, n = host.normal_topology(rest, tri)
    assert rest.shape[0] == 30756 and n == 5160 and int(np.bincount(cls).max()) == 6 and not flip.any()


def test_weld_positions_welds_a_boxs_corners():
    pos, nrm = scenes.box((-1.0, -1.0, -1.0), (1.0, 2.0, 3.0))
    rest, tri = nc.mesh(pos, nrm)
    assert rest.shape[0] == 36
    cls, flip, n = host.normal_topology(rest, tri)
    assert n == 24 and not flip.any()  # a corner per face: the normals differ
    cls, flip, n = host.normal_topology(rest, tri, host.NORMALS_WELD_POSITIONS)
    assert n == 8 and not flip.any()
    out = host.rebuild_normals(rest, tri, cls, flip)
    d = out[:, 3:6] * np.sign(rest[:, 0:3] - np.array([0.0, 0.5, 1.0], np.float32))
    assert (d > 0).all()  # every corner normal points out of the box along all three axes


def test_positions_to_vertices():
    _, rest, tri, moved, _ = _case("11 ")
    out = host.positions_to_vertices(rest, moved[:, 0:3])
    assert (_bits(out) == _bits(nm.positions_to_vertices(rest, moved[:, 0:3]))).all()
    assert (_bits(out[:, 0:3]) == _bits(moved[:, 0:3])).all() and (_bits(out[:, 3:]) == _bits(rest[:, 3:])).all()


def test_refusals():
    L = host.lib()
    fp, u32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
    _, rest, tri, moved, _ = _case("2 ")
    n, nt = rest.shape[0], tri.shape[0]
    cls, flip = np.zeros(n, np.uint32), np.zeros(nt, np.uint8)
    P = lambda a, t: a.ctypes.data_as(t)

    def topo(r=rest, t=tri, n_vert=n, n_tri=nt, flags=0, c=cls, f=flip):
        return L.glrt_normal_topology(None if r is None else P(r, fp), n_vert, None if t is None else P(t, fp), n_tri, flags, None if c is None else P(c, u32p),
                                      None if f is None else P(f, u8p), None)

    def rebuild(v, t=tri, n_vert=n, n_tri=nt, c=cls, f=flip):
        return L.glrt_rebuild_normals(None if v is None else P(v, fp), n_vert, None if t is None else P(t, fp), n_tri, None if c is None else P(c, u32p),
                                      None if f is None else P(f, u8p))

    assert topo() == 0
    assert topo(r=None) == -1 and topo(t=None) == -1 and topo(c=None) == -1 and topo(f=None) == -1
    assert topo(flags=2) == -1 and topo(flags=3) == -1 and topo(flags=1) == 0
    assert topo(n_tri=2 ** 31) == -1  # (refused before a triangle is read)
    for bad in (float(n), -1.0, 0.5, np.nan, np.inf, 3e9):
        t = tri.copy(); t[1, 2] = bad
        assert topo(t=t) == -1, bad
        assert rebuild(moved.copy(), t=t) == -1, bad
    t = tri.copy(); t[1, 3] = np.nan  # (the material is not a corner)
    assert topo(t=t) == 0
    assert topo(n_vert=0, n_tri=0) == 0 and topo(r=None, t=None, n_vert=0, n_tri=0, c=None, f=None) == 0
    work = moved.copy()
    assert rebuild(work) == 0
    assert rebuild(None) == -1 and rebuild(work, t=None) == -1 and rebuild(work, c=None) == -1 and rebuild(work, f=None) == -1
    before = work.copy()
    c = cls.copy(); c[4] = n
    assert rebuild(work, c=c) == -1 and (_bits(work) == _bits(before)).all()
    c[4] = n - 1
    assert rebuild(work, c=c) == 0
    assert L.glrt_positions_to_vertices(None, P(rest, fp), n, P(work, fp)) == -1 and L.glrt_positions_to_vertices(P(rest, fp), None, n, P(work, fp)) == -1
    assert L.glrt_positions_to_vertices(P(rest, fp), P(rest, fp), n, None) == -1
