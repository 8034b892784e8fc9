"""The sparse deform statement (libglrt_host.so: glrt_deform_vertices_sparse, glrt_morph_sparsify) without a GPU: against its numpy statement
(tests/deform_sparse_math.py) bit for bit on the hostile grid and every index pattern; the two relations to the dense form that the header states (include/glrtx.h
"Deforming", SPARSE TARGETS); what glrt_morph_sparsify keeps; every refusal, with the words the device library gives for it (glrtx_debug_deform_sparse makes the
same check before it touches a device, so its message is read here without one); and sets of 65 and 1024 targets going through."""
import ctypes as C

import numpy as np
import pytest

import deform_math as dm
import deform_sparse_math as ds
from glrt_amd import device, host
from test_skin_host import BONES, SIZES


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seed(n_vert, n_bones):
    return 1000 * n_vert + n_bones


def _assert_same(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (f"{what}: {int(bad.any(1).sum())} vertices differ; first {np.argwhere(bad)[0].tolist()}: "
                           f"{got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}")


GRID = [(n, mode) for n in SIZES for mode in (0, 1)]


@pytest.mark.parametrize("n_vert,mode", GRID, ids=[f"{n}v-{'dq' if m else 'mat'}" for n, m in GRID])
def test_equals_numpy_on_hostile_cases(n_vert, mode):
    """n_vert x mode x n_targets in [0, 1, 3, 64, 65, 1024] x the seven index patterns; the bone count goes round BONES with the pattern, and every bone count
    is taken once (deform_sparse_math.grid_cases)."""
    for what, name, rest, bones, weights, data, o, v, d, w in ds.grid_cases(n_vert, mode, BONES):
        got = host.deform_vertices_sparse(rest, bones, weights, data, mode, o, v, d, w)
        _assert_same(got, ds.deform(rest, bones, weights, data, mode, o, v, d, w), what)
        if name == "inactive_nan":  # entries of inactive targets never enter the arithmetic: the output of no targets at all
            assert o[-1] > 0 and np.isnan(d).all()
            _assert_same(got, host.deform_vertices(rest, bones, weights, data, mode), what + ": against no targets")


@pytest.mark.parametrize("mode", [0, 1], ids=["mat", "dq"])
@pytest.mark.parametrize("n_vert", SIZES)
def test_relation_1_all_listed_is_the_dense_form(n_vert, mode):
    """Every target lists every vertex: the dense form's operation sequence, so its bits on any data -- hostile values, NaN and Inf under inactive weights and
    negative zeros included.  n_targets <= 64, the dense statement's cap."""
    for n_bones in BONES:
        for n_targets in (1, 3, 64):
            rest, bones, weights, data, dense, mw = ds.hostile_sparse(n_vert, n_bones, mode, n_targets, _seed(n_vert, n_bones))
            o, v, d, w = ds.pattern("all", dense, mw, 0)
            assert int(o[-1]) == n_targets * n_vert
            _assert_same(host.deform_vertices_sparse(rest, bones, weights, data, mode, o, v, d, w),
                         host.deform_vertices(rest, bones, weights, data, mode, dense, mw), f"{n_bones} bones, {n_targets} targets")


def _away_from_negative_zeros(rest):
    """The rest pose with every position and normal component that is a negative zero or a negative denormal made positive: relation 2's precondition."""
    r = np.array(rest, np.float32)
    u = r[:, 0:6].view(np.uint32)
    bad = ((u & 0x7F800000) == 0) & ((u >> 31) == 1)
    u[bad] &= np.uint32(0x7FFFFFFF)
    return r, int(bad.sum())


@pytest.mark.parametrize("mode", [0, 1], ids=["mat", "dq"])
def test_relation_2_dropping_zero_entries(mode):
    """Dense deltas that are exactly zero (either sign, or denormal) on a random 90 % of the entries: morph_sparsify drops those, and the sparse statement equals
    the dense one bit for bit when no rest position or normal component is a negative zero or a negative denormal.  With one rest component set to -0.0 under
    a dropped entry, that one word differs in its sign bit and in nothing else (shown with matrices, where a bone can be written that carries the sign of p.x
    to the output; a dual quaternion's L01 = 2 (xy - wz) cannot be made -0 beside L02)."""
    n, nb, T = 1000, 5, 16
    rest, bones, weights, data, dense, mw = ds.hostile_sparse(n, nb, mode, T, _seed(n, nb))
    rest, moved = _away_from_negative_zeros(rest)
    assert moved > 0  # the hostile rig did hold some
    rng = np.random.default_rng(12)
    drop = rng.random((T, n)) < 0.9
    zeros = np.array([0.0, -0.0, 1e-40, -1e-40], np.float32)
    dense = dense.copy()
    dense[drop] = zeros[rng.integers(0, 4, (int(drop.sum()), 6))]
    o, v, d = host.morph_sparsify(dense)
    kept = np.array([[ds_kept(dense[k, i]) for i in range(n)] for k in range(T)])
    assert int(o[-1]) == int(kept.sum()) and not kept[drop].any() and 0.05 * T * n < int(o[-1]) < 0.15 * T * n
    ref = host.deform_vertices(rest, bones, weights, data, mode, dense, mw)
    _assert_same(host.deform_vertices_sparse(rest, bones, weights, data, mode, o, v, d, mw), ref, "under the precondition")
    _assert_same(ds.deform(rest, bones, weights, data, mode, o, v, d, mw), ref, "numpy, under the precondition")

    # outside the precondition, matrices: vertex 17 has p = (-0, 1, 1) and its only entry, under an active positive weight, is six +0 -- dropped.  The dense
    # form computes p.x = -0 + w * (+0) = +0, the sparse form keeps -0.  One bone {1, 0, 0, 0} whose matrix has L01 = L02 = t.x = -0, so that
    # x' = ((-0 * 1 + -0 * 1) + 1 * p.x) + -0 keeps p.x's sign: that one output word differs, in its sign bit, and nothing else does.
    if mode:
        return
    k = next(t for t in dm.active_targets(mw) if mw[t] > 0)
    dense2 = np.zeros_like(dense)
    rest2 = rest.copy()
    rest2[:, 0:3] = np.float32(1.0)
    rest2[:, 3:6] = (0.0, 0.0, 1.0)
    i = 17
    rest2[i, 0] = np.float32(-0.0)
    bones2 = np.zeros_like(bones)
    weights2 = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    M = np.array([[1, -0.0, -0.0, -0.0, 0, 1, 0, 0, 0, 0, 1, 0]], np.float32)
    o2, v2, d2 = host.morph_sparsify(dense2)
    assert int(o2[-1]) == 0 and mw[k] > 0
    a = host.deform_vertices(rest2, bones2, weights2, M, 0, dense2, mw)
    b = host.deform_vertices_sparse(rest2, bones2, weights2, M, 0, o2, v2, d2, mw)
    assert np.argwhere(_bits(a) != _bits(b)).tolist() == [[i, 0]]
    assert _bits(a)[i, 0] == 0x00000000 and _bits(b)[i, 0] == 0x80000000
    _assert_same(ds.deform(rest2, bones2, weights2, M, 0, o2, v2, d2, mw), b, "numpy, outside the precondition")
    _assert_same(dm.deform(rest2, bones2, weights2, M, 0, dense2, mw), a, "numpy, the dense form outside the precondition")


def ds_kept(d6):
    return bool((np.asarray(d6, np.float32).view(np.uint32) & 0x7F800000).any())


def test_sparsify_keeps_what_it_says():
    """Denormal-only and zero-only entries are out, entries with one normal number, one NaN or one Inf are in; the counting call and the filling call agree."""
    d = np.zeros((5, 7, 6), np.float32)
    d[0, 1] = (1e-40, -1e-40, 0.0, -0.0, 1e-45, 0.0)  # out
    d[0, 3, 4] = 1.17549435e-38  # 2^-126: the smallest normal number, in
    d[1, 0, 5] = np.nan
    d[1, 6, 0] = -np.inf
    d[3, 2] = (0, 0, 1e-40, 0, 0, 2.5)
    d[3, 5, 1] = np.inf
    # (targets 2 and 4 stay empty)
    o, v, out = host.morph_sparsify(d)
    assert o.tolist() == [0, 1, 3, 3, 5, 5] and v.tolist() == [3, 0, 6, 2, 5]
    assert (_bits(out) == _bits(d[[0, 1, 1, 3, 3], [3, 0, 6, 2, 5]])).all()  # the six floats as they are, the denormal beside 2.5 included
    L = host.lib()
    u64, u32, fp = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    count = np.full(6, 99, np.uint64)
    assert L.glrt_morph_sparsify(d.ctypes.data_as(fp), 5, 7, count.ctypes.data_as(u64), None, None) == 0
    assert count.tolist() == o.tolist()
    o0 = np.full(1, 99, np.uint64)
    assert L.glrt_morph_sparsify(None, 0, 7, o0.ctypes.data_as(u64), None, None) == 0 and o0.tolist() == [0]
    assert L.glrt_morph_sparsify(d.ctypes.data_as(fp), 5, 7, None, None, None) == -1
    assert L.glrt_morph_sparsify(None, 5, 7, count.ctypes.data_as(u64), None, None) == -1
    assert L.glrt_morph_sparsify(d.ctypes.data_as(fp), 1025, 7, count.ctypes.data_as(u64), None, None) == -1
    assert L.glrt_morph_sparsify(d.ctypes.data_as(fp), -1, 7, count.ctypes.data_as(u64), None, None) == -1
    assert L.glrt_morph_sparsify(d.ctypes.data_as(fp), 5, 7, count.ctypes.data_as(u64), v.ctypes.data_as(u32), None) == -1
    big = np.zeros((1024, 3, 6), np.float32)
    big[:, 1, 2] = 1.0
    o, v, out = host.morph_sparsify(big)
    assert o.tolist() == list(range(1025)) and (v == 1).all()


def _refusal_case():
    rest, bones, weights, mats, dense, mw = ds.hostile_sparse(10, 3, 0, 3, 1)
    o, v, d, mw = ds.pattern("random5", dense, mw, 3)
    o, v, d = ds.from_mask(dense, np.array([[1, 0, 1, 0, 0, 0, 1, 0, 0, 1], [0] * 10, [0, 1, 1, 0, 0, 0, 0, 0, 0, 0]], bool))
    return rest, bones, weights, mats, o, v, d, mw


REFUSALS = [
    ("offsets[0]", lambda o, v, d: (np.array([1, 4, 4, 6], np.uint64), v, d), "offsets[0] is 1, not 0"),
    ("decreasing", lambda o, v, d: (np.array([0, 4, 3, 6], np.uint64), v, d), "target 1: offsets decrease from 4 to 3"),
    ("nnz", lambda o, v, d: (np.array([0, 4, 4, 2 ** 31], np.uint64), v, d), "2147483648 entries (at most 2^31 - 1)"),
    ("index", lambda o, v, d: (o, np.array([0, 2, 6, 10, 1, 2], np.uint32), d), "target 0, entry 3: vertex index 10 of 10"),
    ("equal", lambda o, v, d: (o, np.array([0, 2, 6, 9, 2, 2], np.uint32), d), "target 2, entry 1: vertex index 2 after 2, not strictly ascending"),
    ("descending", lambda o, v, d: (o, np.array([0, 6, 2, 9, 1, 2], np.uint32), d), "target 0, entry 2: vertex index 2 after 6, not strictly ascending"),
]


@pytest.mark.parametrize("name,spoil,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_of_the_set(name, spoil, message):
    rest, bones, weights, mats, o, v, d, mw = _refusal_case()
    assert o.tolist() == [0, 4, 4, 6] and v.tolist() == [0, 2, 6, 9, 1, 2]
    host.deform_vertices_sparse(rest, bones, weights, mats, 0, o, v, d, mw)  # the set itself goes through
    o2, v2, d2 = spoil(o, v, d)
    L, D = host.lib(), device.lib()
    fp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), bones.ctypes.data_as(C.POINTER(C.c_int32))
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    out = np.full_like(rest, 7.0)
    args = (fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, o2.ctypes.data_as(u64), v2.ctypes.data_as(u32), fp(d2), fp(mw), 3, fp(out))
    assert L.glrt_deform_vertices_sparse(*args) == -1
    assert D.glrtx_debug_deform_sparse(*args) == -1
    assert message in D.glrtx_last_error(None).decode(), D.glrtx_last_error(None)
    assert (out == 7.0).all()


def test_refusals_of_the_arguments():
    rest, bones, weights, mats, o, v, d, mw = _refusal_case()
    L, D = host.lib(), device.lib()
    fp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), bones.ctypes.data_as(C.POINTER(C.c_int32))
    po, pv = o.ctypes.data_as(C.POINTER(C.c_uint64)), v.ctypes.data_as(C.POINTER(C.c_uint32))
    out = np.zeros_like(rest)
    good = [fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, pv, fp(d), fp(mw), 3, fp(out)]

    def both(pos, value, message=None):
        a = list(good)
        a[pos] = value
        assert L.glrt_deform_vertices_sparse(*a) == -1, pos
        assert D.glrtx_debug_deform_sparse(*a) == -1, pos
        if message:
            assert message in D.glrtx_last_error(None).decode(), D.glrtx_last_error(None)

    assert L.glrt_deform_vertices_sparse(*good) == 0
    for pos in (0, 2, 3, 4, 12):  # rest, bones, weights, bone data, out
        both(pos, None)
    both(5, 0); both(5, 65537)
    both(6, 2, "mode"); both(6, -1, "mode")
    both(7, None, "NULL offsets")
    both(8, None, "NULL vertex or deltas"); both(9, None, "NULL vertex or deltas")
    both(10, None, "NULL morph weights")
    both(11, -1, "-1 sparse morph targets (0 .. 1024)"); both(11, 1025, "1025 sparse morph targets (0 .. 1024)")
    for bad in (np.nan, np.inf, -np.inf):
        w2 = mw.copy(); w2[1] = bad
        both(10, fp(w2), "morph weight")
    for badb in (np.where(bones == 2, 3, bones), np.where(bones == 0, -1, bones)):
        both(2, np.ascontiguousarray(badb, np.int32).ctypes.data_as(C.POINTER(C.c_int32)), "bone")
    # what is no refusal: no targets with no array at all; targets with nnz == 0 and NULL vertex and deltas
    a = list(good); a[7] = a[8] = a[9] = a[10] = None; a[11] = 0
    assert L.glrt_deform_vertices_sparse(*a) == 0
    empty = np.zeros(4, np.uint64)
    a = list(good); a[7] = empty.ctypes.data_as(C.POINTER(C.c_uint64)); a[8] = a[9] = None
    assert L.glrt_deform_vertices_sparse(*a) == 0
    assert (_bits(out) == _bits(host.deform_vertices(rest, bones, weights, mats, 0))).all()


@pytest.mark.parametrize("n_targets", [65, 1024])
def test_more_targets_than_the_dense_cap_go_through(n_targets):
    """All of them active, ordinary deltas, each target a contiguous run of vertices with overlaps: against float64 sums to a few ulps, and against numpy bit
    for bit."""
    n, nb = 300, 5
    rest, bones, weights, data, _, _ = ds.hostile_sparse(n, nb, 0, 0, 9)
    rng = np.random.default_rng(n_targets)
    dense = (rng.standard_normal((n_targets, n, 6)) * 0.01).astype(np.float32)
    first = rng.integers(0, n - 10, n_targets)
    mask = (np.arange(n)[None, :] >= first[:, None]) & (np.arange(n)[None, :] < first[:, None] + 10)
    o, v, d = ds.from_mask(dense, mask)
    mw = rng.uniform(0.1, 1.0, n_targets).astype(np.float32)
    got = host.deform_vertices_sparse(rest, bones, weights, data, 0, o, v, d, mw)
    _assert_same(got, ds.deform(rest, bones, weights, data, 0, o, v, d, mw), f"{n_targets} targets")
    assert (_bits(got) != _bits(host.deform_vertices(rest, bones, weights, data, 0))).any()
