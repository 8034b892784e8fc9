"""glrt_map_normal / glrt_map_decode / glrt_map_alpha (host/maps.cpp) against the numpy statement (tests/maps_math.py), bit for bit, on tests/maps_cases.py's
batch, and the properties the contract promises of the rule (include/glrtx.h "Material maps")."""
import numpy as np
import pytest

import maps_cases
import maps_math
from conftest import bits


def host():
    from glrt_amd import host as h
    return h


def ulp_distance(a, b):
    return np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))


@pytest.mark.parametrize("scale", maps_cases.SCALES)
def test_map_normal_equals_the_numpy_statement(scale):
    rec = maps_cases.batch()
    got, want = host().map_normal(rec, scale), maps_math.normal(rec, scale)
    bad = np.argwhere((bits(got) != bits(want)).any(1)).ravel()
    assert bad.size == 0, (scale, bad[:8], got[bad[:2]], want[bad[:2]])


def test_the_edge_cases_keep_or_change_the_normal_as_the_contract_says():
    rec = maps_cases.edge_records()
    out = host().map_normal(rec, 1.0)
    kept = (bits(out) == bits(rec[:, 0:3])).all(1)
    # rows of edge_records(): 0 plain; 1-2 det 0; 3-4 det < 0; 5-8 det not finite; 9-10 n parallel to Tr; 11-13 flat; 14 m.z = 0; 15 m zero; 16 b only;
    # 17 denormal a, b; 18-21 non-finite texels; 22 q overflows; 23 q underflows; 24-25 a NaN / inf normal; 26 a zero normal; 27 degenerate triangle; 28 denormal edge (a zero under the flush: Tr = 0);
    # 29 l2 overflows; 30 det underflows
    expect_kept = {1, 2, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 17, 18, 19, 20, 21, 22, 23, 24, 25, 27, 28, 29, 30}
    assert set(np.flatnonzero(kept).tolist()) == expect_kept, sorted(set(np.flatnonzero(kept).tolist()) ^ expect_kept)
    assert np.isfinite(out[~kept]).all()
    # a scale of 0 keeps everything
    assert (bits(host().map_normal(maps_cases.batch(), 0.0)) == bits(maps_cases.batch()[:, 0:3])).all()


def test_decode_and_alpha_equal_the_numpy_statement():
    rng = np.random.default_rng(3)
    c = rng.uniform(-0.5, 1.5, (256, 3)).astype(np.float32)
    c[:12] = np.array([[0.5, 0.5, 1.0], [0, 0, 0], [1, 1, 1], [np.nan, 0.2, 0.3], [np.inf, -np.inf, 0.1], [1e-3, 1e-3, 0], [9.9e-4, 1.0001e-3, 0],
                       [1e-41, -1e-41, 1e-41], [-0.0, 0.0, 0.5], [-1, -2, -3], [0.05, 0.5, np.nan], [3e38, 1e-38, 0]], np.float32)
    assert (bits(host().map_decode(c)) == bits(maps_math.decode(c))).all()
    a = host().map_alpha(c)
    assert (bits(a) == bits(maps_math.alpha(c))).all()
    assert (a >= np.float32(1e-3)).all() and a[3, 0] == np.float32(1e-3) and a[6].tolist() == [np.float32(1e-3), np.float32(1.0001e-3)]
    assert host().map_decode([[0.5, 0.5, 1.0]]).tolist() == [[0.0, 0.0, 1.0]]  # the flat texel decodes to (0, 0, 1) exactly


def test_a_flat_map_returns_the_input_words():
    rec = maps_cases.random_records(256, seed=11)
    rec[:, 15:18] = np.float32([0.0, 0.0, 1.0])
    rec[::2, 15] = np.float32(-0.0)
    for scale in (1.0, -3.0, 0.0):
        assert (bits(host().map_normal(rec, scale)) == bits(rec[:, 0:3])).all()


def test_the_result_is_a_unit_vector_within_2_ulp():
    rec = maps_cases.random_records(2048, seed=5)
    out = host().map_normal(rec, 1.0).astype(np.float64)
    changed = (bits(out.astype(np.float32)) != bits(rec[:, 0:3])).any(1)
    assert changed.mean() > 0.99
    l = np.sqrt((out[changed] ** 2).sum(1)).astype(np.float32)
    # p * rsq(q): sqrt and the reciprocal are correctly rounded (half an ulp each), the three products another half each: |n'| is within 2 ulp of 1
    assert ulp_distance(l, np.ones_like(l)).max() <= 2, ulp_distance(l, np.ones_like(l)).max()


def test_translating_the_coordinates_changes_nothing():
    rec = maps_cases.random_records(512, seed=9)
    # coordinates on a grid of 1/64 and a shift that is a multiple of it: every difference s1 - s0 is exact before and after
    rec[:, 9:15] = np.round(rec[:, 9:15] * 64) / 64
    moved = rec.copy()
    moved[:, 9:15:2] += np.float32(3.25)
    moved[:, 10:15:2] += np.float32(-1.5)
    assert (bits(host().map_normal(rec, 1.0)) == bits(host().map_normal(moved, 1.0))).all()


def test_mirroring_s_mirrors_the_tangent_component():
    """The handedness case: with s running the other way across the same triangle the tangent turns round, the bitangent stays: (m.x, m.y, m.z) on the mirrored
    triangle is (-m.x, m.y, m.z) on the original, bit for bit."""
    rec = maps_cases.random_records(512, seed=13)
    mirrored = rec.copy()
    mirrored[:, 9:15:2] = -rec[:, 9:15:2]
    flipped = rec.copy()
    flipped[:, 15] = -rec[:, 15]
    assert (bits(host().map_normal(mirrored, 1.0)) == bits(host().map_normal(flipped, 1.0))).all()


def test_the_quad_tilts_towards_plus_s():
    """The quad y = 0 with s along +x and t along -z: m = (sin th, 0, cos th) gives (sin th, cos th, 0) to 1e-6, on both of its triangles."""
    th = np.linspace(-1.4, 1.4, 57)
    m = np.stack([np.sin(th), np.zeros_like(th), np.cos(th)], 1)
    k = len(th)
    n = np.tile([0.0, 1.0, 0.0], (k, 1))
    want = np.stack([np.sin(th), np.cos(th), np.zeros_like(th)], 1)
    # triangle (a, b, c): a = (0, 0, 0) st (0, 0), b = (2, 0, 0) st (1, 0), c = (2, 0, -2) st (1, 1); triangle (a, c, d): d = (0, 0, -2) st (0, 1)
    for e1, e2, st1, st2 in (((2, 0, 0), (2, 0, -2), (1, 0), (1, 1)), ((2, 0, -2), (0, 0, -2), (1, 1), (0, 1))):
        rec = host().map_records(n, np.tile(e1, (k, 1)), np.tile(e2, (k, 1)), np.zeros((k, 2)), np.tile(st1, (k, 1)), np.tile(st2, (k, 1)), m)
        got = host().map_normal(rec, 1.0)
        assert np.abs(got - want).max() <= 1e-6, np.abs(got - want).max()
    # and m = (0, sin th, cos th) tilts towards +t = -z
    rec = host().map_records(n, np.tile((2, 0, 0), (k, 1)), np.tile((2, 0, -2), (k, 1)), np.zeros((k, 2)), np.tile((1, 0), (k, 1)), np.tile((1, 1), (k, 1)), m[:, [1, 0, 2]])
    assert np.abs(host().map_normal(rec, 1.0) - np.stack([np.zeros_like(th), np.cos(th), -np.sin(th)], 1)).max() <= 1e-6


def test_null_pointers_are_refused():
    import ctypes as C
    L = host().lib()
    out = np.zeros(3, np.float32)
    assert L.glrt_map_normal(None, 1, C.c_float(1.0), out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert L.glrt_map_alpha(None, 1, out.ctypes.data_as(C.POINTER(C.c_float))) == -1
    assert L.glrt_map_decode(None, 0, None) == 0
