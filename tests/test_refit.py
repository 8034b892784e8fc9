"""glrt_bvh_refit (include/glrt_host.h): the refit rule against a numpy statement of it, on fuzz trees of every builder; what it gives back for unchanged
vertices; the chain's suffix boxes; error codes; and the new entry points of the refit in the header, the library and the Python binding."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

from fuzz_scenes import fuzz_scene
from glrt_amd import device, host, scenes

ROOT = pathlib.Path(__file__).resolve().parents[1]
BUILDERS = ["sah", "sah-reinsert", "lbvh", "sahl", "reference", "chain"]


def _key(f):
    u = np.ascontiguousarray(f, np.float32).view(np.uint32)
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k).astype(np.uint32).view(np.float32)


def refit_statement(vert, tri, nodes):
    """Rule 1 in numpy: leaf = min / max of its triangle's positions, fork = min / max of its present children, childless fork keeps its box, unreachable
    nodes untouched; min / max on ordered-integer keys."""
    pos = np.asarray(vert, np.float32).reshape(-1, 15)[:, :3]
    t = np.asarray(tri, np.float32).reshape(-1, 4)[:, :3].astype(np.int64)
    b = np.asarray(nodes, np.float32).reshape(-1, 9).copy()
    keys = {}

    def visit(n):  # (iterative post-order: chains are deep)
        st = [(n, False)]
        while st:
            m, done = st.pop()
            if b[m, 8] >= 0:
                k = _key(pos[t[int(b[m, 8])]])
                keys[m] = np.concatenate([k.min(0), k.max(0)])
                continue
            kids = [int(c) for c in b[m, 6:8] if c >= 0]
            if not done:
                st.append((m, True))
                st.extend((c, False) for c in kids)
                continue
            if not kids:
                keys[m] = _key(b[m, :6])
            else:
                ks = np.stack([keys[c] for c in kids])
                keys[m] = np.concatenate([ks[:, :3].min(0), ks[:, 3:].max(0)])

    visit(0)
    for m, k in keys.items():
        b[m, :6] = _unkey(k)
    return b


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _moved(scene, seed):
    """The scene's vertices translated, rotated, jittered, with +-0 and duplicated coordinates mixed in."""
    rng = np.random.default_rng(seed)
    v = scene["vert"].reshape(-1, 15).copy()
    p = v[:, :3].astype(np.float64)
    a = rng.uniform(0, 2 * np.pi)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    p = p @ R.T + rng.normal(0, 0.3, 3) + rng.normal(0, 0.02, p.shape)
    p = p.astype(np.float32)
    p[::7, 0] = np.float32(-0.0)
    p[1::7, 0] = np.float32(0.0)
    p[2::11] = p[0]  # coincident vertices
    v[:, :3] = p
    v[:, 3:6] = rng.normal(0, 1, (len(v), 3)).astype(np.float32)
    return v


@pytest.mark.parametrize("kind", BUILDERS)
@pytest.mark.parametrize("seed,flags", [(31, {}), (32, dict(duplicates=True)), (33, dict(degenerate=True)), (34, dict(axis_aligned=True, degenerate=True))])
def test_refit_matches_the_numpy_statement(kind, seed, flags):
    sc = fuzz_scene(seed, 90, kind, **flags)
    v = _moved(sc, seed)
    got = host.refit_bvh(v, sc["tri"], sc["bvh"]).reshape(-1, 9)
    assert _same_bits(got, refit_statement(v, sc["tri"], sc["bvh"]))
    assert _same_bits(got[:, 6:], sc["bvh"].reshape(-1, 9)[:, 6:])  # topology untouched


def test_refit_one_child_forks_childless_forks_and_unreachable_nodes():
    sc = fuzz_scene(35, 40, "sah")
    b = sc["bvh"].reshape(-1, 9).copy()
    forks = np.flatnonzero(b[:, 8] < 0)
    # cut one child of some forks (its subtree becomes unreachable) and both children of another (a childless fork with a box of its own)
    cut = [int(f) for f in forks[1:6]]
    for k, f in enumerate(cut[:4]):
        b[f, 6 + (k & 1)] = -1.0
    b[cut[4], 6:8] = -1.0
    b[cut[4], :6] = np.float32([-5, -6, -7, 5, 6, 7])
    unreachable_before = b.copy()
    v = _moved(sc, 36)
    got = host.refit_bvh(v, sc["tri"], b).reshape(-1, 9)
    want = refit_statement(v, sc["tri"], b)
    assert _same_bits(got, want)
    # what the walk from node 0 never meets keeps its bits
    reach = set()
    st = [0]
    while st:
        n = st.pop()
        reach.add(n)
        if b[n, 8] < 0:
            st.extend(int(c) for c in b[n, 6:8] if c >= 0)
    other = [n for n in range(len(b)) if n not in reach]
    assert other and _same_bits(got[other], unreachable_before[other])
    assert _same_bits(got[cut[4], :6], np.float32([-5, -6, -7, 5, 6, 7]))


def test_refit_order_is_total_on_bit_patterns():
    # three triangles sharing coordinates +0 / -0 and denormals: the box takes -0 as the smaller zero and keeps denormal bits
    pos = np.float32([[0.0, 1e-42, 1.0], [-0.0, -1e-42, 2.0], [0.0, 3e-43, 3.0]])
    v = np.zeros((3, 15), np.float32)
    v[:, :3] = pos
    tri = np.float32([[0, 1, 2, 0]])
    nodes = np.zeros((1, 9), np.float32)
    nodes[0, 6:] = [-1, -1, 0]
    got = host.refit_bvh(v, tri, nodes).reshape(-1, 9)[0]
    assert got[:3].view(np.uint32).tolist() == np.float32([-0.0, -1e-42, 1.0]).view(np.uint32).tolist()
    assert got[3:6].view(np.uint32).tolist() == np.float32([0.0, 1e-42, 3.0]).view(np.uint32).tolist()


@pytest.mark.parametrize("kind", ["sah", "sah-reinsert", "lbvh", "sahl", "reference"])
def test_refit_of_unchanged_vertices_gives_back_the_builders_boxes(kind):
    sc = fuzz_scene(41, 150, kind, duplicates=True)
    b = sc["bvh"].reshape(-1, 9)
    got = host.refit_bvh(sc["vert"], sc["tri"], b).reshape(-1, 9)
    forks = b[:, 8] < 0
    assert np.array_equal(got[forks, :6], b[forks, :6]), f"{kind}: a builder's fork box is not the tight box of its leaves"


def test_refit_gives_chain_trees_suffix_boxes():
    sc = fuzz_scene(42, 60, "chain")
    b = sc["bvh"].reshape(-1, 9)
    got = host.refit_bvh(sc["vert"], sc["tri"], b).reshape(-1, 9)
    pos = sc["vert"].reshape(-1, 15)[:, :3]
    tb = pos[sc["tri"][:, :3].astype(np.int64)]
    n = len(tb)
    # glrt_bvh_build_chain: fork i at node 2i has triangle i (node 2i + 1) and the rest of the chain; its refitted box is that of triangles i .. n - 1
    for i in range(n - 1):
        assert np.array_equal(got[2 * i, :3], tb[i:].reshape(-1, 3).min(0))
        assert np.array_equal(got[2 * i, 3:6], tb[i:].reshape(-1, 3).max(0))
    assert np.array_equal(b[2, :6], b[0, :6])  # the builder's global boxes ...
    assert not np.array_equal(got[2 * (n - 2), :6], got[0, :6])  # ... become suffix boxes


def test_refit_error_codes_leave_the_tree_alone():
    L = host.lib()
    sc = fuzz_scene(43, 20, "sah")
    v, t = np.ascontiguousarray(sc["vert"].reshape(-1, 15)), np.ascontiguousarray(sc["tri"])
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
    b = np.ascontiguousarray(sc["bvh"].reshape(-1, 9)).copy()
    keep = b.copy()
    assert L.glrt_bvh_refit(None, len(v), fp(t), len(t), fp(b), len(b)) == -1
    assert L.glrt_bvh_refit(fp(v), len(v), fp(t), 0, fp(b), len(b)) == -1
    assert L.glrt_bvh_refit(fp(v), len(v), fp(t), len(t), fp(b), 0) == -1
    bad_t = t.copy()
    bad_t[3, 1] = len(v)
    assert L.glrt_bvh_refit(fp(v), len(v), fp(bad_t), len(t), fp(b), len(b)) == -2
    bad = b.copy()
    bad[0, 6] = len(b)  # a child out of range
    assert L.glrt_bvh_refit(fp(v), len(v), fp(t), len(t), fp(bad), len(b)) == -1
    assert _same_bits(bad[:, :6], keep[:, :6])
    bad = b.copy()
    bad[0, 6] = bad[0, 7]  # a node reached twice
    assert L.glrt_bvh_refit(fp(v), len(v), fp(t), len(t), fp(bad), len(b)) == -1
    leaf = int(np.flatnonzero(b[:, 8] >= 0)[0])
    bad = b.copy()
    bad[leaf, 8] = len(t)  # a leaf triangle out of range
    assert L.glrt_bvh_refit(fp(v), len(v), fp(t), len(t), fp(bad), len(b)) == -1
    assert _same_bits(b, keep)
    with pytest.raises(RuntimeError):
        host.refit_bvh(v, bad_t, b)


def test_update_entry_points_in_header_library_and_binding():
    hdr = (ROOT / "include" / "glrtx.h").read_text()
    names = ["glrtx_update_vertices", "glrtx_update_vertices_device", "glrtx_group_update_vertices", "glrtx_debug_read_scene"]
    for n in names:
        assert re.search(rf"\b{n}\(", hdr), n
        assert n in device.EXPORTS
        assert hasattr(device.lib(), n)
    assert re.search(r"\bglrt_bvh_refit\(", (ROOT / "include" / "glrt_host.h").read_text())
    assert hasattr(host.lib(), "glrt_bvh_refit")
    assert callable(device.Device.update_vertices) and callable(device.Group.update_vertices) and callable(host.refit_bvh)


def test_update_vertices_rejects_wrong_dtype_and_shape_before_any_device_call():
    with pytest.raises(TypeError):
        device._host_vertices(np.zeros((4, 15), np.float64))
    with pytest.raises(ValueError):
        device._host_vertices(np.zeros((4, 14), np.float32))
    a, n = device._host_vertices(np.zeros((4, 15), np.float32))
    assert n == 4
    _, n = device._host_vertices(np.zeros(45, np.float32))
    assert n == 3
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        device._device_vertices(torch.zeros(30, dtype=torch.float64), 0)
    with pytest.raises(ValueError):
        device._device_vertices(torch.zeros(30, dtype=torch.float32), 0)  # a CPU tensor


def test_scene_vertices_keep_the_wire_layout():
    sc, _ = scenes.config_c1(16, 16, subdiv=1)
    assert sc["vert"].size % 15 == 0
