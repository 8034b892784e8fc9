"""glrtx_trace_rays on the rays a picking / visibility / height-probe host sends (query_rays.py: axial_rays, in_plane_rays, feature_rays,
range_edge_rays, scaled_rays) and on batches that mix searched and dead rays lane by lane (interleave): the device's four words per ray equal the CPU
statement's (glrt_trace_rays, itself pinned to a brute force on these sets by test_query_hostile_host.py), bit for bit, in both modes and both node
layouts -- and the layout is the one the test asked for, read back from stats.node_layout_last, the silent fallback to the 64-byte records included."""
import numpy as np
import pytest

import query_rays as qr
from fuzz_scenes import CASES, case_scene_and_params
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _expected_layout(d, scene, compact):
    """trace_launch's rule (glrtx.hip) from host-side facts: GLRTX_COMPACT_NODES=1 runs the compact kernel unless the tree is a vine or the per-lane stacks
    plus the rank table exceed 160 KiB of LDS."""
    if compact == "0" or d.read_scene("vine").size > 0:
        return 0
    from test_host import _pack
    stack_entries = _pack(scene)[3]
    ranks = device.pack_compact(scene)[1]
    return int(2 * stack_entries * 256 * 4 + 8 * ranks.shape[0] <= 160 * 1024)


def _check(d, monkeypatch, scene, label, n=240, sets=None, want_layout=None):
    d.upload_scene(scene)
    sets = sets or qr.hostile_sets(scene, n)
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        want = _expected_layout(d, scene, compact)
        if want_layout is not None:
            assert want == want_layout[compact], (label, compact, want)
        for name, rays in sets.items():
            for any_hit in (False, True):
                qr.compare(d, scene, rays, f"{label} compact={compact} {name}", any_hit)
                assert d.stats().node_layout_last == want, f"{label}: GLRTX_COMPACT_NODES={compact} ran layout {d.stats().node_layout_last}, expected {want}"
        print(f"{label}: GLRTX_COMPACT_NODES={compact} ran layout {want}; {sum(len(r) for r in sets.values())} rays x 2 modes")


@pytest.mark.parametrize("case", [0, 1, 3, 6, 10, 11, 12], ids=lambda c: f"fuzz{CASES[c][0]}-{CASES[c][2]}")
def test_fuzz_cases(gpu_device, monkeypatch, case):
    scene, _ = case_scene_and_params(CASES[case])
    _check(gpu_device, monkeypatch, scene, f"case {CASES[case][0]}", want_layout={"0": 0, "1": 1})


@pytest.mark.parametrize("kind", ["one_child", "one_child_chains", "comb"])
def test_trees_with_absent_children_and_the_deepest_stack(gpu_device, monkeypatch, kind):
    """comb: 63 triangles, a stack entry per level -- the per-lane stacks in LDS at their largest (test_gpu_parity.py: test_deep_traversal_stacks_match_the_oracle)."""
    from test_compact_nodes import _scene
    _check(gpu_device, monkeypatch, _scene(kind), kind, want_layout={"0": 0, "1": 1})


def test_vines(gpu_device, monkeypatch):
    scene, _ = scenes.config_c3(96, 64, n=3000)  # the chain builder: every fork has the same box (the uniform list)
    _check(gpu_device, monkeypatch, scene, "c3 uniform vine", want_layout={"0": 0, "1": 0})
    tight = dict(scene, bvh=host.refit_bvh(scene["vert"], scene["tri"], scene["bvh"]))  # suffix boxes: a vine whose forks differ
    _check(gpu_device, monkeypatch, tight, "c3 vine, suffix boxes", want_layout={"0": 0, "1": 0})
    root = gpu_device.read_scene("root").view(np.int32)
    assert root[9] == 0 and root[11] > 0  # not uniform, a vine


def test_large_tree(gpu_device, monkeypatch):
    scene, _ = scenes.config_c5(128, 96, n=20_000)
    _check(gpu_device, monkeypatch, scene, "c5 20k", n=1200, want_layout={"0": 0, "1": 1})


def test_rank_table_too_large_falls_back_to_the_64_byte_records(gpu_device, monkeypatch):
    """400 k triangles: the rank table alone is ~160 KB, so GLRTX_COMPACT_NODES=1 cannot be honoured -- and the launch says so."""
    scene, _ = scenes.config_c5(64, 36, n=400_000, bvh="lbvh")
    _check(gpu_device, monkeypatch, scene, "c5 400k lbvh", n=240, want_layout={"0": 0, "1": 0})


def test_after_a_vertex_update(gpu_device, monkeypatch):
    scene, _ = case_scene_and_params(CASES[0])
    d = gpu_device
    d.upload_scene(scene)
    v = scene["vert"].reshape(-1, 15).copy()
    v[:, :3] += np.random.default_rng(3).normal(0, 0.1, (len(v), 3)).astype(np.float32)
    d.update_vertices(v)
    moved = dict(scene, vert=v, bvh=host.refit_bvh(v, scene["tri"], scene["bvh"]))
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        for name, rays in qr.hostile_sets(moved).items():
            for any_hit in (False, True):
                qr.compare(d, moved, rays, f"moved {name} compact={compact}", any_hit)
                assert d.stats().node_layout_last == int(compact)


def _pools(scene, n=1500):
    """(live: searched rays that pass the root box, feature rays (long searches) first; dead: rays that are never active)."""
    pool = np.concatenate([qr.feature_rays(scene, n), qr.axial_rays(scene, n), qr.in_plane_rays(scene, n)])
    live = pool[qr.reach(scene, pool, pool[:, 7])[0].any(1)]
    dead = qr.dead_rays(scene, 200)
    assert len(live) > n and (host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], dead)[1] == -1).all()
    return live, dead


def _batches(scene):
    live, dead = _pools(scene)
    out = {name: qr.interleave(live, dead, name) for name in qr.lane_patterns()}
    # one long search next to 63 short ones, chunk after chunk: a feature ray that hits among axial rays in box face planes (they end within a few steps)
    t, tri, _, _ = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], live)
    long_, short = live[tri >= 0], qr.axial_rays(scene, 63 * 6, seed=29)
    b = short[np.arange(64 * 6) % len(short)].copy()
    b[::64] = long_[:6]
    out["long_among_short"] = b
    return out


@pytest.mark.parametrize("tree", ["small", "large"])
def test_interleaved_batches(gpu_device, monkeypatch, tree):
    scene = case_scene_and_params(CASES[0])[0] if tree == "small" else scenes.config_c5(128, 96, n=20_000)[0]
    _check(gpu_device, monkeypatch, scene, f"interleaved, {tree} tree", sets=_batches(scene), want_layout={"0": 0, "1": 1})


def test_interleaved_batch_larger_than_the_resident_grid(gpu_device, monkeypatch):
    """1 000 001 rays: more chunks than the persistent grid has waves, so every wave fetches chunk after chunk -- alternate lanes dead, every seventh chunk
    dead as a whole, a partial last chunk of one ray."""
    scene = case_scene_and_params(CASES[0])[0]
    live, dead = _pools(scene)
    i = np.arange(1_000_001)
    batch = qr.interleave(live, dead, ((i % 64) % 3 != 0) & ((i // 64) % 7 != 3))
    d = gpu_device
    d.upload_scene(scene)
    for any_hit in (False, True):
        ref = np.stack([np.asarray(x).view(np.uint32) for x in host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], batch, any_hit)], 1)
        for compact in ("0", "1"):
            monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
            got = np.stack([np.asarray(x).view(np.uint32) for x in d.trace_rays(batch, any_hit=any_hit)], 1)
            assert d.stats().node_layout_last == int(compact)
            bad = np.nonzero((got != ref).any(1))[0]
            assert bad.size == 0, f"any={any_hit} compact={compact}: {bad.size} rays differ, first {bad[0]}: device {got[bad[0]].tolist()} cpu {ref[bad[0]].tolist()}"


def test_interleaved_batches_through_torch_tensors(gpu_device, monkeypatch):
    import torch
    scene = case_scene_and_params(CASES[0])[0]
    d = gpu_device
    d.upload_scene(scene)
    monkeypatch.setenv("GLRTX_COMPACT_NODES", "1")
    for name, batch in _batches(scene).items():
        r = torch.from_numpy(batch).cuda()
        torch.cuda.synchronize()
        for any_hit in (False, True):
            t, tri, u, v = d.trace_rays(r, any_hit=any_hit)
            d.sync()
            got = torch.stack([t, tri.view(torch.float32), u, v], 1).cpu().numpy().view(np.uint32)
            ref = np.stack([np.asarray(x).view(np.uint32) for x in host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], batch, any_hit)], 1)
            assert np.array_equal(got, ref), f"{name} any={any_hit}"
            assert d.stats().node_layout_last == 1
