"""glrtx_trace_rays / glrtx_trace_rays_device (csrc/query.hip.h) on the GPU: the device's hits equal the CPU statement's (glrt_trace_rays) in all four
words, bit for bit, in both modes and both node layouts, on fuzz, vine, config and denormal scenes and on every ray set; after vertex updates; through
torch tensors on the context's stream; and queries leave the renderer's accumulator and ray counts as they were."""
import numpy as np
import pytest

import query_rays as qr
from conftest import assert_bit_equal
from fuzz_scenes import CASES, case_scene_and_params, fuzz_scene
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _denormal_scene():
    """Triangles of denormal size next to ordinary ones (the scene of test_gpu_refit.py)."""
    pos, nrm, _ = scenes.random_triangles(40, 5, 1.0, 0.5)
    pos[:20] *= np.float32(1e-39)
    pos[20:25, :, 0] = np.float32(-0.0)
    b = scenes.SceneBuilder()
    m0 = b.add_material(scenes.diffuse((0.5, 0.5, 0.5)))
    m1 = b.add_material(scenes.emitter((4.0, 4.0, 4.0)))
    b.add_mesh(pos, nrm, np.where(np.arange(40) % 9 == 0, m1, m0))
    return b.build("sah")


def _ray_sets(scene, params, n=2000):
    cam = qr.camera_rays(params, min(params["width"], 64), min(params["height"], 48))
    inc = qr.incoherent_rays(scene, n)
    sh = qr.shadow_rays(scene, n)
    s0 = qr.incoherent_rays(scene, n // 2, seed=5, tmin=0.0)
    s1 = s0.copy()
    s1[:, 3] = np.float32(1e-4)
    return {"camera": cam, "incoherent": inc, "shadow": sh, "surface_tmin0": s0, "surface_tmin1e-4": s1, "no_search": qr.special_rays()}


_compare = qr.compare


def _assert_layout(d, compact):
    """GLRTX_COMPACT_NODES=1 asks for the 48-byte records; the launch takes them when the tree is no vine (n_crank > 0: a rank table exists) and the table
    fits in LDS next to the stacks.  Every scene of this file is small enough: a tree ran the kernel the test asked for, a vine never the compact one."""
    vine = d.read_scene("vine").size > 0
    assert d.stats().node_layout_last == (int(compact) if not vine else 0)


def _check_scene(d, monkeypatch, scene, params, label, n=2000):
    d.upload_scene(scene)
    sets = _ray_sets(scene, params, n)
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        for name, rays in sets.items():
            for any_hit in (False, True):
                _compare(d, scene, rays, f"{label} compact={compact} {name}", any_hit)
                _assert_layout(d, compact)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[f"fuzz{c[0]}-{c[2]}" for c in CASES])
def test_fuzz_cases(gpu_device, monkeypatch, case):
    scene, params = case_scene_and_params(CASES[case])
    _check_scene(gpu_device, monkeypatch, scene, params, f"case {CASES[case][0]}")


def test_vines(gpu_device, monkeypatch):
    scene, params = scenes.config_c3(96, 64, n=3000)  # the chain builder: every fork has the same box (the uniform list)
    _check_scene(gpu_device, monkeypatch, scene, params, "c3 uniform vine")
    gpu_device.upload_scene(scene)
    assert gpu_device.read_scene("vine").size > 0
    tight = dict(scene, bvh=host.refit_bvh(scene["vert"], scene["tri"], scene["bvh"]))  # suffix boxes: a vine whose forks differ
    _check_scene(gpu_device, monkeypatch, tight, params, "c3 vine, suffix boxes")
    gpu_device.upload_scene(tight)
    root = gpu_device.read_scene("root").view(np.int32)
    assert root[9] == 0 and root[11] > 0  # not uniform, a vine


@pytest.mark.parametrize("name", ["c1", "c2", "c5"])
def test_configs_reduced(gpu_device, monkeypatch, name):
    if name == "c1":
        scene, params = scenes.config_c1(128, 96, subdiv=2)
    elif name == "c2":
        scene, params = scenes.config_c2(128, 96, subdiv=2)
    else:
        scene, params = scenes.config_c5(128, 96, n=20_000)
    _check_scene(gpu_device, monkeypatch, scene, params, name, n=4000)


def test_denormal_scene(gpu_device, monkeypatch):
    scene = _denormal_scene()
    c2w, s2c = scenes.camera((0.3, 0.2, 3.0), (0, 0, 0), (0, 1, 0), 45.0, 48, 32)
    _check_scene(gpu_device, monkeypatch, scene, scenes.make_params(c2w, s2c, 48, 32, 4), "denormal")
    rays = qr.incoherent_rays(scene, 500, seed=9, tmin=0.0)
    rays[:, 0:3] *= np.float32(1e-39)  # origins of denormal size: read as zeros on both sides
    for any_hit in (False, True):
        _compare(gpu_device, scene, rays, "denormal origins", any_hit)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1_000_001])
def test_batch_sizes(gpu_device, n):
    scene, params = case_scene_and_params(CASES[0])
    gpu_device.upload_scene(scene)
    rays = qr.incoherent_rays(scene, n, seed=n)
    for any_hit in (False, True):
        _compare(gpu_device, scene, rays, f"n={n}", any_hit)


def test_after_vertex_updates(gpu_device, monkeypatch):
    import torch
    scene, params = case_scene_and_params(CASES[0])
    d = gpu_device
    d.upload_scene(scene)
    rng = np.random.default_rng(3)
    for step, use_torch in ((0, False), (1, True)):
        v = scene["vert"].reshape(-1, 15).copy()
        v[:, :3] += rng.normal(0, 0.1, (len(v), 3)).astype(np.float32)
        if use_torch:
            d.update_vertices(torch.from_numpy(v).cuda())
        else:
            d.update_vertices(v)
        moved = dict(scene, vert=v, bvh=host.refit_bvh(v, scene["tri"], scene["bvh"]))
        for name, rays in _ray_sets(moved, params, 1500).items():
            for compact in ("0", "1"):
                monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
                for any_hit in (False, True):
                    _compare(d, moved, rays, f"update {step} {name} compact={compact}", any_hit)


def test_torch_tensors_on_the_contexts_stream(gpu_device):
    import torch
    scene, params = scenes.config_c1(128, 96, subdiv=2)
    d = gpu_device
    d.upload_scene(scene)
    rays = qr.incoherent_rays(scene, 100_000, seed=11)
    ref = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], rays)
    s = torch.cuda.Stream()
    d.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):  # the producer runs on the context's stream: no sync before the query
            base = torch.zeros((len(rays), 8), dtype=torch.float32, device="cuda")
            torch.cuda._sleep(20_000_000)
            r = base + torch.from_numpy(rays).cuda()
            t, tri, u, v = d.trace_rays(r)
            assert t.device.type == "cuda" and tri.dtype == torch.int32
            out = torch.stack([t, tri.view(torch.float32), u, v], 1).cpu()  # ordered behind the query on the same stream
        s.synchronize()
        got = out.numpy().view(np.uint32)
        want = np.stack([np.asarray(x).view(np.uint32) for x in ref], 1)
        assert np.array_equal(got, want)
        # a caller-owned output tensor, any-hit
        o = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
        with torch.cuda.stream(s):
            d.trace_rays(r, any_hit=True, out=o)
        s.synchronize()
        ra = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], rays, True)
        assert np.array_equal(o.cpu().numpy().view(np.uint32), np.stack([np.asarray(x).view(np.uint32) for x in ra], 1))
    finally:
        d.set_stream(0)


def _setup(d, scene, params):
    d.upload_scene(scene)
    d.set_variant(2)
    d.set_partition(0, 1, 16)
    d.resize(params["width"], params["height"])
    d.clear()
    d.reset_stats()
    d.count_rays(True)


def test_query_between_renders_changes_nothing(gpu_device):
    """render N frames, query, render M frames == N + M frames without the query: accumulator and ray counts; the single-frame calls form fed bursts, so the
    queries also land inside open bursts (which they seal)."""
    scene, params = scenes.config_c1(160, 120, max_depth=4, subdiv=2)
    d = gpu_device
    seeds = [host.frame_seed(i) for i in range(6)]
    rays = qr.incoherent_rays(scene, 50_000, seed=12)

    def run(query):
        _setup(d, scene, params)
        d.render_frames(params, seeds[:2])
        if query:
            d.trace_rays(rays)
        d.render_frames(params, seeds[2:3])
        for k, sd in enumerate(seeds[3:]):
            d.render(dict(params, seed=sd))  # single-frame calls back to back: a fed burst
            if query:
                d.trace_rays(rays, any_hit=bool(k & 1))
        d.sync()
        return d.read_accum().copy(), d.stats().rays

    acc_q, rays_q = run(True)
    acc, n = run(False)
    assert rays_q == n
    assert_bit_equal(acc_q, acc, "renders with queries in between")
    d.count_rays(False)


def test_errors(gpu_device):
    import ctypes as C
    d = device.Device()
    try:
        L = d.L
        fp = C.POINTER(C.c_float)
        r = np.zeros((4, 8), np.float32)
        o = np.zeros((4, 4), np.float32)
        assert L.glrtx_trace_rays(d.h, r.ctypes.data_as(fp), 4, o.ctypes.data_as(fp), 0) == -1  # no scene
        scene, _ = case_scene_and_params(CASES[0])
        d.upload_scene(scene)
        assert L.glrtx_trace_rays(d.h, r.ctypes.data_as(fp), 4, o.ctypes.data_as(fp), 2) == -1  # unknown flag
        assert L.glrtx_trace_rays(d.h, None, 4, o.ctypes.data_as(fp), 0) == -1
        assert L.glrtx_trace_rays_device(d.h, None, 4, None, 0) == -1
        assert L.glrtx_trace_rays(d.h, r.ctypes.data_as(fp), 1 << 31, o.ctypes.data_as(fp), 0) == -1
        assert L.glrtx_trace_rays(d.h, None, 0, None, 0) == 0
        assert L.glrtx_trace_rays_device(d.h, None, 0, None, 1) == 0
        assert (o == 0).all()
    finally:
        d.close()
