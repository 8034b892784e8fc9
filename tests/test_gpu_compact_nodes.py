"""The compact node array on the device (stats.node_layout_last = 1; glrtx.hip: pack_compact, trav_asm.hip.h: GLRTX_TRAV_STEP_ASM_COMPACT): bit for bit
the 64-byte layout's images and ray counts, and the oracle's -- golden scenes, oracle configs, fuzz seeds, fed and adaptive launches, presentation,
groups --, the host's choice of layout, and the compiled step's registers."""
import subprocess
import sys

import pytest

from conftest import ROOT, assert_bit_equal, golden_names, load_golden
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _render(d, scene, params, frames=None, count_rays=True):
    d.upload_scene(scene)
    d.set_partition(0, 1, 16)
    d.resize(params["width"], params["height"])
    d.reset_stats()
    d.count_rays(count_rays)
    for sd in (frames or [params["seed"]]):
        d.render(dict(params, seed=sd))
    d.sync()
    return d.read_accum(), d.stats()


def _is_vine(scene):
    """Every fork has a leaf as children.y (glrt_bvh_build_chain): the list scan runs, never a tree layout (glrtx.hip: pack_scene)."""
    b = scene["bvh"].reshape(-1, 9)
    n = 0
    while len(b) and b[n, 8] < 0:
        r, l = int(b[n, 7]), int(b[n, 6])
        if r < 0 or l < 0 or b[r, 8] < 0:
            return False
        n = l
    return len(b) > 1


def _both(d, monkeypatch, scene, params, frames=None, count_rays=True):
    out = {}
    vine = _is_vine(scene)
    for layout in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", layout)
        acc, st = _render(d, scene, params, frames, count_rays)
        assert st.node_layout_last == (0 if vine else int(layout)) and st.node_fetch_last == 0
        out[layout] = (acc, int(st.rays))
    assert out["0"][1] == out["1"][1]
    assert_bit_equal(out["1"][0], out["0"][0], "compact vs 64-byte records")
    return out["1"]


@pytest.mark.parametrize("name", golden_names())
def test_golden_scenes_in_both_layouts(gpu_device, monkeypatch, name):
    monkeypatch.setenv("GLRTX_PAIR_FETCH", "0")
    scene, params, rows, frames, rgb, cnt = load_golden(name)
    acc, _ = _both(gpu_device, monkeypatch, scene, params, frames)
    acc = acc[rows[0]:rows[1]]
    assert_bit_equal(acc[..., :3], rgb, f"{name} rgb")
    assert_bit_equal(acc[..., 3], cnt, f"{name} count")


@pytest.mark.parametrize("cfg,kw", [("headline", dict(width=480, height=270)), ("c2", dict(width=480, height=270, max_depth=4)),
                                    ("c4", dict(width=384, height=216, max_depth=8, n_samples=4)), ("c1", dict(width=200, height=120, max_depth=16, n_samples=2)),
                                    ("c3", dict(width=240, height=135, max_depth=1, n=10_000, bvh="sah"))])
@pytest.mark.parametrize("count_rays", [True, False], ids=["counting", "timed"])
def test_configs_in_both_layouts_match_the_oracle(gpu_device, monkeypatch, cfg, kw, count_rays):
    from oracle import pt_oracle
    scene, params = scenes.CONFIGS[cfg](**kw)
    acc, rays = _both(gpu_device, monkeypatch, scene, params, count_rays=count_rays)
    ref, ref_rays = pt_oracle.render(scene, params)
    assert_bit_equal(acc, ref, f"{cfg} {kw}")
    if count_rays:
        assert rays == ref_rays


def test_host_picks_the_compact_layout_for_the_headline_and_not_for_config5(gpu_device, monkeypatch):
    monkeypatch.delenv("GLRTX_COMPACT_NODES", raising=False)
    monkeypatch.delenv("GLRTX_PAIR_FETCH", raising=False)
    scene, params = scenes.config_headline(64, 36)
    _, st = _render(gpu_device, scene, params)
    assert st.node_layout_last == 1 and st.node_fetch_last == 0
    scene, params = scenes.config_c5(64, 36, n=100_000)
    _, st = _render(gpu_device, scene, params)
    assert st.node_layout_last == 0 and st.node_fetch_last == 1  # config 5: the rank table does not fit; the pair-cooperative fetch, unchanged
    monkeypatch.setenv("GLRTX_PAIR_FETCH", "0")
    _, st = _render(gpu_device, scene, params)
    assert st.node_layout_last == 0, "100 k triangles: four workgroups per CU would not fit the rank table"
    scene, params = scenes.config_c3(64, 36, n=300)  # a vine: the list scan, never the compact array
    _, st = _render(gpu_device, scene, params)
    assert st.node_layout_last == 0


@pytest.mark.parametrize("k", [0, 1, 2, 3, 4, 5])
def test_fuzz_scenes_in_both_layouts(gpu_device, monkeypatch, k):
    from fuzz_scenes import CASES, case_scene_and_params
    from oracle import pt_oracle
    case = CASES[k * len(CASES) // 6]
    seed = case[0]
    scene, params = case_scene_and_params(case)
    monkeypatch.setenv("GLRTX_PAIR_FETCH", "0")
    acc, rays = _both(gpu_device, monkeypatch, scene, params)
    ref, ref_rays = pt_oracle.render(scene, params)
    assert rays == ref_rays
    assert_bit_equal(acc, ref, f"fuzz seed {seed}")


def test_fed_and_adaptive_launches_in_both_layouts(gpu_device, monkeypatch):
    scene, params = scenes.config_headline(320, 180, n_samples=1)
    seeds = [host.frame_seed(i) for i in range(6)]
    out = {}
    for layout in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", layout)
        d = gpu_device
        d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"])
        d.count_rays(True); d.reset_stats()
        d.render_frames(params, seeds[:4])
        for s in seeds[4:]:
            d.render(dict(params, seed=s))  # a burst: fed launches take these
        d.sync()
        fed = (d.read_accum(), int(d.stats().rays))
        assert d.stats().node_layout_last == int(layout)
        d.clear(); d.reset_stats()
        d.render_frames(params, seeds[:4])
        d.render_adaptive(params, seeds[4:], threshold=0.05, min_samples=2)
        d.sync()
        ad = (d.read_accum(), int(d.stats().rays))
        assert d.stats().node_layout_last == int(layout)
        out[layout] = (fed, ad)
    for k in range(2):
        assert out["0"][k][1] == out["1"][k][1]
        assert_bit_equal(out["1"][k][0], out["0"][k][0], ("fed", "adaptive")[k])


def test_presentation_and_groups_in_both_layouts(monkeypatch):
    import torch
    if torch.cuda.is_available():
        torch.cuda.init()
    scene, params = scenes.config_c2(256, 144, max_depth=4)
    seeds = [host.frame_seed(i) for i in range(3)]
    out = {}
    for layout in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", layout)
        g = device.Group([0, 0])
        try:
            g.upload_scene(scene)
            g.resize(params["width"], params["height"])
            g.render_frames(params, seeds)
            g.sync()
            out[layout] = g.read_accum()
        finally:
            g.close()
        d = device.Device()
        try:
            d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"])
            d.present_enable(4)
            for s in seeds:
                d.render(dict(params, seed=s))
            d.sync()
            out[layout + "p"] = d.read_accum()
            assert d.stats().node_layout_last == int(layout)
        finally:
            d.close()
    assert_bit_equal(out["1"], out["0"], "group")
    assert_bit_equal(out["1p"], out["0p"], "presentation")


def test_compact_instantiations_keep_four_workgroups_per_cu():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py"), "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for inst in ("false, false, 8", "true, false, 8", "false, false, 12", "true, false, 12"):
        rows = [ln.split()[-7:] for ln in r.stdout.splitlines() if ln.startswith(f"glrtx::pt_render_wgwf<{inst}>")]
        assert rows, inst
        vgpr, agpr, sgpr, vspill, sspill, scratch, _ = (int(v) for v in rows[0])
        assert vgpr + agpr <= 128 and vspill == 0 and sspill == 0 and scratch == 0, (inst, rows[0])
