"""The environment through the C++ facade on the GPU (glrt::Scene::parse's "environment" block, glrt::Window's upload, glrt_main): JSON + OBJ + PFM in, PNG
out, byte for byte the image the Python-driven device render of the same buffers and the same map resolves to -- once from a lat-long picture, once from an
octahedral map --, and --env-mode overrides the file."""
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import host, scenes
from test_scene_parse import _probe as scene_probe

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES = 64, 48, 4, 3


def _main(js, out, *more):
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--extensions", "--max-depth", str(DEPTH), "--frames", str(FRAMES), "--out", str(out), *more],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _device_image(d, js, env_map, cfg):
    got = scene_probe(js)  # the buffers Scene::parse hands to the device
    scene = dict(vert=got["vert"], tri=got["tri"], mat=got["mat"], light=got["light"], bvh=got["nodes"])
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, W, H)
    params = scenes.make_params(c2w, s2c, W, H, DEPTH, 1)
    d.set_variant(2); d.set_extensions(0)
    d.upload_scene(scene); d.upload_spheres(None)
    d.set_partition(0, 1, 16); d.resize(W, H); d.clear()
    d.upload_environment(env_map, cfg)
    try:
        for f in range(FRAMES):
            d.render(dict(params, seed=host.frame_seed(f), focal=0.0))  # absent focalLength parses as 0 (scene.cpp:71-74)
        d.sync()
        return d.resolve_rgba8(2.2, True), d.stats().variant_last
    finally:
        d.upload_environment(None)


@pytest.mark.parametrize("layout", ["latlong", "octahedral"])
def test_glrt_main_renders_an_environment_like_the_binding(tmp_path, gpu_device, layout):
    from PIL import Image
    rng = np.random.default_rng(9)
    _, _, wall = scenes.config_textured_wall(n=2)
    js = scenes.export_json_obj(wall["builder"], tmp_path, W, H, *wall["camera"])
    if layout == "latlong":
        ll = rng.uniform(0.0, 3.0, (16, 32, 3)).astype(np.float32)  # rows from the top down
        scenes.write_pfm(tmp_path / "sky.pfm", ll[::-1])
        block = {"file": "sky.pfm", "size": 24, "mode": "sampled", "scale": [1.0, 0.75, 1.5], "rotate_y": 90, "light_pick": 0.5}
        env_map = (host.env_from_latlong(ll, 24), "rgba32f", "bilinear")
    else:
        tex = rng.uniform(0.0, 3.0, (10, 10, 3)).astype(np.float32)
        scenes.write_pfm(tmp_path / "sky.pfm", tex)
        block = {"file": "sky.pfm", "layout": "octahedral", "mode": "sampled", "scale": [1.0, 0.75, 1.5], "rotate_y": 90, "light_pick": 0.5, "filter": "nearest"}
        env_map = (tex, "rgba32f", "nearest")
    doc = json.loads(js.read_text())
    doc["environment"] = block
    js.write_text(json.dumps(doc, indent=1))
    images = {}
    for mode in ("sampled", "escape"):
        out = tmp_path / f"{mode}.png"
        log = _main(js, out, *(() if mode == "sampled" else ("--env-mode", "escape")))
        assert "environment: " in log and f"{mode} mode" in log
        img = np.asarray(Image.open(out))
        ref, variant = _device_image(gpu_device, js, env_map, host.env_cfg(mode, light_pick=0.5, scale=(1.0, 0.75, 1.5), rotate_y=90))
        assert variant == 1 and img.shape == (H, W, 4)
        assert np.array_equal(img, ref), f"{layout}, {mode}: {int((img != ref).any(-1).sum())} pixels differ"
        images[mode] = img
    assert (images["sampled"] != images["escape"]).any(-1).mean() > 0.2, "--env-mode changes the estimator"
