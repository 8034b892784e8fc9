"""Material maps through the C++ facade on the GPU (glrt::Scene::parse's "normal_map" block, glrt::Window's upload and binding, glrt_main): with a flat PFM
normal map glrt_main writes the same bytes as without the key; with a bump map it writes different bytes, the ones the Python-driven device render of the same
buffers with the same map resolves to."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import host, scenes
from test_scene_parse import _probe as scene_probe

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES, N = 64, 48, 4, 2, 4


def _main(js, out):
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(DEPTH), "--frames", str(FRAMES), "--out", str(out)],
                       capture_output=True, text=True, timeout=120, env=dict(os.environ, GLRT_EXTENSIONS="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _device_image(d, js, textures, normal):
    got = scene_probe(js)  # the buffers Scene::parse hands to the device
    scene = dict(vert=got["vert"], tri=got["tri"], mat=got["mat"], light=got["light"], bvh=got["nodes"])
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, W, H)
    params = scenes.make_params(c2w, s2c, W, H, DEPTH, 1)
    d.set_variant(2); d.set_extensions(0)
    d.upload_scene(scene); d.upload_spheres(None)
    d.set_partition(0, 1, 16); d.resize(W, H); d.clear()
    d.upload_textures(textures, np.full(normal.size, -1, np.int32))
    d.bind_material_maps(normal=normal, normal_scale=0.8)
    try:
        for f in range(FRAMES):
            d.render(dict(params, seed=host.frame_seed(f), focal=0.0))  # absent focalLength parses as 0
        d.sync()
        return d.resolve_rgba8(2.2, True)
    finally:
        d.upload_textures(None, None)


def test_glrt_main_with_a_flat_map_and_with_a_bump_map(tmp_path, gpu_device):
    from PIL import Image
    rng = np.random.default_rng(8)
    scenes.write_pfm(tmp_path / "flat.pfm", np.tile(np.float32([0.5, 0.5, 1.0]), (2, 2, 1)))
    m = np.concatenate([rng.uniform(-0.7, 0.7, (8, 8, 2)), np.ones((8, 8, 1))], -1)
    bump = ((m / np.linalg.norm(m, axis=-1, keepdims=True) + 1.0) / 2.0).astype(np.float32)
    scenes.write_pfm(tmp_path / "bump.pfm", bump)
    images = {}
    for name, block in (("none", None), ("flat", {"file": "flat.pfm"}), ("bump", {"file": "bump.pfm", "scale": 0.8})):
        _, _, wall = scenes.config_mapped_wall(n=N, wall="conductor", uv="corner", normal_map=block)
        js = scenes.export_json_obj(wall["builder"], tmp_path / name, W, H, *wall["camera"])
        if block:
            (tmp_path / name / block["file"]).write_bytes((tmp_path / block["file"]).read_bytes())
        out = tmp_path / f"{name}.png"
        log = _main(js, out)
        assert ("material maps: 1" in log) == (block is not None), log
        images[name] = (out.read_bytes(), np.asarray(Image.open(out)), js)
    assert images["flat"][0] == images["none"][0]  # the same bytes as without the key
    assert images["bump"][0] != images["none"][0]
    assert (images["bump"][1] != images["none"][1]).any(-1).mean() > 0.1
    normal = np.full(4, -1, np.int32)
    normal[wall["material"]] = 0
    ref = _device_image(gpu_device, images["bump"][2], [(bump, "rgba32f", "repeat", "bilinear")], normal)
    assert np.array_equal(images["bump"][1], ref), f"{int((images['bump'][1] != ref).any(-1).sum())} pixels differ"
