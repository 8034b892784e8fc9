"""Emission maps through the C++ facade on the GPU (glrt::Scene::parse's "emission_map" block, glrt::Window's upload, glrt_main): JSON + OBJ with vt lines + a PPM
in, PNG out, byte for byte the image the Python-driven device render of the same buffers, the same set and the same bindings resolves to; with extensions off
the key is ignored and the image is the plain emitter's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import host, scenes
from test_scene_parse import _probe as scene_probe

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES, N = 96, 64, 4, 3, 4


def _main(js, out, extensions):
    env = dict(os.environ, GLRT_EXTENSIONS="1" if extensions else "0")
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(DEPTH), "--frames", str(FRAMES), "--out", str(out)],
                       capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _device_image(d, js, textures, emit):
    got = scene_probe(js)  # the buffers Scene::parse hands to the device
    scene = dict(vert=got["vert"], tri=got["tri"], mat=got["mat"], light=got["light"], bvh=got["nodes"])
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, W, H)
    params = scenes.make_params(c2w, s2c, W, H, DEPTH, 1)
    d.set_variant(2); d.set_extensions(0)
    d.upload_scene(scene); d.upload_spheres(None)
    d.set_partition(0, 1, 16); d.resize(W, H); d.clear()
    if textures:
        d.upload_textures(textures, np.full(emit.size, -1, np.int32))
        d.bind_emission_maps(emit)
    try:
        for f in range(FRAMES):
            d.render(dict(params, seed=host.frame_seed(f), focal=0.0))  # absent focalLength parses as 0 (scene.cpp:71-74)
        d.sync()
        return d.resolve_rgba8(2.2, True), d.stats().variant_last, d.last_kernel()
    finally:
        d.upload_textures(None, None)


def test_glrt_main_renders_an_emission_map_like_the_binding(tmp_path, gpu_device):
    from PIL import Image
    rng = np.random.default_rng(8)
    glow = rng.integers(0, 256, (6, 7, 3), dtype=np.uint8)
    scenes.write_ppm(tmp_path / "glow.ppm", glow)
    _, _, wall = scenes.config_emissive_wall(n=N, uv="corner", emission_map={"file": "glow.ppm", "wrap": "clamp"})
    js = scenes.export_json_obj(wall["builder"], tmp_path, W, H, *wall["camera"])
    out = tmp_path / "out.png"
    log = _main(js, out, True)
    assert "emission maps: 1" in log and "emission map: " in log
    img = np.asarray(Image.open(out))
    emit = np.full(4, -1, np.int32)
    emit[wall["material"]] = 0
    ref, variant, kernel = _device_image(gpu_device, js, [(glow, "rgba8_srgb", "clamp", "bilinear")], emit)
    assert variant == 1 and kernel.endswith("emission maps)") and img.shape == (H, W, 4)
    assert np.array_equal(img, ref), f"{int((img != ref).any(-1).sum())} pixels differ"
    # extensions off: the key is ignored -- the plain emitter's image, which is another one
    plain_out = tmp_path / "plain.png"
    assert "emission maps:" not in _main(js, plain_out, False)
    plain = np.asarray(Image.open(plain_out))
    ref_plain, variant, _ = _device_image(gpu_device, js, None, None)
    assert variant == 2 and np.array_equal(plain, ref_plain)
    assert (plain != img).any(-1).mean() > 0.2
