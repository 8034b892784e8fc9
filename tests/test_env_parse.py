"""The scene file's "environment" block (glrt::Scene::parse, host/scene.h) without a GPU, through glrt_scene_environment_probe: both layouts, the defaults, the
mode override of glrt_main --env-mode, the fatal errors that name the key, and the key ignored with extensions off."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import host, scenes

LIB = PKG / "lib" / "libglrt.so"
ARGS = "[C.c_char_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]"


def _scene(tmp_path, block):
    _, _, wall = scenes.config_textured_wall(n=2)
    js = scenes.export_json_obj(wall["builder"], tmp_path, 64, 48, *wall["camera"])
    doc = json.loads(js.read_text())
    if block is not None:
        doc["environment"] = block
    js.write_text(json.dumps(doc, indent=1))
    return js


def _probe(js, extensions=1, mode=-1):
    L = C.CDLL(str(LIB))
    L.glrt_scene_environment_probe.argtypes = eval(ARGS)
    info, values, texels = np.zeros(7, np.int32), np.zeros(5, np.float32), np.zeros(1 << 20, np.uint8)
    assert L.glrt_scene_environment_probe(str(js).encode(), extensions, mode, info.ctypes.data, values.ctypes.data, texels.ctypes.data, texels.size) == 0
    return info.tolist(), values.tolist(), texels[:info[6]]


def _run(js, extensions=1, volume=False):
    """A fatal error ends the process: the probe (or glrt_main's parse, for --enable-volume) in a child."""
    if volume:
        return subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--extensions", "--enable-volume", "--frames", "1", "--out", str(js) + ".png"],
                              capture_output=True, text=True, timeout=60)
    code = (f"import ctypes as C, sys; L = C.CDLL(sys.argv[1]); L.glrt_scene_environment_probe.argtypes = {ARGS}; "
            "i = (C.c_int * 7)(); v = (C.c_float * 5)(); L.glrt_scene_environment_probe(sys.argv[2].encode(), int(sys.argv[3]), -1, i, v, None, 0)")
    return subprocess.run([sys.executable, "-c", code, str(LIB), str(js), str(extensions)], capture_output=True, text=True, timeout=60)


def _latlong(seed=2, h=8, w=16):
    return np.random.default_rng(seed).uniform(0, 4, (h, w, 3)).astype(np.float32)  # rows from the top of the picture down, as host.env_from_latlong takes it


def test_a_latlong_file_is_resampled_into_an_octahedral_float_map(tmp_path):
    ll = _latlong()
    scenes.write_pfm(tmp_path / "sky.pfm", ll[::-1])  # (write_pfm takes row 0 as the bottom row)
    js = _scene(tmp_path, {"file": "sky.pfm", "size": 12, "mode": "sampled", "scale": [1.0, 0.5, 2.0], "rotate_y": 90, "light_pick": 0.25, "filter": "nearest"})
    info, values, texels = _probe(js)
    assert info == [1, host.ENV_SAMPLED, 12, host.TEX_RGBA32F, host.TEX_NEAREST, 1, 12 * 12 * 16]
    assert values == [1.0, 0.5, 2.0, 90.0, 0.25]
    assert np.array_equal(texels.view(np.float32).reshape(12, 12, 4), host.env_from_latlong(ll, 12))
    # the defaults: lat-long, 512 a side, escape, scale 1, no turn, light_pick 0.5, bilinear
    info, values, _ = _probe(_scene(tmp_path, {"file": "sky.pfm"}))
    assert info[:6] == [1, host.ENV_ESCAPE, 512, host.TEX_RGBA32F, host.TEX_BILINEAR, 1] and values == [1.0, 1.0, 1.0, 0.0, 0.5]
    # glrt_main --env-mode overrides the file
    assert _probe(js, mode=host.ENV_ESCAPE)[0][1] == host.ENV_ESCAPE and _probe(_scene(tmp_path, {"file": "sky.pfm"}), mode=host.ENV_SAMPLED)[0][1] == host.ENV_SAMPLED


def test_a_latlong_ppm_goes_through_its_formats_decode(tmp_path):
    img = np.random.default_rng(3).integers(0, 256, (6, 12, 3), dtype=np.uint8)
    scenes.write_ppm(tmp_path / "sky.ppm", img[::-1])
    for srgb in (True, False):
        _, _, texels = _probe(_scene(tmp_path, {"file": "sky.ppm", "size": 8, "srgb": srgb}))
        lin = host.srgb_table()[img] if srgb else (img.astype(np.float32) / np.float32(255.0)).astype(np.float32)
        assert np.array_equal(texels.view(np.float32).reshape(8, 8, 4), host.env_from_latlong(lin, 8))


def test_an_octahedral_file_is_the_map(tmp_path):
    tex = np.random.default_rng(5).uniform(0, 4, (6, 6, 3)).astype(np.float32)
    scenes.write_pfm(tmp_path / "oct.pfm", tex)
    info, values, texels = _probe(_scene(tmp_path, {"file": "oct.pfm", "layout": "octahedral", "scale": 3, "size": 99}))
    assert info == [1, host.ENV_ESCAPE, 6, host.TEX_RGBA32F, host.TEX_BILINEAR, 0, 6 * 6 * 16] and values[:3] == [3.0, 3.0, 3.0]
    got = texels.view(np.float32).reshape(6, 6, 4)
    assert np.array_equal(got[..., :3], tex) and (got[..., 3] == 1).all()  # row 0 is t = 0
    tex8 = np.random.default_rng(6).integers(0, 256, (4, 4, 3), dtype=np.uint8)
    scenes.write_ppm(tmp_path / "oct.ppm", tex8)
    info, _, texels = _probe(_scene(tmp_path, {"file": "oct.ppm", "layout": "octahedral", "srgb": False}))
    assert info[2:4] == [4, host.TEX_RGBA8_UNORM] and np.array_equal(texels.reshape(4, 4, 4)[..., :3], tex8)
    assert _probe(_scene(tmp_path, {"file": "oct.ppm", "layout": "octahedral"}))[0][3] == host.TEX_RGBA8_SRGB


def test_with_extensions_off_the_key_is_ignored(tmp_path):
    js = _scene(tmp_path, {"file": "missing.pfm", "mode": "nonsense"})
    info, _, texels = _probe(js, extensions=0)
    assert info == [0, 0, 0, 0, 1, 1, 0] and texels.size == 0
    assert _probe(_scene(tmp_path, None))[0][0] == 0


@pytest.mark.parametrize("block,words", [
    ("a string", '"environment" is not an object'),
    ({}, '"environment" has no "file" string'),
    ({"file": "missing.pfm"}, 'environment "file":'),
    ({"file": "sky.pfm", "layout": "cube"}, 'environment "layout" is not "latlong" or "octahedral"'),
    ({"file": "sky.pfm", "mode": "mis"}, 'environment "mode" is not "escape" or "sampled"'),
    ({"file": "sky.pfm", "filter": 3}, 'environment "filter" is not "bilinear" or "nearest"'),
    ({"file": "sky.pfm", "srgb": "yes"}, 'environment "srgb" is not true or false'),
    ({"file": "sky.pfm", "scale": [1, 2]}, 'environment "scale" is not a number or [r, g, b]'),
    ({"file": "sky.pfm", "rotate_y": "90"}, 'environment "rotate_y" is not a number'),
    ({"file": "sky.pfm", "light_pick": [0.5]}, 'environment "light_pick" is not a number'),
    ({"file": "sky.pfm", "size": 1}, 'environment "size" 1 lies outside 2 .. 16384'),
    ({"file": "sky.pfm", "layout": "octahedral"}, "an octahedral map is square"),
])
def test_fatal_errors_name_the_key(tmp_path, block, words):
    scenes.write_pfm(tmp_path / "sky.pfm", _latlong()[::-1])
    r = _run(_scene(tmp_path, block))
    assert r.returncode != 0 and words in r.stdout + r.stderr, r.stdout + r.stderr


def test_an_environment_and_the_volume_do_not_combine(tmp_path):
    scenes.write_pfm(tmp_path / "sky.pfm", _latlong()[::-1])
    r = _run(_scene(tmp_path, {"file": "sky.pfm", "size": 4}), volume=True)
    assert r.returncode != 0 and "do not combine: the volume branch has its own escape path" in r.stdout + r.stderr, r.stdout + r.stderr
