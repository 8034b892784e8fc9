"""The scene file's "emission_map" block (glrt::Scene::parse, host/scene.h: emissionMapSpecs) without a GPU, through glrt_scene_emission_probe: the block and
its defaults on an emitter shape, both image formats, the fatal errors that name the shape and the key, the key ignored with extensions off, and the
exporter writing the block."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np

from conftest import PKG
from glrt_amd import host, scenes

LIB = PKG / "lib" / "libglrt.so"
N = 3


def _write(tmp_path, block, image="ppm"):
    rng = np.random.default_rng(4)
    if image == "ppm":
        scenes.write_ppm(tmp_path / "glow.ppm", rng.integers(0, 256, (4, 5, 3), dtype=np.uint8))
    else:
        scenes.write_pfm(tmp_path / "glow.pfm", rng.uniform(0, 1, (4, 5, 3)).astype(np.float32))
    scene, params, wall = scenes.config_emissive_wall(n=N, uv="corner", emission_map=block)
    return scenes.export_json_obj(wall["builder"], tmp_path, 64, 48, *wall["camera"]), wall


def _probe(js, extensions=1):
    L = C.CDLL(str(LIB))
    L.glrt_scene_emission_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.c_int]
    info = np.zeros((8, 6), np.int32)
    n = L.glrt_scene_emission_probe(str(js).encode(), extensions, info.ctypes.data_as(C.POINTER(C.c_int)), 8)
    return n, info


def _run(js, extensions=1):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); "
            "L.glrt_scene_emission_probe.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_int]; "
            "L.glrt_scene_emission_probe(sys.argv[2].encode(), int(sys.argv[3]), None, 0)")
    return subprocess.run([sys.executable, "-c", code, str(LIB), str(js), str(extensions)], capture_output=True, text=True, timeout=60)


def test_the_block_and_its_defaults(tmp_path):
    js, wall = _write(tmp_path, {"file": "glow.ppm", "filter": "nearest", "wrap": "clamp", "srgb": False})
    n, info = _probe(js)
    assert n == 1 and info[0].tolist() == [wall["material"], 5, 4, host.TEX_RGBA8_UNORM, host.TEX_CLAMP, host.TEX_NEAREST]
    js, wall = _write(tmp_path, {"file": "glow.ppm"})  # the defaults, as "texture": bilinear, repeat, a PPM is sRGB
    n, info = _probe(js)
    assert n == 1 and info[0].tolist() == [wall["material"], 5, 4, host.TEX_RGBA8_SRGB, host.TEX_REPEAT, host.TEX_BILINEAR]
    js, wall = _write(tmp_path, {"file": "glow.pfm"}, image="pfm")
    n, info = _probe(js)
    assert n == 1 and info[0].tolist()[:4] == [wall["material"], 5, 4, host.TEX_RGBA32F]


def test_the_exporter_writes_the_block_and_extensions_off_ignore_it(tmp_path):
    block = {"file": "glow.ppm", "filter": "nearest"}
    js, wall = _write(tmp_path, block)
    shapes = json.loads(js.read_text())["scene"]
    carrying = [s for s in shapes if "emission_map" in s]
    assert len(carrying) == 1 and carrying[0]["material"] == "emitter" and carrying[0]["emission_map"] == block
    n, _ = _probe(js, extensions=0)
    assert n == 0
    (tmp_path / "glow.ppm").unlink()  # with extensions off the file is not even opened
    assert _run(js, extensions=0).returncode == 0


def test_fatal_errors_name_the_shape_and_the_key(tmp_path):
    for block, words in [("glow.ppm", '"emission_map" is not an object'), ({"filter": "nearest"}, '"emission_map" has no "file" string'),
                         ({"file": "glow.ppm", "filter": "cubic"}, 'emission_map "filter" is not "bilinear" or "nearest"'),
                         ({"file": "glow.ppm", "wrap": "mirror"}, 'emission_map "wrap" is not "repeat" or "clamp"'),
                         ({"file": "glow.ppm", "srgb": 1}, 'emission_map "srgb" is not true or false'),
                         ({"file": "missing.ppm"}, 'emission_map "file"')]:
        js, wall = _write(tmp_path, {"file": "glow.ppm"})
        doc = json.loads(js.read_text())
        k = next(i for i, s in enumerate(doc["scene"]) if "emission_map" in s)
        doc["scene"][k]["emission_map"] = block
        js.write_text(json.dumps(doc))
        r = _run(js)
        assert r.returncode != 0 and words in r.stdout + r.stderr and f"shape {k}" in r.stdout + r.stderr, (block, r.stdout, r.stderr)
