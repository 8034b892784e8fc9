"""The scene file's "cutout" block (glrt::Scene::parse, host/scene.h: CutoutSpec) without a GPU, through glrt_scene_cutout_probe: the block and its defaults on
a diffuse and on a conductor shape, both image formats, the fatal errors that name the shape and the key, and the key ignored with extensions off."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import host, scenes
from test_scene_parse import _probe as scene_probe

LIB = PKG / "lib" / "libglrt.so"
N = 3


def _write(tmp_path, block, image="ppm"):
    rng = np.random.default_rng(4)
    if image == "ppm":
        scenes.write_ppm(tmp_path / "mask.ppm", rng.integers(0, 256, (4, 5, 3), dtype=np.uint8))
    else:
        scenes.write_pfm(tmp_path / "mask.pfm", rng.uniform(0, 1, (4, 5, 3)).astype(np.float32))
    uv = rng.uniform(-1, 2, (2 * N * N, 3, 2)).astype(np.float32)
    scene, params, wall = scenes.config_cutout_wall(n=N, uv=uv, cutout=block)
    return scenes.export_json_obj(wall["builder"], tmp_path, 64, 48, *wall["camera"]), wall


def _probe(js, extensions=1):
    L = C.CDLL(str(LIB))
    L.glrt_scene_cutout_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]
    info, cutoff = np.zeros((8, 7), np.int32), np.zeros(8, np.float32)
    n = L.glrt_scene_cutout_probe(str(js).encode(), extensions, info.ctypes.data_as(C.POINTER(C.c_int)), cutoff.ctypes.data_as(C.POINTER(C.c_float)), 8)
    return n, info, cutoff


def _run(js, extensions=1):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); "
            "L.glrt_scene_cutout_probe.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]; "
            "L.glrt_scene_cutout_probe(sys.argv[2].encode(), int(sys.argv[3]), None, None, 0)")
    return subprocess.run([sys.executable, "-c", code, str(LIB), str(js), str(extensions)], capture_output=True, text=True, timeout=60)


def test_the_block_and_its_defaults(tmp_path):
    js, wall = _write(tmp_path, {"file": "mask.ppm", "channel": "g", "cutoff": 0.25, "filter": "nearest", "wrap": "clamp"})
    n, info, cutoff = _probe(js)
    assert n == 1 and info[0].tolist() == [wall["material"], 1, 5, 4, host.TEX_RGBA8_UNORM, host.TEX_CLAMP, host.TEX_NEAREST] and cutoff[0] == np.float32(0.25)
    js, wall = _write(tmp_path, {"file": "mask.ppm"})  # the defaults: channel r, cutoff 0.5, bilinear, repeat; a PPM is linear
    n, info, cutoff = _probe(js)
    assert n == 1 and info[0].tolist() == [wall["material"], 0, 5, 4, host.TEX_RGBA8_UNORM, host.TEX_REPEAT, host.TEX_BILINEAR] and cutoff[0] == np.float32(0.5)
    js, wall = _write(tmp_path, {"file": "mask.pfm", "channel": "b", "srgb": False, "cutoff": -1}, image="pfm")
    n, info, cutoff = _probe(js)
    assert n == 1 and info[0].tolist()[:5] == [wall["material"], 2, 5, 4, host.TEX_RGBA32F] and cutoff[0] == -1.0


def test_a_conductor_shape_takes_one_and_the_texture_block_stays(tmp_path):
    scenes.write_ppm(tmp_path / "mask.ppm", np.full((2, 2, 3), 200, np.uint8))
    _, _, wall = scenes.config_mapped_wall(n=N)
    wall["builder"].materials[wall["material"]]["cutout"] = {"file": "mask.ppm"}
    wall["builder"].materials[1]["cutout"] = {"file": "mask.ppm", "channel": "b"}  # the copper sphere
    js = scenes.export_json_obj(wall["builder"], tmp_path, 64, 48, *wall["camera"])
    n, info, _ = _probe(js)
    assert n == 2 and info[:2, :2].tolist() == [[1, 2], [wall["material"], 0]]  # in shape order


def test_the_key_is_ignored_with_extensions_off(tmp_path):
    js, _ = _write(tmp_path, {"file": "missing.ppm", "channel": 7})
    assert _probe(js, extensions=0)[0] == 0
    plain = scenes.export_json_obj(scenes.config_textured_wall(n=N)[2]["builder"], tmp_path / "plain", 64, 48, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)
    assert _probe(plain, extensions=1)[0] == 0  # a file without the key, extensions on
    a, b = scene_probe(js), scene_probe(plain)
    assert np.array_equal(a["mat"], b["mat"]) and np.array_equal(a["nodes"], b["nodes"])


@pytest.mark.parametrize("block,words", [
    ("mask.ppm", 'shape 3: "cutout" is not an object'),
    ({"channel": "r"}, 'shape 3: "cutout" has no "file" string'),
    ({"file": 3}, 'shape 3: "cutout" has no "file" string'),
    ({"file": "missing.ppm"}, 'shape 3: cutout "file": cannot open'),
    ({"file": "shape0.obj"}, 'shape 3: cutout "file": '),
    ({"file": "mask.ppm", "filter": "linear"}, 'shape 3: cutout "filter" is not "bilinear" or "nearest"'),
    ({"file": "mask.ppm", "wrap": "mirror"}, 'shape 3: cutout "wrap" is not "repeat" or "clamp"'),
    ({"file": "mask.ppm", "wrap": 0}, 'shape 3: cutout "wrap" is not "repeat" or "clamp"'),
    ({"file": "mask.ppm", "srgb": True}, 'shape 3: cutout "srgb": a mask holds coverage'),
    ({"file": "mask.ppm", "channel": "a"}, 'shape 3: cutout "channel" is not "r", "g" or "b"'),
    ({"file": "mask.ppm", "channel": 3}, 'shape 3: cutout "channel" is not "r", "g" or "b"'),
    ({"file": "mask.ppm", "cutoff": "half"}, 'shape 3: cutout "cutoff" is not a finite number'),
    ({"file": "mask.ppm", "cutoff": 1e60}, 'shape 3: cutout "cutoff" is not a finite number'),
])
def test_fatal_errors_name_the_shape_and_the_key(tmp_path, block, words):
    js, _ = _write(tmp_path, block)
    r = _run(js)
    assert r.returncode != 0 and "[ERROR]" in r.stderr and words in r.stderr, r.stderr[-400:]
    assert _run(js, extensions=0).returncode == 0


def test_a_cutout_on_an_emitter_is_fatal(tmp_path):
    scenes.write_ppm(tmp_path / "mask.ppm", np.full((2, 2, 3), 200, np.uint8))
    _, _, wall = scenes.config_textured_wall(n=N)
    wall["builder"].materials[2]["cutout"] = {"file": "mask.ppm"}  # the lamp
    js = scenes.export_json_obj(wall["builder"], tmp_path, 64, 48, *wall["camera"])
    r = _run(js)
    assert r.returncode != 0 and 'shape 2: "cutout" on a emitter shape (a diffuse or conductor shape takes one)' in r.stderr, r.stderr[-400:]
