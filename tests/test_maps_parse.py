"""The scene file's "normal_map" / "roughness_map" blocks (glrt::Scene::parse, host/scene.h: MapSpec) without a GPU, through glrt_scene_map_probe: the blocks and
their defaults, the fatal errors that name the key -- an sRGB map among them --, and the keys ignored with extensions off, as "texture" is."""
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


def _write(tmp_path, normal_map=None, roughness_map=None, wall="conductor"):
    rng = np.random.default_rng(4)
    tmp_path.mkdir(exist_ok=True)
    scenes.write_ppm(tmp_path / "bump.ppm", rng.integers(0, 256, (4, 5, 3), dtype=np.uint8))
    scenes.write_pfm(tmp_path / "bump.pfm", rng.uniform(0, 1, (3, 2, 3)).astype(np.float32))
    scene, params, info = scenes.config_mapped_wall(n=N, wall=wall, uv="corner", normal_map=normal_map, roughness_map=roughness_map)
    return scenes.export_json_obj(info["builder"], tmp_path, 64, 48, *info["camera"]), scene, info


def _probe(js, extensions=1):
    L = C.CDLL(str(LIB))
    L.glrt_scene_map_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_int]
    info = np.zeros((8, 7), np.int32)
    scale = np.zeros(8, np.float32)
    n = L.glrt_scene_map_probe(str(js).encode(), extensions, info.ctypes.data_as(C.POINTER(C.c_int)), scale.ctypes.data_as(C.POINTER(C.c_float)), 8)
    return n, info[:n].tolist(), scale[:n].tolist()


def _run(js, extensions=1):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); "
            "L.glrt_scene_map_probe.argtypes = [C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]; "
            "L.glrt_scene_map_probe(sys.argv[2].encode(), int(sys.argv[3]), None, None, 0)")
    return subprocess.run([sys.executable, "-c", code, str(LIB), str(js), str(extensions)], capture_output=True, text=True, timeout=60)


def test_the_blocks_and_their_defaults(tmp_path):
    js, scene, wall = _write(tmp_path, {"file": "bump.pfm", "filter": "nearest", "wrap": "clamp", "scale": 0.5}, {"file": "bump.ppm"})
    n, info, scale = _probe(js)
    w = wall["material"]
    assert n == 2
    assert info[0] == [w, 0, 2, 3, host.TEX_RGBA32F, host.TEX_CLAMP, host.TEX_NEAREST] and scale[0] == 0.5
    assert info[1] == [w, 1, 5, 4, host.TEX_RGBA8_UNORM, host.TEX_REPEAT, host.TEX_BILINEAR] and scale[1] == 1.0  # a PPM map is linear bytes, never sRGB
    # a normal map alone on a diffuse wall, "srgb": false accepted
    js, _, wall = _write(tmp_path, {"file": "bump.ppm", "srgb": False}, wall="diffuse")
    n, info, scale = _probe(js)
    assert n == 1 and info[0] == [wall["material"], 0, 5, 4, host.TEX_RGBA8_UNORM, host.TEX_REPEAT, host.TEX_BILINEAR] and scale[0] == 1.0
    # the OBJ's vt coordinates reach the vertex buffer
    got = scene_probe(js)
    want = scenes.config_mapped_wall(n=N, wall="diffuse", uv="corner")[0]["vert"].reshape(-1, 15)
    assert np.array_equal(got["vert"][:, 6:8].view(np.uint32), want[:, 6:8].view(np.uint32)) and want[wall["vert"].start:, 6:8].any()


def test_the_keys_are_ignored_with_extensions_off(tmp_path):
    js, _, _ = _write(tmp_path, {"file": "missing.pfm", "filter": 7}, {"file": "bump.ppm", "srgb": True})
    assert _probe(js, extensions=0)[0] == 0
    plain, _, _ = _write(tmp_path / "plain")
    assert _probe(plain, extensions=1)[0] == 0  # a file without the keys, extensions on
    a, b = scene_probe(js), scene_probe(plain)
    assert np.array_equal(a["mat"], b["mat"]) and np.array_equal(a["nodes"], b["nodes"])


@pytest.mark.parametrize("normal_map,roughness_map,wall,words", [
    ({"file": "bump.ppm", "srgb": True}, None, "conductor", 'normal_map "srgb": a map holds vectors, not colours (an sRGB map is refused)'),
    (None, {"file": "bump.ppm", "srgb": True}, "conductor", 'roughness_map "srgb": a map holds vectors, not colours (an sRGB map is refused)'),
    ("bump.ppm", None, "conductor", '"normal_map" is not an object'),
    ({"filter": "nearest"}, None, "conductor", '"normal_map" has no "file" string'),
    (None, {"file": 3}, "conductor", '"roughness_map" has no "file" string'),
    ({"file": "missing.ppm"}, None, "diffuse", 'normal_map "file": cannot open'),
    ({"file": "bump.ppm", "filter": "linear"}, None, "diffuse", 'normal_map "filter" is not "bilinear" or "nearest"'),
    (None, {"file": "bump.ppm", "wrap": "mirror"}, "conductor", 'roughness_map "wrap" is not "repeat" or "clamp"'),
    ({"file": "bump.ppm", "scale": "big"}, None, "conductor", 'normal_map "scale" is not a finite number'),
    (None, {"file": "bump.ppm", "scale": 2.0}, "conductor", 'roughness_map has no "scale"'),
    (None, {"file": "bump.ppm"}, "diffuse", '"roughness_map" on a diffuse shape'),
])
def test_fatal_errors_name_the_key(tmp_path, normal_map, roughness_map, wall, words):
    js, _, _ = _write(tmp_path, normal_map, roughness_map, wall)
    r = _run(js)
    assert r.returncode != 0 and "[ERROR]" in r.stderr and words in r.stderr, r.stderr[-400:]
    assert _run(js, extensions=0).returncode == 0
