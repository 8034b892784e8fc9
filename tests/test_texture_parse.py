"""The scene file's "texture" block (glrt::Scene::parse, host/scene.h; host/texture_file.h) without a GPU, through glrt_scene_texture_probe: the block and its
defaults, both file readers and the PPM's row flip, the vt coordinates in the vertex buffer, the fatal errors that name the key, and the key ignored with
extensions off."""
import ctypes as C
import json
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
        tex = rng.integers(0, 256, (4, 5, 3), dtype=np.uint8)
        scenes.write_ppm(tmp_path / "wall.ppm", tex)
    else:
        tex = rng.uniform(0, 2, (4, 5, 3)).astype(np.float32)
        scenes.write_pfm(tmp_path / "wall.pfm", tex)
    uv = rng.uniform(-1, 2, (2 * N * N, 3, 2)).astype(np.float32)
    scene, params, wall = scenes.config_textured_wall(n=N, uv=uv, texture=block)
    js = scenes.export_json_obj(wall["builder"], tmp_path, 64, 48, *wall["camera"])
    return js, scene, wall, tex


def _probe(js, extensions=1):
    L = C.CDLL(str(LIB))
    L.glrt_scene_texture_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]
    counts = (C.c_longlong * 2)()
    info = np.zeros((8, 7), np.int32)
    texels = np.zeros(1 << 16, np.uint8)
    assert L.glrt_scene_texture_probe(str(js).encode(), extensions, counts, info.ctypes.data_as(C.POINTER(C.c_int)), texels.ctypes.data, texels.size) == 0
    return int(counts[0]), int(counts[1]), info, texels


def _run(js, extensions=1):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); c = (C.c_longlong * 2)(); "
            "L.glrt_scene_texture_probe.argtypes = [C.c_char_p, C.c_int, C.POINTER(C.c_longlong), C.c_void_p, C.c_void_p, C.c_size_t]; "
            "L.glrt_scene_texture_probe(sys.argv[2].encode(), int(sys.argv[3]), c, None, None, 0)")
    return subprocess.run([sys.executable, "-c", code, str(LIB), str(js), str(extensions)], capture_output=True, text=True, timeout=60)


def test_the_block_and_the_ppm_reader(tmp_path):
    js, scene, wall, tex = _write(tmp_path, {"file": "wall.ppm", "filter": "nearest", "wrap": "clamp", "srgb": False})
    n, n_mat, info, texels = _probe(js)
    assert (n, n_mat) == (1, 4)
    assert info[0].tolist() == [wall["material"], 5, 4, host.TEX_RGBA8_UNORM, host.TEX_CLAMP, host.TEX_NEAREST, 5 * 4 * 4]
    got = texels[:80].reshape(4, 5, 4)
    assert np.array_equal(got[..., :3], tex) and (got[..., 3] == 255).all()  # row 0 is t = 0: the file's LAST row
    raw = (tmp_path / "wall.ppm").read_bytes()
    assert raw.startswith(b"P6\n5 4\n255\n") and raw[-15:] == tex[0].tobytes()  # ... and the top row of the file is t = 1
    # the defaults: bilinear, repeat, sRGB
    js, _, _, _ = _write(tmp_path, {"file": "wall.ppm"})
    assert _probe(js)[2][0].tolist()[3:6] == [host.TEX_RGBA8_SRGB, host.TEX_REPEAT, host.TEX_BILINEAR]
    # a header with a comment and other whitespace
    (tmp_path / "wall.ppm").write_bytes(b"P6 # made by hand\n5\t4\n# another\n255 " + tex[::-1].tobytes())
    assert np.array_equal(_probe(js)[3][:80].reshape(4, 5, 4)[..., :3], tex)


def test_the_pfm_reader(tmp_path):
    js, scene, wall, tex = _write(tmp_path, {"file": "wall.pfm", "srgb": True}, image="pfm")
    n, _, info, texels = _probe(js)
    assert n == 1 and info[0].tolist() == [wall["material"], 5, 4, host.TEX_RGBA32F, host.TEX_REPEAT, host.TEX_BILINEAR, 5 * 4 * 16]
    got = texels[:320].view(np.float32).reshape(4, 5, 4)
    assert np.array_equal(got[..., :3].view(np.uint32), tex.view(np.uint32)) and (got[..., 3] == 1).all()  # a PFM's rows already run from the bottom up
    (tmp_path / "wall.pfm").write_bytes(b"PF\n5 4\n1.0\n" + tex.astype(">f4").tobytes())  # big-endian
    assert np.array_equal(_probe(js)[3][:320].view(np.float32).reshape(4, 5, 4)[..., :3], tex)
    (tmp_path / "wall.pfm").write_bytes(b"Pf\n5 4\n-1.0\n" + tex[..., 0].astype("<f4").tobytes())  # one channel
    assert np.array_equal(_probe(js)[3][:320].view(np.float32).reshape(4, 5, 4)[..., :3], np.repeat(tex[..., :1], 3, -1))


def test_the_obj_coordinates_reach_the_vertex_buffer(tmp_path):
    js, scene, wall, _ = _write(tmp_path, {"file": "wall.ppm"})
    got = scene_probe(js)
    want = scene["vert"].reshape(-1, 15)
    assert np.array_equal(got["vert"][:, 6:8].view(np.uint32), want[:, 6:8].view(np.uint32)) and want[wall["vert"].start:, 6:8].any()
    assert not got["vert"][: wall["vert"].start, 6:9].any() and np.array_equal(got["tri"], scene["tri"].reshape(-1, 4))


def test_the_key_is_ignored_with_extensions_off(tmp_path):
    js, _, _, _ = _write(tmp_path, {"file": "missing.ppm", "filter": 7})
    n, n_mat, _, _ = _probe(js, extensions=0)
    assert (n, n_mat) == (0, 4)
    plain = scenes.export_json_obj(scenes.config_textured_wall(n=N)[2]["builder"], tmp_path / "plain", 64, 48, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)
    assert _probe(plain, extensions=1)[:2] == (0, 4)  # a file without the key, extensions on
    a, b = scene_probe(js), scene_probe(plain)
    assert np.array_equal(a["mat"], b["mat"]) and np.array_equal(a["nodes"], b["nodes"])


@pytest.mark.parametrize("block,words", [
    ("wall.ppm", '"texture" is not an object'),
    ({"filter": "nearest"}, '"texture" has no "file" string'),
    ({"file": 3}, '"texture" has no "file" string'),
    ({"file": "missing.ppm"}, 'texture "file": cannot open'),
    ({"file": "shape0.obj"}, 'texture "file": '),
    ({"file": "wall.ppm", "filter": "linear"}, 'texture "filter" is not "bilinear" or "nearest"'),
    ({"file": "wall.ppm", "filter": 1}, 'texture "filter" is not "bilinear" or "nearest"'),
    ({"file": "wall.ppm", "wrap": "mirror"}, 'texture "wrap" is not "repeat" or "clamp"'),
    ({"file": "wall.ppm", "srgb": "yes"}, 'texture "srgb" is not true or false'),
    ({"file": "wall.ppm", "srgb": 1}, 'texture "srgb" is not true or false'),
])
def test_fatal_errors_name_the_key(tmp_path, block, words):
    js, _, _, _ = _write(tmp_path, block)
    r = _run(js)
    assert r.returncode != 0 and "[ERROR]" in r.stderr and words in r.stderr, r.stderr[-400:]
    assert _run(js, extensions=0).returncode == 0


@pytest.mark.parametrize("data,words", [
    (b"P5\n5 4\n255\n" + bytes(20), "neither a binary PPM"),
    (b"P6\n5 4\n65535\n" + bytes(120), "maxval 65535"),
    (b"P6\n0 4\n255\n", "width and height must be 1 .. 16384"),
    (b"P6\n5 4\n255\n" + bytes(59), "the file ends before its 20 pixels do"),
    (b"PF\n5 4\n0\n" + bytes(240), "bad PFM scale"),
    (b"PF\n5 4\n-1.0\n" + bytes(239), "the file ends before its 20 pixels do"),
])
def test_a_broken_image_file_is_fatal(tmp_path, data, words):
    js, _, _, _ = _write(tmp_path, {"file": "wall.ppm"})
    (tmp_path / "wall.ppm").write_bytes(data)
    r = _run(js)
    assert r.returncode != 0 and 'texture "file"' in r.stderr and words in r.stderr, r.stderr[-400:]
