"""The host side of the volume branch without a GPU: the C++ VOL reader / writer (host/volume.cpp), the "volume" block of a media shape in
Scene::parse, and glrt_main's --enable-volume switch."""
import ctypes as C
import json
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, assert_bit_equal
from glrt_amd import scenes

LIB = PKG / "lib" / "libglrt.so"


@pytest.fixture(scope="module")
def L():
    L = C.CDLL(str(LIB))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    L.glrt_vol_read.argtypes = [C.c_char_p, ip, fp, fp, C.c_size_t, C.c_char_p, C.c_size_t]
    L.glrt_vol_write.argtypes = [C.c_char_p, ip, fp, fp]
    L.glrt_scene_volume_probe.argtypes = [C.c_char_p, C.c_int, ip, fp, fp]
    return L


def _p(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def vol_read(L, path, n=1 << 16):
    dims, bbox, data = np.zeros(4, np.int32), np.zeros(6, np.float32), np.zeros(n, np.float32)
    err = C.create_string_buffer(256)
    rc = L.glrt_vol_read(str(path).encode(), _p(dims, C.c_int), _p(bbox), _p(data), n, err, 256)
    return rc, dims, bbox, data, err.value.decode()


def test_cpp_reader_reads_what_the_python_writer_wrote(L, tmp_path):
    g = np.random.default_rng(3).random((5, 7, 12, 2), dtype=np.float32)
    p = tmp_path / "a.vol"
    scenes.write_vol(p, g, (-1, 0, 2), (3, 4, 5))
    rc, dims, bbox, data, _ = vol_read(L, p)
    assert rc == 0 and dims.tolist() == [12, 7, 5, 2]
    assert bbox.tolist() == [-1, 0, 2, 3, 4, 5]
    assert_bit_equal(data[: g.size], g.reshape(-1), "data")


def test_cpp_writer_writes_what_the_python_reader_reads(L, tmp_path):
    g = np.random.default_rng(4).random((3, 4, 6), dtype=np.float32)
    dims, bbox = np.array([6, 4, 3, 1], np.int32), np.array([0, 0, 0, 1, 2, 3], np.float32)
    p = tmp_path / "b.vol"
    assert L.glrt_vol_write(str(p).encode(), _p(dims, C.c_int), _p(bbox), _p(np.ascontiguousarray(g))) == 0
    back, lo, hi = scenes.read_vol(p)
    assert_bit_equal(back[..., 0], g, "grid")
    assert (lo, hi) == ((0, 0, 0), (1, 2, 3))
    q = tmp_path / "c.vol"
    scenes.write_vol(q, g, (0, 0, 0), (1, 2, 3))
    assert p.read_bytes() == q.read_bytes()  # the two writers agree byte for byte


@pytest.mark.parametrize("what,msg", [("magic", "not a VOL"), ("version", "version 2"), ("encoding", "encoding 2"), ("short", "file size")])
def test_cpp_reader_rejects(L, tmp_path, what, msg):
    p = tmp_path / "g.vol"
    scenes.write_vol(p, np.zeros((2, 2, 2), np.float32))
    raw = bytearray(p.read_bytes())
    if what == "magic":
        raw[:3] = b"VOX"
    elif what == "version":
        raw[3] = 2
    elif what == "encoding":
        raw[4:8] = np.array([2], "<i4").tobytes()
    else:
        raw = raw[:-4]
    p.write_bytes(bytes(raw))
    rc, *_, err = vol_read(L, p)
    assert rc == -1 and msg in err


def _scene_with_volume(tmp_path, files=True, header_bbox=(-9, -9, -9, 9, 9, 9)):
    """A media box with a volume block whose bbox differs from the grid files' own headers; a 2-channel density file."""
    b = scenes.SceneBuilder()
    block = {"density": "d.vol", "temperature": "t.vol", "bboxMin": [-1.0, 0.05, -1.0], "bboxMax": [1.0, 2.05, 1.0]}
    fog = b.add_material(scenes.media(block))
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    lamp = b.add_material(scenes.emitter((6.0, 6.0, 6.0)))
    b.add_mesh(*scenes.box((-1, 0.05, -1), (1, 2.05, 1)), fog)
    b.add_mesh(*scenes.quad((-6, 0, 6), (12, 0, 0), (0, 0, -12)), grey)
    b.add_mesh(*scenes.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2)), lamp)
    js = scenes.export_json_obj(b, tmp_path, 32, 24, (0, 2, 6), (0, 1, 0), (0, 1, 0), 40.0)
    d = np.random.default_rng(5).random((4, 3, 5, 2), dtype=np.float32)
    d[..., 1] *= 3.0  # the second channel holds the maximum
    if files:
        scenes.write_vol(tmp_path / "d.vol", d, header_bbox[:3], header_bbox[3:])
        scenes.write_vol(tmp_path / "t.vol", np.full((4, 3, 5), 7.0, np.float32), header_bbox[:3], header_bbox[3:])
    return js, d


def _vprobe(L, js, enable):
    info, bbox, dmax = np.zeros(5, np.int32), np.zeros(6, np.float32), C.c_float(0)
    assert L.glrt_scene_volume_probe(str(js).encode(), int(enable), _p(info, C.c_int), _p(bbox), C.byref(dmax)) == 0
    return info, bbox, dmax.value


def test_parse_keeps_the_volume_block(L, tmp_path):
    js, d = _scene_with_volume(tmp_path)
    assert json.loads(js.read_text())["scene"][0]["volume"]["density"] == "d.vol"
    info, bbox, _ = _vprobe(L, js, False)
    assert info[0] == 1 and info[1] == 0  # kept, files not read without the switch
    assert bbox.tolist() == [np.float32(v) for v in (-1.0, 0.05, -1.0, 1.0, 2.05, 1.0)]  # the JSON's bbox, not the files' headers
    info, bbox, dmax = _vprobe(L, js, True)
    assert info.tolist() == [1, 1, 5, 3, 4]
    assert dmax == float(d.max())  # u_densityMax over every channel of the file


def test_missing_volume_files_matter_only_with_the_switch(L, tmp_path):
    js, _ = _scene_with_volume(tmp_path, files=False)
    info, _, _ = _vprobe(L, js, False)  # parses as today
    assert info[0] == 1 and info[1] == 0
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); i = (C.c_int * 5)(); b = (C.c_float * 6)(); m = C.c_float();"
            "L.glrt_scene_volume_probe(sys.argv[2].encode(), 1, i, b, C.byref(m))")
    r = subprocess.run([sys.executable, "-c", code, str(LIB), str(js)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "d.vol" in (r.stdout + r.stderr)


def test_glrt_main_has_the_volume_switch():
    r = subprocess.run([str(PKG / "lib" / "glrt_main")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--enable-volume" in r.stdout
