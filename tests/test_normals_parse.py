"""The animation file's "rebuild_normals" and "weld" keys (glrt::Scene::parseAnimation) without a GPU, through glrt_scene_normals_probe: both keys are accepted,
a file without them says nothing, and a value that is not true or false, or a weld the parser does not know, is a fatal error that names the key."""
import ctypes as C
import subprocess
import sys

import pytest

import animate_cases as ac
import deform_cases as dc


def _write(tmp_path, **keys):
    js = dc.write_scene(tmp_path)
    dc.write_target(tmp_path)
    doc = dc.steps_doc(True)
    doc.update(keys)
    return js, dc.write_animation(tmp_path, doc)


def _probe(js, an):
    L = C.CDLL(str(ac.LIB))
    L.glrt_scene_normals_probe.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_int)]
    out = (C.c_int * 2)(-1, -1)
    assert L.glrt_scene_normals_probe(str(js).encode(), str(an).encode(), out) == 0
    return out[0], out[1]


def _run(js, an):
    code = "import ctypes as C, sys; L = C.CDLL(sys.argv[1]); o = (C.c_int * 2)(); L.glrt_scene_normals_probe(sys.argv[2].encode(), sys.argv[3].encode(), o)"
    return subprocess.run([sys.executable, "-c", code, str(ac.LIB), str(js), str(an)], capture_output=True, text=True, timeout=60)


def test_the_keys_are_accepted(tmp_path):
    assert _probe(*_write(tmp_path)) == (0, 0)  # a file without the keys
    assert _probe(*_write(tmp_path, rebuild_normals=True)) == (1, 0)
    assert _probe(*_write(tmp_path, rebuild_normals=False)) == (0, 0)
    assert _probe(*_write(tmp_path, rebuild_normals=True, weld="positions")) == (1, 1)
    assert _probe(*_write(tmp_path, rebuild_normals=True, weld="normals")) == (1, 0)
    assert _probe(*_write(tmp_path, rebuild_normals=True, sparse_targets=True)) == (1, 0)


@pytest.mark.parametrize("value", [1, 0, "true", "yes", [True], {"on": True}])
def test_a_rebuild_normals_that_is_not_true_or_false_is_fatal(tmp_path, value):
    r = _run(*_write(tmp_path, rebuild_normals=value))
    assert r.returncode != 0 and "[ERROR]" in r.stderr and '"rebuild_normals" is not true or false' in r.stderr, r.stderr[-400:]


@pytest.mark.parametrize("value", ["position", "Positions", "", 1, True, ["positions"]])
def test_an_unknown_weld_is_fatal(tmp_path, value):
    r = _run(*_write(tmp_path, rebuild_normals=True, weld=value))
    assert r.returncode != 0 and "[ERROR]" in r.stderr and '"weld" is not "positions" or "normals"' in r.stderr, r.stderr[-400:]
