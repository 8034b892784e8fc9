"""The animation file's morph targets (glrt::Scene::parseAnimation, opengl-raytracer_amd/host/scene.cpp) without a GPU, through glrt_scene_morph_probe: the
targets' shapes, the deltas as target - rest of what the scene's own OBJ loader yields, zero outside the shape, the weights per step with 0 for targets a step
does not list, a file without targets, and the messages of the malformed cases -- the vertex-count error names both counts."""
import subprocess
import sys

import numpy as np
import pytest

import animate_cases as ac
import deform_cases as dc
from test_scene_parse import _probe


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_targets_deltas_and_weights(tmp_path):
    js = dc.write_scene(tmp_path)
    dc.write_target(tmp_path)
    got = dc.probe(js, dc.write_animation(tmp_path))
    first = ac.probe(js, tmp_path / "morph.json")["first_vertex"].tolist()
    n0 = 3 * dc.builder()._pos[0].shape[0]
    assert first == [0, n0, n0 + 6]
    assert got["target_shape"].tolist() == [0] and got["deltas"].shape == (1, n0 + 6, 6)
    assert got["weights"].tolist() == [[0.5], [1.25]]
    # the delta is target - rest, one float subtraction each, of what loadObj gives for either file: the target parsed as a scene of its own
    rest = _probe(js)["vert"].reshape(-1, 15)
    doc = __import__("json").loads(js.read_text())
    doc["scene"][0]["filename"] = "egg.obj"
    (tmp_path / "egg_scene.json").write_text(__import__("json").dumps(doc))
    egg = _probe(tmp_path / "egg_scene.json")["vert"].reshape(-1, 15)
    want = egg[:n0, 0:6] - rest[:n0, 0:6]
    assert (_bits(got["deltas"][0, :n0]) == _bits(want)).all()
    assert np.abs(want[:, 0:3]).max() > 0.4 and np.abs(want[:, 3:6]).max() > 0.05
    assert not got["deltas"][0, n0:].any()  # zero outside the shape
    assert (_bits(got["deltas"][0, n0:]) == 0).all()


def test_unlisted_targets_get_zero_and_two_targets_keep_their_order(tmp_path):
    js = dc.write_scene(tmp_path)
    dc.write_target(tmp_path)
    lamp_pos, lamp_nrm = dc.builder()._pos[1], dc.builder()._nrm[1]
    dc.write_obj(tmp_path / "lamp_up.obj", lamp_pos + np.float32([0, 0.5, 0]), lamp_nrm)
    doc = dc.steps_doc()
    doc["targets"] = [{"shape": 1, "file": "lamp_up.obj"}, {"shape": 0, "file": "egg.obj"}]
    doc["steps"] = [{"weights": [[1, 0.75]]}, {}, {"weights": [[0, -2], [1, 1e-3]]}]
    got = dc.probe(js, dc.write_animation(tmp_path, doc))
    n0 = 3 * dc.builder()._pos[0].shape[0]
    assert got["target_shape"].tolist() == [1, 0]
    assert got["weights"].tolist() == [[0.0, 0.75], [0.0, 0.0], [-2.0, np.float32(1e-3)]]
    assert not got["deltas"][0, :n0].any() and (got["deltas"][0, n0:, 1] == 0.5).all() and not got["deltas"][0, n0:, [0, 2, 3, 4, 5]].any()
    assert got["deltas"][1, :n0].any() and not got["deltas"][1, n0:].any()


def test_a_file_without_targets_has_none(tmp_path):
    js = dc.write_scene(tmp_path)
    got = dc.probe(js, dc.write_animation(tmp_path, dc.steps_doc(targets=False)))
    assert got["target_shape"].size == 0 and got["deltas"].shape[0] == 0 and got["weights"].shape == (2, 0)
    plain = ac.probe(js, tmp_path / "morph.json")  # and the existing probe reads the file as before
    assert plain["matrices"].shape == (2, 2, 12)


def _run(scene_json, animation_json):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); c = (C.c_longlong * 3)();"
            "L.glrt_scene_morph_probe(sys.argv[2].encode(), sys.argv[3].encode(), c, None, None, None)")
    return subprocess.run([sys.executable, "-c", code, str(ac.LIB), str(scene_json), str(animation_json)], capture_output=True, text=True, timeout=60)


def _doc(**kw):
    d = dc.steps_doc()
    d.update(kw)
    return d


BAD = [
    ("vertex-count", _doc(targets=[{"shape": 1, "file": "egg.obj"}]), "egg.obj has 240 vertices, shape 1 has 6"),
    ("shape-2", _doc(targets=[{"shape": 2, "file": "egg.obj"}]), "animation target 0: shape index 2 is out of range (the scene has 2 shapes)"),
    ("shape-missing", _doc(targets=[{"file": "egg.obj"}]), "animation target 0: shape index"),
    ("no-file", _doc(targets=[{"shape": 0, "file": "nope.obj"}]), "nope.obj"),
    ("targets-not-an-array", _doc(targets={"shape": 0}), '"targets" is not an array'),
    ("sixty-five", _doc(targets=[{"shape": 0, "file": "egg.obj"}] * 65), "65 morph targets (at most 64)"),
    ("target-index-1", _doc(steps=[{"weights": [[1, 0.5]]}]), "animation step 0: target index 1 is out of range (the file has 1 targets)"),
    ("weight-not-a-number", _doc(steps=[{}, {"weights": [[0, "x"]]}]), "animation step 1: a weight entry is a target index and a number"),
    ("weight-three-entries", _doc(steps=[{"weights": [[0, 1, 2]]}]), "a weight entry is a target index and a number"),
]


@pytest.mark.parametrize("name,doc,message", BAD, ids=[b[0] for b in BAD])
def test_malformed_files_abort_with_a_message(tmp_path, name, doc, message):
    js = dc.write_scene(tmp_path)
    dc.write_target(tmp_path)
    r = _run(js, dc.write_animation(tmp_path, doc))
    assert r.returncode != 0 and "[ERROR]" in r.stderr and message in r.stderr, (r.returncode, r.stderr[-400:])
    assert _run(js, dc.write_animation(tmp_path)).returncode == 0
