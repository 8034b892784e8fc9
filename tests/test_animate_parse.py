"""The animation file's parser (glrt::Scene::parseAnimation, opengl-raytracer_amd/host/scene.cpp) without a GPU, through a probe like the scene parser's: the
shapes' vertex ranges, the matrices as Python reads the same file, the identity for unlisted shapes, the optional camera through the scene camera's own code,
and the two messages for a shape index out of range and a matrix with 11 numbers."""
import json
import subprocess
import sys

import numpy as np
import pytest

import animate_cases as ac
from conftest import assert_bit_equal
from glrt_amd import host


def test_shape_ranges_matrices_and_defaults(tmp_path):
    js, an = ac.write_scene(tmp_path), ac.write_animation(tmp_path)
    got = ac.probe(js, an)
    b = ac.builder()
    sizes = [3 * p.shape[0] for p in b._pos]  # three fresh vertices a triangle, shape after shape
    assert got["first_vertex"].tolist() == [0, sizes[0], sizes[0] + sizes[1], sum(sizes)]
    doc = ac.steps_doc()
    want = ac.pose_matrices(doc, 3)
    assert got["matrices"].shape == (3, 3, 12)
    assert_bit_equal(got["matrices"], want, "matrices")
    ident = np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32)
    assert (got["matrices"][:, 2] == ident).all() and (got["matrices"][0, 0] == ident).all()  # not listed: the identity
    assert not (got["matrices"][:, 1] == ident).all(-1).any()
    assert np.float32(0.28) in got["matrices"][0, 1] and got["matrices"][2, 1, 3] == np.float32(1.1)  # doubles cast to float


def test_the_optional_camera_goes_through_the_scene_cameras_code(tmp_path):
    js, an = ac.write_scene(tmp_path, 96, 64), ac.write_animation(tmp_path)
    got = ac.probe(js, an)
    assert got["has_camera"].tolist() == [False, False, True]
    assert not got["view"][:2].any() and not got["proj"][:2].any()
    view, proj, ap, fo = ac.camera_params(ac.CAMERA2, 96, 64)
    assert_bit_equal(got["view"][2], view.reshape(16), "view")
    assert_bit_equal(got["proj"][2], proj.reshape(16), "proj")
    assert got["lens"][2].tolist() == [ap, fo]
    # the same block as the scene file's own camera gives the same matrices there
    doc = json.loads(js.read_text())
    doc["camera"] = ac.CAMERA2
    js2 = tmp_path / "scene2.json"
    js2.write_text(json.dumps(doc))
    import test_scene_parse as tsp
    sc = tsp._probe(js2)
    assert_bit_equal(sc["view"], got["view"][2], "scene view")
    assert_bit_equal(sc["proj"], got["proj"][2], "scene proj")
    assert sc["lens"].tolist() == got["lens"][2].tolist()


def test_an_empty_animation_and_a_step_without_matrices(tmp_path):
    js = ac.write_scene(tmp_path)
    got = ac.probe(js, ac.write_animation(tmp_path, {"steps": []}))
    assert got["matrices"].shape == (0, 3, 12)
    got = ac.probe(js, ac.write_animation(tmp_path, {"steps": [{}, {"matrices": []}]}))
    assert got["matrices"].shape == (2, 3, 12) and (got["matrices"] == ac.pose_matrices({"steps": [{}, {}]}, 3)).all()


def _run(scene_json, animation_json):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); c = (C.c_longlong * 2)();"
            "L.glrt_scene_animation_probe(sys.argv[2].encode(), sys.argv[3].encode(), c, None, None, None, None)")
    return subprocess.run([sys.executable, "-c", code, str(ac.LIB), str(scene_json), str(animation_json)], capture_output=True, text=True, timeout=60)


ROW = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
BAD = [
    ("index-3", {"steps": [{"matrices": [[3] + ROW]}]}, "animation step 0: shape index 3 is out of range (the scene has 3 shapes)"),
    ("index-negative", {"steps": [{}, {"matrices": [[-1] + ROW]}]}, "animation step 1: shape index -1 is out of range (the scene has 3 shapes)"),
    ("index-fraction", {"steps": [{"matrices": [[1.5] + ROW]}]}, "animation step 0: shape index 1.5 is out of range"),
    ("eleven-numbers", {"steps": [{"matrices": [[1] + ROW[:11]]}]}, "animation step 0: a matrix entry is a shape index and 12 numbers, this one has 11"),
    ("thirteen-numbers", {"steps": [{"matrices": [[1] + ROW + [0]]}]}, "a matrix entry is a shape index and 12 numbers, this one has 13"),
    ("a-string", {"steps": [{"matrices": [[1] + ROW[:11] + ["x"]]}]}, "a matrix entry is a shape index and 12 numbers"),
    ("no-steps", {"frames": []}, 'animation: no "steps" array'),
]


@pytest.mark.parametrize("name,doc,message", BAD, ids=[b[0] for b in BAD])
def test_malformed_files_abort_with_a_message(tmp_path, name, doc, message):
    js = ac.write_scene(tmp_path)
    r = _run(js, ac.write_animation(tmp_path, doc))
    assert r.returncode != 0 and "[ERROR]" in r.stderr and message in r.stderr, (r.returncode, r.stderr[-400:])


def test_a_missing_or_broken_file_aborts(tmp_path):
    js = ac.write_scene(tmp_path)
    r = _run(js, tmp_path / "nope.json")
    assert r.returncode != 0 and "nope.json" in r.stderr
    bad = tmp_path / "bad.json"
    bad.write_text('{"steps": [')
    r = _run(js, bad)
    assert r.returncode != 0 and "[ERROR]" in r.stderr and "animation" in r.stderr
    assert _run(js, ac.write_animation(tmp_path)).returncode == 0
