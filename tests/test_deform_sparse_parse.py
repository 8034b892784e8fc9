"""The animation file's "sparse_targets": true (glrt::Scene::parseAnimation) without a GPU, through glrt_scene_morph_sparse_probe: 65 targets parse; the index
the parser builds directly from the target OBJs is glrt_morph_sparsify of the deltas the same targets give through the dense path; without the key 65 targets
are the fatal error they were, word for word."""
import json
import subprocess
import sys

import numpy as np

import animate_cases as ac
import deform_cases as dc
import deform_sparse_cases as sc
from glrt_amd import host


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _write(tmp_path, doc, name="morph.json"):
    js = dc.write_scene(tmp_path)
    sc.write_targets(tmp_path)
    return js, dc.write_animation(tmp_path, doc, name=name)


def test_sixty_five_sparse_targets_parse(tmp_path):
    js, an = _write(tmp_path, sc.steps_doc(True, 65))
    got = sc.probe(js, an)
    assert got["sparse"] and got["target_shape"].tolist() == [[0, 0, 1][k % 3] for k in range(65)]
    assert got["offsets"][0] == 0 and (np.diff(got["offsets"].astype(np.int64)) > 0).all() and int(got["offsets"][-1]) == got["vertex"].size
    assert got["weights"].shape == (2, 65) and got["weights"][1, 64] == 0.25 and got["weights"][0, 0] == 0.5 and not got["weights"][0, 2:].any()
    per = np.diff(got["offsets"].astype(np.int64))
    assert (per[0::3] == per[0]).all() and (per[1::3] == per[1]).all() and (per[2::3] == 6).all()
    dense = dc.probe(js, an)  # the dense array is never built for such a file
    assert dense["target_shape"].size == 65 and not dense["deltas"].any()


def test_the_parsed_index_is_sparsify_of_the_dense_parse(tmp_path):
    js, an = _write(tmp_path, sc.steps_doc(True))
    _, an_dense = _write(tmp_path, sc.steps_doc(False), name="dense.json")
    got, dense = sc.probe(js, an), dc.probe(js, an_dense)
    assert got["sparse"] and not sc.probe(js, an_dense)["sparse"] and sc.probe(js, an_dense)["vertex"].size == 0
    o, v, d = host.morph_sparsify(dense["deltas"])
    assert got["offsets"].tolist() == o.tolist() and got["vertex"].tolist() == v.tolist()
    assert (_bits(got["deltas"]) == _bits(d)).all()
    assert (got["weights"] == dense["weights"]).all() and got["target_shape"].tolist() == dense["target_shape"].tolist() == [0, 0, 1]
    n0 = 3 * dc.builder()._pos[0].shape[0]
    per = np.diff(o.astype(np.int64)).tolist()
    assert 0 < per[1] < per[0] <= n0 and per[2] == 6  # the cap moves a few vertices of the sphere, the egg nearly all of them, the lamp target the lamp
    assert (v[int(o[2]):] >= n0).all() and (v[:int(o[2])] < n0).all()
    cap = d[int(o[1]):int(o[2])]
    assert (cap[:, 1] != 0).all() and not cap[:, [0, 2, 3, 4, 5]].any()


def _run(scene_json, animation_json):
    code = ("import ctypes as C, sys; L = C.CDLL(sys.argv[1]); c = (C.c_longlong * 5)();"
            "L.glrt_scene_morph_sparse_probe(sys.argv[2].encode(), sys.argv[3].encode(), c, None, None, None, None, None)")
    return subprocess.run([sys.executable, "-c", code, str(ac.LIB), str(scene_json), str(animation_json)], capture_output=True, text=True, timeout=60)


def test_without_the_key_the_limit_is_what_it_was(tmp_path):
    js, an = _write(tmp_path, sc.steps_doc(False, 65))
    r = _run(js, an)
    assert r.returncode != 0 and "[ERROR]" in r.stderr and "animation: 65 morph targets (at most 64)" in r.stderr, r.stderr[-400:]
    doc = sc.steps_doc(False, 65)
    doc["sparse_targets"] = False  # the key set to false is the key left out
    r = _run(*_write(tmp_path, doc))
    assert r.returncode != 0 and "animation: 65 morph targets (at most 64)" in r.stderr, r.stderr[-400:]
    assert _run(*_write(tmp_path, sc.steps_doc(True, 65))).returncode == 0
    r = _run(*_write(tmp_path, sc.steps_doc(True, 1025)))
    assert r.returncode != 0 and "animation: 1025 sparse morph targets (at most 1024)" in r.stderr, r.stderr[-400:]
    doc = sc.steps_doc(False)
    doc["sparse_targets"] = 1
    r = _run(*_write(tmp_path, doc))
    assert r.returncode != 0 and '"sparse_targets" is not true or false' in r.stderr, r.stderr[-400:]
