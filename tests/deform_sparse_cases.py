"""What the sparse-target facade tests share (glrt_main --animate with "sparse_targets": true, Scene::parseAnimation): deform_cases' scene with a second target
that moves only the cap of the sphere, animation files with and without the key, and the parser's sparse morph probe."""
from __future__ import annotations

import ctypes as C

import numpy as np

import animate_cases as ac
import deform_cases as dc
from glrt_amd import scenes


def cap_mesh():
    """The sphere of shape 0 with the vertices above y = 1.7 lifted by 0.3; every other vertex, and every normal, as it is: most deltas are exactly zero."""
    pos, nrm = scenes.icosphere(1, 1.0, (0.0, 1.0, 0.0))
    p = np.array(pos, np.float32)
    p[p[..., 1] > 1.7, 1] += np.float32(0.3)
    return p, nrm


def write_targets(directory):
    dc.write_target(directory)
    dc.write_obj(directory / "cap.obj", *cap_mesh())
    lamp_pos, lamp_nrm = dc.builder()._pos[1], dc.builder()._nrm[1]
    dc.write_obj(directory / "lamp_up.obj", lamp_pos + np.float32([0, 0.5, 0]), lamp_nrm)


def steps_doc(sparse, n_targets=3):
    """deform_cases.steps_doc's two steps over n_targets targets going round {egg, cap, lamp_up}; step 0 weighs targets 0 and 1, step 1 targets 1 and 2 (and the
    last, if there are more than three)."""
    doc = dc.steps_doc(False)
    pool = [{"shape": 0, "file": "egg.obj"}, {"shape": 0, "file": "cap.obj"}, {"shape": 1, "file": "lamp_up.obj"}]
    doc["targets"] = [pool[k % 3] for k in range(n_targets)]
    doc["steps"][0]["weights"] = [[0, 0.5], [1, 1.0]]
    doc["steps"][1]["weights"] = [[1, -0.5], [2, 0.75]] + ([[n_targets - 1, 0.25]] if n_targets > 3 else [])
    if sparse:
        doc["sparse_targets"] = True
    return doc


def probe(scene_json, animation_json):
    """dict(sparse, target_shape (targets,), offsets (targets + 1,), vertex (entries,), deltas (entries, 6), weights (steps, targets), n_vert) of
    glrt_scene_morph_sparse_probe."""
    L = C.CDLL(str(ac.LIB))
    fp, ip, llp, u64, u32 = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_longlong), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.glrt_scene_morph_sparse_probe.argtypes = [C.c_char_p, C.c_char_p, llp, ip, u64, u32, fp, fp]
    counts = (C.c_longlong * 5)()
    a = (str(scene_json).encode(), str(animation_json).encode(), counts)
    L.glrt_scene_morph_sparse_probe(*a, None, None, None, None, None)
    n_steps, n_targets, n_vert, nnz, sparse = (int(v) for v in counts)
    shape = np.zeros(n_targets, np.int32)
    offsets = np.zeros(n_targets + 1, np.uint64)
    vertex = np.zeros(nnz, np.uint32)
    deltas = np.zeros((nnz, 6), np.float32)
    weights = np.zeros((n_steps, n_targets), np.float32)
    L.glrt_scene_morph_sparse_probe(*a, shape.ctypes.data_as(ip), offsets.ctypes.data_as(u64), vertex.ctypes.data_as(u32), deltas.ctypes.data_as(fp),
                                    weights.ctypes.data_as(fp))
    return dict(sparse=bool(sparse), target_shape=shape, offsets=offsets, vertex=vertex, deltas=deltas, weights=weights, n_vert=n_vert)
