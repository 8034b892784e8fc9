"""What the morph-target facade tests share (glrt_main --animate with "targets", Scene::parseAnimation): a small scene of two OBJ shapes -- a copper icosphere
and its lamp --, a target OBJ for the sphere, the animation file, and the parser's morph probe."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

import animate_cases as ac
from glrt_amd import scenes

CAMERA = dict(origin=(0, 2, 7), target=(0, 1, 0), up=(0, 1, 0), fov=40.0)


def builder():
    """Shape 0: a copper icosphere; shape 1: the lamp above it."""
    b = scenes.SceneBuilder()
    cu = b.add_material(scenes.conductor(scenes.COPPER["eta"], scenes.COPPER["kappa"], 0.2))
    lamp = b.add_material(scenes.emitter((10.0, 9.0, 8.0)))
    b.add_mesh(*scenes.icosphere(1, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*scenes.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    return b


def write_scene(directory, width=64, height=48):
    return scenes.export_json_obj(builder(), directory, width, height, CAMERA["origin"], CAMERA["target"], CAMERA["up"], CAMERA["fov"])


def write_obj(path, pos, nrm):
    """One OBJ the way scenes.export_json_obj writes a shape: three fresh vertices and normals a triangle, 9 significant digits."""
    pos, nrm = np.asarray(pos, np.float32).reshape(-1, 3), np.asarray(nrm, np.float32).reshape(-1, 3)
    lines = ["v %.9g %.9g %.9g" % tuple(p) for p in pos] + ["vn %.9g %.9g %.9g" % tuple(n) for n in nrm]
    lines += [f"f {a}//{a} {a + 1}//{a + 1} {a + 2}//{a + 2}" for a in range(1, pos.shape[0] + 1, 3)]
    path.write_text("\n".join(lines) + "\n")
    return path


def target_mesh():
    """The sphere of shape 0 pulled into an egg: y stretched about the centre by 1.5, x squeezed by 0.8; normals of the ellipsoid."""
    pos, nrm = scenes.icosphere(1, 1.0, (0.0, 1.0, 0.0))
    c = np.array([0.0, 1.0, 0.0])
    p = (pos.astype(np.float64) - c) * np.array([0.8, 1.5, 1.0]) + c
    n = nrm.astype(np.float64) / np.array([0.8, 1.5, 1.0])
    return p.astype(np.float32), (n / np.linalg.norm(n, axis=-1, keepdims=True)).astype(np.float32)


def write_target(directory, name="egg.obj"):
    return write_obj(directory / name, *target_mesh())


def steps_doc(targets=True):
    """Two steps: the sphere (shape 0) half-way to the egg and shifted, then a little past it (weight 1.25); without `targets`, the same matrices alone."""
    m0 = [0, 1, 0, 0, 0.25, 0, 1, 0, 0, 0, 0, 1, 0]
    m1 = [0, 0.96, 0, -0.28, -0.5, 0, 1, 0, 0.125, 0.28, 0, 0.96, 0]
    doc = {"steps": [{"matrices": [m0]}, {"matrices": [m1]}]}
    if targets:
        doc["targets"] = [{"shape": 0, "file": "egg.obj"}]
        doc["steps"][0]["weights"] = [[0, 0.5]]
        doc["steps"][1]["weights"] = [[0, 1.25]]
    return doc


def write_animation(directory, doc=None, name="morph.json"):
    p = directory / name
    p.write_text(json.dumps(steps_doc() if doc is None else doc))
    return p


def probe(scene_json, animation_json):
    """dict(target_shape (targets,), deltas (targets, vertices, 6), weights (steps, targets)) of glrt_scene_morph_probe."""
    L = C.CDLL(str(ac.LIB))
    fp, ip, llp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_longlong)
    L.glrt_scene_morph_probe.argtypes = [C.c_char_p, C.c_char_p, llp, ip, fp, fp]
    counts = (C.c_longlong * 3)()
    L.glrt_scene_morph_probe(str(scene_json).encode(), str(animation_json).encode(), counts, None, None, None)
    n_steps, n_targets, n_vert = (int(v) for v in counts)
    shape = np.zeros(n_targets, np.int32)
    deltas = np.zeros((n_targets, n_vert, 6), np.float32)
    weights = np.zeros((n_steps, n_targets), np.float32)
    L.glrt_scene_morph_probe(str(scene_json).encode(), str(animation_json).encode(), counts, shape.ctypes.data_as(ip), deltas.ctypes.data_as(fp),
                             weights.ctypes.data_as(fp))
    return dict(target_shape=shape, deltas=deltas, weights=weights)
