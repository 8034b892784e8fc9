"""What the animation tests share (glrt_main --animate, Scene::parseAnimation): a small scene of two OBJ shapes and a lamp, its animation file, and the parser probe."""
from __future__ import annotations

import ctypes as C
import json

import numpy as np

from conftest import PKG
from glrt_amd import scenes

LIB = PKG / "lib" / "libglrt.so"
CAMERA = dict(origin=(0, 3, 9), target=(0, 1, 0), up=(0, 1, 0), fov=40.0)
CAMERA2 = {"type": "perspective", "fov": 35.0, "nearClip": 0.1, "farClip": 100.0, "apertureRadius": 0.05, "focalLength": 8.5,
           "lookAt": {"origin": [1.5, 3.5, 8.0], "target": [0.25, 1.0, 0.0], "up": [0, 1, 0]}}


def builder():
    """Shape 0: the ground; shape 1: a copper icosphere; shape 2: the lamp."""
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    cu = b.add_material(scenes.conductor(scenes.COPPER["eta"], scenes.COPPER["kappa"], 0.2))
    lamp = b.add_material(scenes.emitter((10.0, 9.0, 8.0)))
    b.add_mesh(*scenes.quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*scenes.icosphere(1, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*scenes.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    return b


def write_scene(directory, width=64, height=48):
    return scenes.export_json_obj(builder(), directory, width, height, CAMERA["origin"], CAMERA["target"], CAMERA["up"], CAMERA["fov"])


def steps_doc():
    """Three steps: shape 1 translated further each step (and turned a little: decimal literals only, no trigonometry), the camera changed at step 2."""
    def m(dx, dy):
        return [1, 0.96, 0, -0.28, dx, 0, 1, 0, dy, 0.28, 0, 0.96, 0.125]
    return {"steps": [{"matrices": [m(0.3, 0.0)]}, {"matrices": [m(0.7, 0.1), [0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]]},
                      {"matrices": [m(1.1, 0.25)], "camera": CAMERA2}]}


def write_animation(directory, doc=None, name="anim.json"):
    p = directory / name
    p.write_text(json.dumps(steps_doc() if doc is None else doc))
    return p


def probe_lib():
    L = C.CDLL(str(LIB))
    fp, llp = C.POINTER(C.c_float), C.POINTER(C.c_longlong)
    L.glrt_scene_animation_probe.argtypes = [C.c_char_p, C.c_char_p, llp, llp, fp, C.POINTER(C.c_int), fp]
    return L


def probe(scene_json, animation_json):
    """dict(first_vertex (shapes + 1,), matrices (steps, shapes, 12), has_camera (steps,), view / proj (steps, 16), lens (steps, 2))."""
    L = probe_lib()
    counts = (C.c_longlong * 2)()
    L.glrt_scene_animation_probe(str(scene_json).encode(), str(animation_json).encode(), counts, None, None, None, None)
    n_steps, n_shapes = int(counts[0]), int(counts[1])
    first = np.zeros(n_shapes + 1, np.int64)
    mats = np.zeros((n_steps, n_shapes, 12), np.float32)
    has = np.zeros(n_steps, np.int32)
    cams = np.zeros((n_steps, 34), np.float32)
    L.glrt_scene_animation_probe(str(scene_json).encode(), str(animation_json).encode(), counts, first.ctypes.data_as(C.POINTER(C.c_longlong)),
                                 mats.ctypes.data_as(C.POINTER(C.c_float)), has.ctypes.data_as(C.POINTER(C.c_int)), cams.ctypes.data_as(C.POINTER(C.c_float)))
    return dict(first_vertex=first, matrices=mats, has_camera=has.astype(bool), view=cams[:, :16], proj=cams[:, 16:32], lens=cams[:, 32:34])


def pose_matrices(doc, n_shapes):
    """The file's matrices as Python reads them: json's doubles cast to float32, the identity for shapes a step does not list.  (steps, shapes, 12) float32."""
    out = np.tile(np.array([1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0], np.float32), (len(doc["steps"]), n_shapes, 1))
    for s, st in enumerate(doc["steps"]):
        for e in st.get("matrices", []):
            out[s, int(e[0])] = np.asarray(e[1:], np.float64).astype(np.float32)
    return out


def camera_params(cam, width, height):
    """(c2w, s2c, aperture, focal) of a "camera" block, through the host library's look_at / perspective as Scene does."""
    from glrt_amd import host
    view = host.look_at(cam["lookAt"]["origin"], cam["lookAt"]["target"], cam["lookAt"]["up"])
    proj = host.perspective(cam["fov"], np.float32(width) / np.float32(height), cam["nearClip"], cam["farClip"])
    return view, proj, np.float32(cam.get("apertureRadius", 0.0)), np.float32(cam.get("focalLength", 0.0))
