"""What rebuilding normals buys (include/glrtx.h "Rebuilding normals"), without a GPU, by the CPU statement and the oracle's renders: the unit icosphere at
subdivision 3 morphed into the ellipsoid y -> 2 y by a target with dpos = (0, y, 0), dnormal = 0, weight 1.  The normals the scene keeps (the sphere's) against
the normals rebuilt from the moved faces, both measured against the ellipsoid's analytic normal: as angles, and as the RMSE of the image rendered with them
against the image rendered with the analytic normals (64 x 64, 32 frames, depth 4, the same seeds), for a diffuse and for a conductor (alpha 0.2) ellipsoid.
The angles and errors are taken in float64 from the fp32 statement's words.  And the rest pose of the headline: the rebuilt normals lie within 1 degree of the
stored ones."""
import numpy as np
import pytest

from glrt_amd import host, scenes
from test_reproject_motion_host import moved_scene

SUBDIV, SIZE, FRAMES, DEPTH = 3, 64, 32, 4


def _verts(scene):
    return np.ascontiguousarray(np.asarray(scene["vert"], np.float32).reshape(-1, 15))


def _angles(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    a, b = a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)
    return np.degrees(np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1)))


def _ellipsoid_scene(material):
    """The sphere at the origin over a ground quad under a lamp; returns (scene, params, the sphere's vertex indices)."""
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    mat = b.add_material(material)
    lamp = b.add_material(scenes.emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*scenes.quad((-10, -2.2, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*scenes.icosphere(SUBDIV, 1.0, (0.0, 0.0, 0.0)), mat)
    b.add_mesh(*scenes.quad((-1.5, 5, -1.5), (3, 0, 0), (0, 0, 3)), lamp)
    scene = b.build("sah")
    c2w, s2c = scenes.camera((0, 1.5, 7), (0, 0, 0), (0, 1, 0), 40.0, SIZE, SIZE)
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    sphere = np.unique(tri[tri[:, 3] == mat, 0:3].astype(np.int64))
    return scene, scenes.make_params(c2w, s2c, SIZE, SIZE, DEPTH), sphere


def _three_vertex_sets(scene, sphere):
    """(stale, rebuilt, analytic): the morphed positions with the rest normals, with glrt_rebuild_normals' and with the ellipsoid's own."""
    rest = _verts(scene)
    stale = rest.copy()
    stale[sphere, 1] = rest[sphere, 1] + np.float32(1.0) * rest[sphere, 1]  # p + w * dpos, dpos = (0, y, 0), w = 1
    cls, flip, _ = host.normal_topology(rest, scene["tri"])
    rebuilt = host.rebuild_normals(stale, scene["tri"], cls, flip)
    analytic = stale.copy()
    g = stale[sphere, 0:3].astype(np.float64) * [1.0, 0.25, 1.0]  # the gradient of x^2 + (y / 2)^2 + z^2
    analytic[sphere, 3:6] = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    return stale, rebuilt, analytic


def _image(scene, params, vert):
    from oracle import pt_oracle
    s, acc = moved_scene(scene, vert), None
    for f in range(FRAMES):
        acc, _ = pt_oracle.render(s, dict(params, seed=host.frame_seed(f)), accum=acc)
    return acc[..., 0:3].astype(np.float64) / acc[..., 3:4]


def _rmse(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def test_rebuilt_normals_follow_the_ellipsoid():
    scene, _, sphere = _ellipsoid_scene(scenes.diffuse((0.8, 0.3, 0.3)))
    stale, rebuilt, analytic = _three_vertex_sets(scene, sphere)
    other = np.setdiff1d(np.arange(stale.shape[0]), sphere)
    assert (rebuilt[other, 3:6] == stale[other, 3:6]).all() or _angles(rebuilt[other, 3:6], stale[other, 3:6]).max() < 1e-3  # the flat quads keep their normals
    a_stale = _angles(stale[sphere, 3:6], analytic[sphere, 3:6])
    a_new = _angles(rebuilt[sphere, 3:6], analytic[sphere, 3:6])
    print(f"angle to the analytic ellipsoid normal, max / mean: stale {a_stale.max():.2f} / {a_stale.mean():.2f} deg, "
          f"rebuilt {a_new.max():.2f} / {a_new.mean():.2f} deg")
    assert a_new.max() <= 1.5 and a_new.mean() <= 0.5
    assert a_new.max() < 0.1 * a_stale.max() and a_new.mean() < 0.1 * a_stale.mean()


@pytest.mark.parametrize("name,material", [("diffuse", scenes.diffuse((0.8, 0.3, 0.3))),
                                           ("conductor", scenes.conductor(scenes.COPPER["eta"], scenes.COPPER["kappa"], 0.2))])
def test_images_with_rebuilt_normals_are_the_analytic_ones_to_a_tenth_of_the_stale_error(name, material):
    scene, params, sphere = _ellipsoid_scene(material)
    stale, rebuilt, analytic = _three_vertex_sets(scene, sphere)
    ref = _image(scene, params, analytic)
    e_stale, e_new = _rmse(_image(scene, params, stale), ref), _rmse(_image(scene, params, rebuilt), ref)
    print(f"{name}: image RMSE against the analytic-normal image: stale {e_stale:.4f}, rebuilt {e_new:.4f}")
    assert e_stale > 0 and e_new < 0.1 * e_stale


def test_headline_rest_pose_is_rebuilt_within_a_degree():
    scene, _ = scenes.config_headline(64, 36)
    rest = _verts(scene)
    cls, flip, _ = host.normal_topology(rest, scene["tri"])
    a = _angles(host.rebuild_normals(rest, scene["tri"], cls, flip)[:, 3:6], rest[:, 3:6])
    print(f"headline rest pose: rebuilt against stored normals, max / mean {a.max():.2f} / {a.mean():.2f} deg")
    assert a.max() <= 1.0
