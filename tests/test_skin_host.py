"""The skinning pass's CPU statement (libglrt_host.so: glrt_skin_vertices) without a GPU: against its numpy statement (tests/skin_math.py) bit for bit on hostile
rigs, the two consequences the contract draws (include/glrtx.h "Posing"), and a rigid pose against the geometry it turns -- posed normals stay on the side of the
posed faces, under a rotation and under a reflection."""
import numpy as np
import pytest

import skin_math as sm
from glrt_amd import host, rig, scenes
from reproject_motion_math import vertices_of_material

SIZES = [1, 3, 63, 64, 65, 255, 257, 1000]
BONES = [1, 2, 5, 300]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def hostile_cases():
    return [(n, nb, 1000 * n + nb) for n in SIZES for nb in BONES]


@pytest.mark.parametrize("n_vert,n_bones,seed", hostile_cases(), ids=[f"{n}v{b}b" for n, b, _ in hostile_cases()])
def test_equals_numpy_on_hostile_rigs(n_vert, n_bones, seed):
    rest, bones, weights, mats = sm.hostile_rig(n_vert, n_bones, seed)
    got = host.skin_vertices(rest, bones, weights, mats)
    ref = sm.skin(rest, bones, weights, mats)
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{int(bad.any(1).sum())} vertices differ; first {np.argwhere(bad)[0].tolist()}: {got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}"
    nan = np.isnan(got[:, [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14]])
    assert (_bits(got[:, [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14]])[nan] == 0x7FC00000).all()  # a stored NaN is canonical
    assert (_bits(got[:, 6:9]) == _bits(rest[:, 6:9])).all()  # uv: the words, whatever they are


def test_the_hostile_rigs_are_hostile():
    """What the cases above claim to cover is in them: both arms of l > 0, NaN and Inf results, denormal inputs, a payload NaN in uv."""
    rest, bones, weights, mats = sm.hostile_rig(1000, 5, 7)
    out = sm.skin(rest, bones, weights, mats)
    tiny = lambda a: (np.abs(a) < np.float32(2.0 ** -126)) & (a != 0)
    assert tiny(rest[:, 0:6]).any() and tiny(weights).any() and np.isnan(rest[:, 0:3]).any() and np.isinf(rest[:, 0:3]).any()
    assert (weights < 0).any() and (weights == 0).all(1).any() and (np.abs(weights.sum(1) - 1) > 0.5).any() and (bones == bones[:, :1]).all(1).any()
    unit = np.abs(np.linalg.norm(out[:, 3:6].astype(np.float64), axis=1) - 1) < 1e-5
    assert unit.any() and (out[:, 3:6] == 0).all(1).any() and np.isnan(out[:, 0:3]).any()
    assert not tiny(out[:, [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14]]).any()  # no operation hands a denormal out
    assert (_bits(rest[:, 6]) == 0x7FA00001).any()
    assert (mats.reshape(-1, 3, 4)[:, :, :3] == 0).all((1, 2)).any() and (np.abs(mats) > 1e19).any()


def _ordinary(n, n_bones, seed):
    """Finite, normal-range, non-zero rest vertices with unit normals, and well-conditioned matrices."""
    rng = np.random.default_rng(seed)
    rest = (rng.standard_normal((n, 15)) + np.where(rng.random((n, 15)) < 0.5, -3.0, 3.0)).astype(np.float32)
    rest[:, 3:6] = (rest[:, 3:6] / np.linalg.norm(rest[:, 3:6].astype(np.float64), axis=1, keepdims=True)).astype(np.float32)
    mats = rng.standard_normal((n_bones, 12)).astype(np.float32)
    return rest, mats


def test_one_bone_rig_blends_to_the_matrix_itself():
    """w = {1, 0, 0, 0}: B == M_b0 up to the sign of a zero, whatever the other three bones are -- seen through pos' against a direct M p in the stated order."""
    n, nb = 257, 5
    rest, mats = _ordinary(n, nb, 11)
    rng = np.random.default_rng(12)
    bones = rng.integers(0, nb, (n, 4)).astype(np.int32)
    weights = np.zeros((n, 4), np.float32)
    weights[:, 0] = 1.0
    got = host.skin_vertices(rest, bones, weights, mats)
    M = mats.reshape(nb, 3, 4)[bones[:, 0]]
    p = rest[:, 0:3]
    for i in range(3):
        direct = sm._op(np.add, sm.dot(M[:, i, 0], M[:, i, 1], M[:, i, 2], p[:, 0], p[:, 1], p[:, 2]), M[:, i, 3])
        assert (_bits(got[:, i]) == _bits(direct)).all(), i
    b2, w2 = rig.rigid(bones[:, 0])
    assert (b2[:, 0] == bones[:, 0]).all() and not b2[:, 1:].any() and (w2 == weights).all() and b2.dtype == np.int32 and w2.dtype == np.float32
    assert (_bits(host.skin_vertices(rest, b2, w2, mats)) == _bits(got)).all()


def _ulps(a, b):
    ia, ib = _bits(a).astype(np.int64), _bits(b).astype(np.int64)
    ia, ib = np.where(ia < 2 ** 31, ia, 2 ** 31 - ia), np.where(ib < 2 ** 31, ib, 2 ** 31 - ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("n_bones", [1, 4])
def test_identity_pose_returns_the_rest_pose(n_bones):
    """Positions, tangents, binormals and uv as bits (normal-range, non-zero inputs: a zero may change sign, a denormal is a zero); normals within 1 ulp of the
    input renormalised in float64.  Blended identity matrices with convex weights that sum to one exactly are the identity as well."""
    n = 1000
    rest, _ = _ordinary(n, n_bones, 21)
    rng = np.random.default_rng(22)
    bones = rng.integers(0, n_bones, (n, 4)).astype(np.int32)
    weights = np.tile(np.array([0.5, 0.25, 0.125, 0.125], np.float32), (n, 1))
    weights[::2] = [1, 0, 0, 0]
    got = host.skin_vertices(rest, bones, weights, rig.identity_pose(n_bones))
    for lo, hi in ((0, 3), (6, 9), (9, 12), (12, 15)):
        assert (_bits(got[:, lo:hi]) == _bits(rest[:, lo:hi])).all(), lo
    nrm = rest[:, 3:6].astype(np.float64)
    want = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(np.float32)
    assert _ulps(got[:, 3:6], want).max() <= 1


def _headline():
    scene, _ = scenes.config_headline(64, 48, subdiv=1)
    vert = np.ascontiguousarray(scene["vert"], np.float32).reshape(-1, 15)
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    return scene, vert, tri


def _about(centre, lin):
    """x -> lin (x - centre) + centre as a 3x4 matrix, built in float64 and cast."""
    lin = np.asarray(lin, np.float64)
    return np.concatenate([lin, (centre - lin @ centre)[:, None]], 1).astype(np.float32).reshape(12)


@pytest.mark.parametrize("what", ["rotation", "reflection"])
def test_rigid_pose_keeps_normals_on_their_faces(what):
    """The headline at subdiv 1, the sphere of material 5 turned by 10 degrees about its centre (or mirrored through it): each posed triangle's face normal
    (a float64 cross product of the posed positions) has a positive dot with the posed normals of its three vertices -- as in the rest pose."""
    scene, vert, tri = _headline()
    idx = vertices_of_material(scene, 5)
    obj = np.zeros(vert.shape[0], np.int32)
    obj[idx] = 1
    centre = vert[idx, 0:3].astype(np.float64).mean(0)
    th = np.deg2rad(10.0)
    c, s = np.cos(th), np.sin(th)
    lin = [[c, 0, s], [0, 1, 0], [-s, 0, c]] if what == "rotation" else np.diag([-1.0, 1.0, 1.0])
    pose = np.stack([rig.IDENTITY, _about(centre, lin)])
    bones, weights = rig.rigid(obj)
    out = host.skin_vertices(vert, bones, weights, pose)
    assert (_bits(out) == _bits(sm.skin(vert, bones, weights, pose))).all()
    others = np.setdiff1d(np.arange(vert.shape[0]), idx)
    assert (_bits(out[others][:, [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14]]) == _bits(vert[others][:, [0, 1, 2, 6, 7, 8, 9, 10, 11, 12, 13, 14]])).all()
    assert np.abs(out[idx, 0:3] - vert[idx, 0:3]).max() > 1e-3  # it moved

    def face_dots(v):
        own = tri[tri[:, 3].astype(np.int64) == 5][:, :3].astype(np.int64)
        p = v[:, 0:3].astype(np.float64)
        face = np.cross(p[own[:, 1]] - p[own[:, 0]], p[own[:, 2]] - p[own[:, 0]])
        return np.einsum("tk,tjk->tj", face, v[own][:, :, 3:6].astype(np.float64))

    assert (face_dots(vert) > 0).all()  # the rest pose: outward normals, counter-clockwise faces
    # A reflection reverses the winding (the cross product of the posed edges points inward) and the cofactor matrix, det L^-T, turns the normals with it: the
    # dot with the triangle's own cross product stays positive, which is what the renderer's two-sided shading sees.
    assert (face_dots(out) > 0).all()


def test_refusals():
    rest, bones, weights, mats = sm.hostile_rig(10, 3, 1)
    with pytest.raises(RuntimeError):
        host.skin_vertices(rest, np.where(bones == 2, 3, bones), weights, mats)  # a bone index of n_bones
    with pytest.raises(RuntimeError):
        host.skin_vertices(rest, np.where(bones == 0, -1, bones), weights, mats)
    L = host.lib()
    fp = lambda a: a.ctypes.data_as(__import__("ctypes").POINTER(__import__("ctypes").c_float))
    out = np.zeros_like(rest)
    assert L.glrt_skin_vertices(fp(rest), 10, None, fp(weights), fp(mats), 3, fp(out)) == -1
    assert L.glrt_skin_vertices(fp(rest), 10, bones.ctypes.data_as(L.glrt_skin_vertices.argtypes[2]), fp(weights), fp(mats), 0, fp(out)) == -1
    assert L.glrt_skin_vertices(fp(rest), 10, bones.ctypes.data_as(L.glrt_skin_vertices.argtypes[2]), fp(weights), fp(mats), 65537, fp(out)) == -1
    assert L.glrt_skin_vertices(fp(rest), 10, bones.ctypes.data_as(L.glrt_skin_vertices.argtypes[2]), fp(weights), None, 3, fp(out)) == -1
