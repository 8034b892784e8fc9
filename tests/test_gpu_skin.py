"""Posing on the device (csrc/skin.hip.h; glrtx_upload_rig, glrtx_pose, glrtx_debug_skin): the kernel equals the CPU statement bit for bit on the hostile rigs;
upload_rig + pose leave every device scene buffer byte for byte what update_vertices of the CPU-skinned vertices leaves, on a tree and on a chain, for rigid and
for blended rigs, and frames rendered afterwards are the oracle's; the rest pose survives a pose; the motion-aware reprojection sees a pose exactly as it sees
an update; refusals change nothing."""
import numpy as np
import pytest

import skin_math as sm
from glrt_amd import device, host, rig, scenes
from test_reproject_motion_host import moved_scene
from test_skin_host import BONES, SIZES, _about

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture()
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


@pytest.fixture()
def other(gpu_device):
    d = device.Device()
    yield d
    d.close()


# ---- 1. the kernel alone
@pytest.mark.parametrize("n_vert", SIZES)
def test_kernel_equals_the_cpu_statement_on_hostile_rigs(gpu_device, n_vert):
    """1 vertex is a partial wave; 63 / 64 / 65 cross a wave; 255 / 257 cross a workgroup."""
    for n_bones in BONES:
        rest, bones, weights, mats = sm.hostile_rig(n_vert, n_bones, 1000 * n_vert + n_bones)
        got = device.debug_skin(rest, bones, weights, mats)
        ref = host.skin_vertices(rest, bones, weights, mats)
        bad = _bits(got) != _bits(ref)
        assert not bad.any(), (f"{n_vert} vertices, {n_bones} bones: {int(bad.any(1).sum())} vertices differ; first {np.argwhere(bad)[0].tolist()}: "
                               f"{got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}")


# ---- 2. the scene after a pose
def _verts(scene):
    return np.ascontiguousarray(np.asarray(scene["vert"], np.float32).reshape(-1, 15))


def _by_material(scene):
    """Bone = material: every vertex follows the material of the triangles that use it (asserted: one material a vertex)."""
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    obj = np.full(_verts(scene).shape[0], -1, np.int64)
    for k in range(3):
        idx, m = tri[:, k].astype(np.int64), tri[:, 3].astype(np.int64)
        assert ((obj[idx] == -1) | (obj[idx] == m)).all()
        obj[idx] = m
    assert (obj >= 0).all()
    return obj.astype(np.int32), int(np.asarray(scene["mat"]).size // 18)


def _turn(deg, axis, centre, shift=(0.0, 0.0, 0.0), mirror=False):
    th = np.deg2rad(deg)
    c, s = np.cos(th), np.sin(th)
    R = {"x": [[1, 0, 0], [0, c, -s], [0, s, c]], "y": [[c, 0, s], [0, 1, 0], [-s, 0, c]], "z": [[c, -s, 0], [s, c, 0], [0, 0, 1]]}[axis]
    R = np.asarray(R, np.float64) @ (np.diag([-1.0, 1.0, 1.0]) if mirror else np.eye(3))
    m = _about(np.asarray(centre, np.float64), R).reshape(3, 4)
    m[:, 3] += np.asarray(shift, np.float32)
    return m.reshape(12)


def _pose_of(n_bones, seed, centre):
    """A pose that moves every bone a little, differently: small turns and shifts, one of them a mirror image."""
    rng = np.random.default_rng(seed)
    return np.stack([_turn(rng.uniform(-12, 12), "xyz"[b % 3], centre, rng.normal(0, 0.05, 3), mirror=(b == 2)) for b in range(n_bones)])


def _scene_bytes(d):
    return {w: d.read_scene(w) for w in device.SCENE_BUFFERS}


def _assert_same_scene(a, b, what):
    for w in device.SCENE_BUFFERS:
        assert a[w].size == b[w].size, (what, w, a[w].size, b[w].size)
        bad = np.flatnonzero(a[w] != b[w])
        assert bad.size == 0, f"{what}: {w} differs in {bad.size} bytes, first at byte {bad[0] if bad.size else -1}"


def _setup(d, scene, params):
    d.set_variant(2)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear()


def _two_frames(d, params):
    d.clear()
    for f in range(2):
        d.render(dict(params, seed=host.frame_seed(f)))
    return d.read_accum()


def _oracle_two_frames(scene, params):
    from oracle import pt_oracle
    acc = None
    for f in range(2):
        acc, _ = pt_oracle.render(scene, dict(params, seed=host.frame_seed(f)), accum=acc)
    return acc


def _c1():
    return scenes.config_c1(64, 48, max_depth=4, subdiv=1)


def _chain():
    return scenes.config_c3(64, 48, n=200)


def _rigid_case(make):
    scene, params = make()
    obj, n_bones = _by_material(scene)
    bones, weights = rig.rigid(obj)
    return scene, params, bones, weights, n_bones, _pose_of(n_bones, 3, (0.0, 1.0, 0.0))


def _blended_case():
    """The red icosphere of config 1 between two bones: half of its vertices hang on both with {0.5, 0.5}."""
    scene, params = _c1()
    obj, n_bones = _by_material(scene)
    bones, weights = rig.rigid(obj)
    red = np.flatnonzero(obj == 1)
    half = red[::2]
    bones[half, 1] = 2
    weights[half] = [0.5, 0.5, 0.0, 0.0]
    return scene, params, bones, weights, n_bones, _pose_of(n_bones, 4, (-2.2, 1.0, 0.0))


CASES = [("c1-rigid", lambda: _rigid_case(_c1)), ("chain-rigid", lambda: _rigid_case(_chain)), ("c1-blended", _blended_case)]


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_pose_leaves_what_an_update_of_the_skinned_vertices_leaves(dev, other, name, make):
    scene, params, bones, weights, n_bones, pose = make()
    rest = _verts(scene)
    skinned = host.skin_vertices(rest, bones, weights, pose)
    assert np.abs(skinned[:, 0:3] - rest[:, 0:3]).max() > 1e-2
    _setup(dev, scene, params); _setup(other, scene, params)
    dev.upload_rig(rest, bones, weights, n_bones)
    dev.pose(pose)
    other.update_vertices(skinned)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name)
    ref = _oracle_two_frames(moved_scene(scene, skinned), params)
    got = _two_frames(dev, params)
    assert (_bits(got) == _bits(ref)).all(), f"{name}: {int((_bits(got) != _bits(ref)).any(-1).sum())} pixels differ from the oracle"
    # pose twice, P then the identity: the rest pose was not overwritten (normals come back renormalised, so not the uploaded bytes)
    dev.pose(rig.identity_pose(n_bones))
    other.update_vertices(host.skin_vertices(rest, bones, weights, rig.identity_pose(n_bones)))
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (identity after P)")
    # and update_vertices keeps the rig: the rest pose is the rig's own copy
    dev.update_vertices(rest)
    dev.pose(pose)
    other.update_vertices(skinned)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (P after an update)")


def test_reprojection_sees_a_pose_as_it_sees_an_update(dev, other):
    """track_motion, 4 frames, render_features, pose, reproject_motion: the accumulator and the counts of the same sequence with update_vertices(skinned)."""
    scene, params, bones, weights, n_bones, pose = _rigid_case(_c1)
    rest = _verts(scene)
    skinned = host.skin_vertices(rest, bones, weights, pose)
    out = []
    for d, move in ((dev, lambda: dev.pose(pose)), (other, lambda: other.update_vertices(skinned))):
        _setup(d, scene, params)
        d.track_motion(True)
        if d is dev:
            d.upload_rig(rest, bones, weights, n_bones)
        for f in range(4):
            d.render(dict(params, seed=host.frame_seed(f)))
        d.render_features(params)
        move()
        d.reproject_motion(params)
        out.append((d.read_accum(), d.reproject_last(), d.read_features_geom()))
    assert (_bits(out[0][0]) == _bits(out[1][0])).all()
    assert out[0][1] == out[1][1] and 0 < out[0][1][0] <= out[0][1][1]
    assert (_bits(out[0][2]) == _bits(out[1][2])).all()


def test_refusals(dev):
    scene, params, bones, weights, n_bones, pose = _rigid_case(_c1)
    rest = _verts(scene)

    def refused(fn, *args):
        with pytest.raises(device.GlrtxError) as e:
            fn(*args)
        assert e.value.code == -1, e.value

    refused(dev.upload_rig, rest, bones, weights, n_bones)  # no scene
    refused(dev.pose, pose)
    _setup(dev, scene, params)
    before = _scene_bytes(dev)
    refused(dev.pose, pose)  # pose before rig
    refused(dev.upload_rig, rest[:-1], bones[:-1], weights[:-1], n_bones)  # not the scene's vertex count
    refused(dev.upload_rig, rest, bones, weights, 0)
    refused(dev.upload_rig, rest, bones, weights, 65537)
    bad = bones.copy(); bad[5, 3] = n_bones
    refused(dev.upload_rig, rest, bad, weights, n_bones)  # a bone index of n_bones
    bad = bones.copy(); bad[7, 0] = -1
    refused(dev.upload_rig, rest, bad, weights, n_bones)
    for v in (np.nan, np.inf):
        bad = weights.copy(); bad[3, 2] = v
        refused(dev.upload_rig, rest, bones, bad, n_bones)
    refused(dev.pose, pose)  # none of them left a rig behind
    dev.upload_rig(rest, bones, weights, n_bones)
    refused(dev.pose, pose[:-1])  # wrong bone count
    refused(dev.pose, np.concatenate([pose, pose[:1]]))
    for v in (np.nan, -np.inf):
        bad = pose.copy(); bad[n_bones - 1, 11] = v
        refused(dev.pose, bad)
    _assert_same_scene(_scene_bytes(dev), before, "after the refusals")
    refused(dev.skin_burst_ms, 2)  # (the timing hook: nothing posed yet)
    dev.pose(pose)  # with everything in place it goes through
    posed = _scene_bytes(dev)
    assert dev.skin_burst_ms(2) > 0.0
    refused(dev.skin_burst_ms, 0)
    _assert_same_scene(_scene_bytes(dev), posed, "after the timing hook")  # (it writes the vertex staging buffer only)
    assert any((_scene_bytes(dev)[w] != before[w]).any() for w in ("nodes", "nrms"))
    dev.upload_scene(scene)  # the rig is forgotten after upload_scene
    refused(dev.pose, pose)
    _assert_same_scene(_scene_bytes(dev), before, "after upload_scene")
    L = dev.L
    assert L.glrtx_pose(None, None, 1) == -1 and L.glrtx_upload_rig(None, None, 0, None, None, 1) == -1
    assert L.glrtx_pose(dev.h, None, n_bones) == -1
