"""Deforming on the device (csrc/skin.hip.h: deform_kernel; glrtx_upload_morph_targets, glrtx_pose_morph, glrtx_pose_dualquat, glrtx_debug_deform): the kernel
equals the CPU statement bit for bit on the hostile grid; a pose with morph weights or with dual quaternions leaves every device scene buffer byte for byte what
update_vertices of the CPU-deformed vertices leaves, on a tree and on a chain, and frames rendered afterwards are the oracle's; the rest pose and the targets
survive a pose and an update; all-zero weights are glrtx_pose; the motion-aware reprojection sees a deform as it sees an update; refusals change nothing."""
import numpy as np
import pytest

import deform_math as dm
from glrt_amd import device, host, rig
from test_gpu_skin import (_assert_same_scene, _blended_case, _c1, _chain, _oracle_two_frames, _rigid_case, _scene_bytes, _setup, _turn, _two_frames,
                           _verts)
from test_reproject_motion_host import moved_scene
from test_skin_host import BONES, SIZES

pytestmark = pytest.mark.gpu

TARGETS = [0, 1, 3, 64]


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
@pytest.mark.parametrize("mode", [0, 1], ids=["mat", "dq"])
@pytest.mark.parametrize("n_vert", SIZES)
def test_kernel_equals_the_cpu_statement_on_hostile_cases(gpu_device, n_vert, mode):
    """1 vertex is a partial wave; 63 / 64 / 65 cross a wave; 255 / 257 cross a workgroup; 64 targets is the full active list (less the inactive ones: the list is
    compacted)."""
    for n_bones in BONES:
        for n_targets in TARGETS:
            rest, bones, weights, data, deltas, mw = dm.hostile_case(n_vert, n_bones, mode, n_targets, 1000 * n_vert + n_bones)
            got = device.debug_deform(rest, bones, weights, data, mode, deltas, mw)
            ref = host.deform_vertices(rest, bones, weights, data, mode, deltas, mw)
            bad = _bits(got) != _bits(ref)
            assert not bad.any(), (f"{n_vert} vertices, {n_bones} bones, {n_targets} targets: {int(bad.any(1).sum())} vertices differ; first "
                                   f"{np.argwhere(bad)[0].tolist()}: {got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}")


def test_all_64_targets_active(gpu_device):
    """The full list: 64 active targets, ordinary deltas."""
    rest, bones, weights, mats, _, _ = dm.hostile_case(257, 5, 0, 0, 3)
    rng = np.random.default_rng(4)
    deltas = (rng.standard_normal((64, 257, 6)) * 0.1).astype(np.float32)
    mw = rng.uniform(0.1, 1.0, 64).astype(np.float32)
    for mode, data in ((0, mats), (1, dm.hostile_dualquats(5, 3)[0])):
        got = device.debug_deform(rest, bones, weights, data, mode, deltas, mw)
        assert (_bits(got) == _bits(host.deform_vertices(rest, bones, weights, data, mode, deltas, mw))).all(), mode


# ---- 2. the scene after a pose
def _targets(rest, seed):
    """Three targets for a scene: small random position and normal deltas; the middle one is never active and holds NaN."""
    rng = np.random.default_rng(seed)
    d = (rng.standard_normal((3, rest.shape[0], 6)) * 0.03).astype(np.float32)
    d[1] = np.nan
    return d, np.array([0.7, 0.0, -0.4], np.float32)


def _gentle_pose(n_bones, seed, centre):
    """_pose_of without the mirror image: a dual quaternion states rotations only."""
    rng = np.random.default_rng(seed)
    return np.stack([_turn(rng.uniform(-12, 12), "xyz"[b % 3], centre, rng.normal(0, 0.05, 3)) for b in range(n_bones)])


def _morph_case(make):
    scene, params, bones, weights, n_bones, pose = _rigid_case(make)
    deltas, mw = _targets(_verts(scene), 8)
    return scene, params, bones, weights, n_bones, pose, 0, deltas, mw


def _dualquat_case(make_rig, centre):
    scene, params, bones, weights, n_bones, _ = make_rig()
    return scene, params, bones, weights, n_bones, rig.dualquat(_gentle_pose(n_bones, 4, centre)), 1, None, None


CASES = [("c1-morph", lambda: _morph_case(_c1)), ("chain-morph", lambda: _morph_case(_chain)),
         ("c1-dualquat", lambda: _dualquat_case(_blended_case, (-2.2, 1.0, 0.0))), ("chain-dualquat", lambda: _dualquat_case(lambda: _rigid_case(_chain), (0.0, 1.0, 0.0)))]


def _pose(d, mode, data, mw):
    (d.pose_dualquat if mode else d.pose_morph)(data, mw)


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_deform_leaves_what_an_update_of_the_deformed_vertices_leaves(dev, other, name, make):
    scene, params, bones, weights, n_bones, data, mode, deltas, mw = make()
    rest = _verts(scene)
    deformed = host.deform_vertices(rest, bones, weights, data, mode, deltas, mw)
    assert np.isfinite(deformed).all() and np.abs(deformed[:, 0:3] - rest[:, 0:3]).max() > 1e-2
    _setup(dev, scene, params); _setup(other, scene, params)
    dev.upload_rig(rest, bones, weights, n_bones)
    if deltas is not None:
        dev.upload_morph_targets(deltas)
    _pose(dev, mode, data, mw)
    other.update_vertices(deformed)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name)
    ref = _oracle_two_frames(moved_scene(scene, deformed), params)
    got = _two_frames(dev, params)
    assert (_bits(got) == _bits(ref)).all(), f"{name}: {int((_bits(got) != _bits(ref)).any(-1).sum())} pixels differ from the oracle"
    # all weights zero: the targets are not read, the rest pose was not overwritten
    zero = None if mw is None else np.zeros_like(mw)
    _pose(dev, mode, data, zero)
    other.update_vertices(host.deform_vertices(rest, bones, weights, data, mode))
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (zero weights)")
    # and update_vertices keeps the rig and the targets: both are the rig's own copies
    dev.update_vertices(rest)
    _pose(dev, mode, data, mw)
    other.update_vertices(deformed)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (after an update)")


def test_dualquats_with_morph_weights(dev, other):
    """Both at once on the blended rig: morph, then the dual-quaternion skinning stage."""
    scene, params, bones, weights, n_bones, data, mode, _, _ = _dualquat_case(_blended_case, (-2.2, 1.0, 0.0))
    rest = _verts(scene)
    deltas, mw = _targets(rest, 9)
    _setup(dev, scene, params); _setup(other, scene, params)
    dev.upload_rig(rest, bones, weights, n_bones)
    dev.upload_morph_targets(deltas)
    dev.pose_dualquat(data, mw)
    other.update_vertices(host.deform_vertices(rest, bones, weights, data, 1, deltas, mw))
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), "dualquat + morph")


# ---- 3. no active target is glrtx_pose
def test_zero_weights_are_a_pose(dev, other):
    scene, params, bones, weights, n_bones, pose, _, deltas, mw = _morph_case(_c1)
    rest = _verts(scene)
    _setup(dev, scene, params); _setup(other, scene, params)
    dev.upload_rig(rest, bones, weights, n_bones)
    dev.upload_morph_targets(deltas)
    dev.pose_morph(pose, np.zeros_like(mw))
    other.upload_rig(rest, bones, weights, n_bones)
    other.pose(pose)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), "zero weights against pose")
    dev.upload_morph_targets(None)  # dropped: a pose without weights goes through, one with weights does not
    dev.pose_morph(pose)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), "no targets against pose")
    with pytest.raises(device.GlrtxError):
        dev.pose_morph(pose, mw)


# ---- 4. reprojection
def test_reprojection_sees_a_deform_as_it_sees_an_update(dev, other):
    """track_motion, 4 frames, render_features, pose_morph, reproject_motion: the accumulator, the counts and the G plane of the same sequence with
    update_vertices(deformed)."""
    scene, params, bones, weights, n_bones, pose, _, deltas, mw = _morph_case(_c1)
    rest = _verts(scene)
    deformed = host.deform_vertices(rest, bones, weights, pose, 0, deltas, mw)
    out = []
    for d, move in ((dev, lambda: dev.pose_morph(pose, mw)), (other, lambda: other.update_vertices(deformed))):
        _setup(d, scene, params)
        d.track_motion(True)
        if d is dev:
            d.upload_rig(rest, bones, weights, n_bones)
            d.upload_morph_targets(deltas)
        for f in range(4):
            d.render(dict(params, seed=host.frame_seed(f)))
        d.render_features(params)
        move()
        d.reproject_motion(params)
        out.append((d.read_accum(), d.reproject_last(), d.read_features_geom()))
    assert (_bits(out[0][0]) == _bits(out[1][0])).all()
    assert out[0][1] == out[1][1] and 0 < out[0][1][0] <= out[0][1][1]
    assert (_bits(out[0][2]) == _bits(out[1][2])).all()


# ---- 5. refusals
def test_refusals(dev):
    scene, params, bones, weights, n_bones, pose, _, deltas, mw = _morph_case(_c1)
    rest = _verts(scene)
    dq = rig.dualquat(_gentle_pose(n_bones, 4, (0.0, 1.0, 0.0)))

    def refused(fn, *args):
        with pytest.raises(device.GlrtxError) as e:
            fn(*args)
        assert e.value.code == -1, e.value

    refused(dev.upload_morph_targets, deltas)  # no scene
    refused(dev.pose_morph, pose, None)
    refused(dev.pose_dualquat, dq, None)
    _setup(dev, scene, params)
    before = _scene_bytes(dev)
    refused(dev.upload_morph_targets, deltas)  # targets before the rig
    refused(dev.pose_morph, pose, None)  # no rig
    refused(dev.pose_dualquat, dq, None)
    dev.upload_rig(rest, bones, weights, n_bones)
    refused(dev.deform_burst_ms, 2)  # (the timing hook: nothing deformed yet)
    refused(dev.upload_morph_targets, deltas[:, :-1])  # not the rig's vertex count
    refused(dev.upload_morph_targets, np.zeros((65, rest.shape[0], 6), np.float32))
    assert dev.L.glrtx_upload_morph_targets(dev.h, None, 3, rest.shape[0]) == -1
    refused(dev.pose_morph, pose, mw)  # none of them left targets behind
    dev.upload_morph_targets(deltas)
    refused(dev.pose_morph, pose, None)  # wrong n_targets
    refused(dev.pose_morph, pose, mw[:-1])
    refused(dev.pose_dualquat, dq, np.concatenate([mw, mw[:1]]))
    refused(dev.pose_morph, pose[:-1], mw)  # wrong n_bones
    refused(dev.pose_dualquat, np.concatenate([dq, dq[:1]]), mw)
    assert dev.L.glrtx_pose_morph(dev.h, None, n_bones, mw.ctypes.data_as(dev.L.glrtx_pose_morph.argtypes[3]), 3) == -1
    assert dev.L.glrtx_pose_dualquat(dev.h, dq.ctypes.data_as(dev.L.glrtx_pose_dualquat.argtypes[1]), n_bones, None, 3) == -1
    for v in (np.nan, np.inf, -np.inf):
        bad = mw.copy(); bad[1] = v
        refused(dev.pose_morph, pose, bad)
        refused(dev.pose_dualquat, dq, bad)
        bad = pose.copy(); bad[n_bones - 1, 11] = v
        refused(dev.pose_morph, bad, mw)
        bad = dq.copy(); bad[0, 5] = v
        refused(dev.pose_dualquat, bad, mw)
    _assert_same_scene(_scene_bytes(dev), before, "after the refusals")
    refused(dev.deform_burst_ms, 2)  # still nothing deformed
    dev.pose_morph(pose, mw)  # with everything in place it goes through
    posed = _scene_bytes(dev)
    assert any((posed[w] != before[w]).any() for w in ("nodes", "nrms"))
    assert dev.deform_burst_ms(2) > 0.0
    refused(dev.deform_burst_ms, 0)
    dev.pose_dualquat(dq, mw)
    assert dev.deform_burst_ms(2) > 0.0
    dev.pose_morph(pose, mw)
    _assert_same_scene(_scene_bytes(dev), posed, "after the timing hook and a dual-quaternion pose in between")
    dev.upload_rig(rest, bones, weights, n_bones)  # after upload_rig the targets are gone
    refused(dev.pose_morph, pose, mw)
    refused(dev.deform_burst_ms, 2)
    dev.pose_morph(pose, None)
    dev.upload_morph_targets(deltas)
    dev.upload_scene(scene)  # after upload_scene both are gone
    refused(dev.pose_morph, pose, None)
    refused(dev.upload_morph_targets, deltas)
    _assert_same_scene(_scene_bytes(dev), before, "after upload_scene")
