"""Rebuilding normals on the device (csrc/normals.hip.h; glrtx_upload_normal_topology, glrtx_update_positions / _device, glrtx_set_pose_normals,
glrtx_debug_rebuild_normals): the passes equal the CPU statement bit for bit on every case of tests/normals_cases.py; a position-only update, from numpy and
from a torch tensor, leaves every device scene buffer byte for byte what update_vertices of the CPU statement's vertices leaves, and a frame rendered afterwards
is the oracle's; with the pose switch on every pose call equals update-of-(deform, then rebuild), with it off nothing changes; the motion-aware reprojection
sees a position update as it sees a vertex update; refusals change nothing; upload_scene forgets the topology and the switch."""
import numpy as np
import pytest

import normals_cases as nc
from glrt_amd import device, host, rig, scenes
from test_gpu_deform import _gentle_pose, _targets
from test_gpu_deform_sparse import _sparse_targets
from test_gpu_skin import _assert_same_scene, _by_material, _pose_of, _rigid_case, _scene_bytes, _setup, _verts
from test_reproject_motion_host import lifted, moved_scene

pytestmark = pytest.mark.gpu

CASES = nc.cases()


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


def _refused(fn, *args, message=None):
    with pytest.raises(device.GlrtxError) as e:
        fn(*args)
    assert e.value.code == -1, e.value
    if message:
        assert message in str(e.value), e.value


# ---- 1. the passes alone
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_passes_equal_the_cpu_statement(gpu_device, case):
    name, rest, tri, moved, class_map = case
    cls, flip, _ = host.normal_topology(rest, tri)
    if class_map is not None:
        cls = class_map
    got = device.debug_rebuild_normals(moved, tri, cls, flip)
    ref = host.rebuild_normals(moved, tri, cls, flip)
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (f"{name}: {int(bad.any(1).sum())} vertices differ; first {np.argwhere(bad)[0].tolist()}: "
                           f"{got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}")


# ---- 2. position-only updates
def _headline():
    return scenes.config_headline(48, 27)


def _c1():
    """test_gpu_skin's config 1 at this file's image size."""
    return scenes.config_c1(48, 27, max_depth=4, subdiv=1)


def _blended_case():
    """test_gpu_skin's blended rig on that scene: half of the red icosphere's vertices hang on two bones with {0.5, 0.5}."""
    scene, params = _c1()
    obj, n_bones = _by_material(scene)
    bones, weights = rig.rigid(obj)
    half = np.flatnonzero(obj == 1)[::2]
    bones[half, 1] = 2
    weights[half] = [0.5, 0.5, 0.0, 0.0]
    return scene, params, bones, weights, n_bones, _pose_of(n_bones, 4, (-2.2, 1.0, 0.0))


def _sphere_lifted(scene):
    return lifted(scene, 1, 0.4)[:, 0:3].copy()


def _ellipsoid_morph(scene):
    """Every sphere of the headline stretched to twice its height about its own centre: p + 1 * dpos with dpos = (0, y - centre.y, 0)."""
    v = _verts(scene)
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    pos = v[:, 0:3].copy()
    for m in np.unique(tri[:, 3]).astype(np.int64):
        idx = np.unique(tri[tri[:, 3] == m, 0:3].astype(np.int64))
        if idx.size > 100:  # a sphere (the walls and the lamp are quads)
            cy = np.float32(0.5) * (v[idx, 1].min() + v[idx, 1].max())
            pos[idx, 1] = v[idx, 1] + (v[idx, 1] - cy)
    return pos


MOVES = [("sphere lifted", _sphere_lifted), ("ellipsoid morph", _ellipsoid_morph)]


@pytest.mark.parametrize("name,move", MOVES, ids=[m[0] for m in MOVES])
def test_update_positions_leaves_what_an_update_of_the_statements_vertices_leaves(dev, other, name, move):
    import torch
    from oracle import pt_oracle
    scene, params = _headline()
    rest, tri = _verts(scene), scene["tri"]
    assert rest.shape[0] == 30756
    pos = move(scene)
    assert np.abs(pos - rest[:, 0:3]).max() > 0.1
    cls, flip, n_classes = host.normal_topology(rest, tri)
    V = host.rebuild_normals(host.positions_to_vertices(rest, pos), tri, cls, flip)
    assert n_classes == 5160 and (_bits(V[:, 3:6]) != _bits(rest[:, 3:6])).any()
    _setup(dev, scene, params); _setup(other, scene, params)
    other.update_vertices(V)
    want = _scene_bytes(other)
    dev.upload_normal_topology(rest, tri)
    dev.update_positions(pos)
    _assert_same_scene(_scene_bytes(dev), want, name + " (numpy)")
    dev.clear()
    dev.render(dict(params, seed=host.frame_seed(0)))
    ref, _ = pt_oracle.render(moved_scene(scene, V), dict(params, seed=host.frame_seed(0)))
    got = dev.read_accum()
    assert (_bits(got) == _bits(ref)).all(), f"{name}: {int((_bits(got) != _bits(ref)).any(-1).sum())} pixels differ from the oracle"
    # back to the rest positions, then the same move from a tensor on the context's GPU
    dev.update_positions(rest[:, 0:3].copy())
    other.update_vertices(host.rebuild_normals(rest, tri, cls, flip))
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (rest positions)")
    t = torch.from_numpy(pos).cuda().contiguous()
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        dev.update_positions(t.double())
    with pytest.raises(ValueError):
        dev.update_positions(t[:, 0:2])
    dev.update_positions(t)
    _assert_same_scene(_scene_bytes(dev), want, name + " (torch)")
    dev.update_positions(t.reshape(-1))
    _assert_same_scene(_scene_bytes(dev), want, name + " (torch, flat)")
    assert dev.normals_burst_ms(2) > 0.0  # the timing hook rebuilds what is there already
    dev.update_vertices(rest)  # update_vertices keeps the topology
    dev.update_positions(pos)
    _assert_same_scene(_scene_bytes(dev), want, name + " (after an update_vertices)")


def test_weld_by_position_through_the_context(dev, other):
    scene, params = _c1()
    rest, tri = _verts(scene), scene["tri"]
    pos = nc.wobble(rest, 21, 0.1)[:, 0:3].copy()
    _setup(dev, scene, params); _setup(other, scene, params)
    for flags in (host.NORMALS_WELD_POSITIONS, 0):  # (the second upload replaces the first topology)
        cls, flip, _ = host.normal_topology(rest, tri, flags)
        dev.upload_normal_topology(rest, tri, flags)
        dev.update_positions(pos)
        other.update_vertices(host.rebuild_normals(host.positions_to_vertices(rest, pos), tri, cls, flip))
        _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), f"flags {flags}")


# ---- 3. the pose switch
def _pose_cases():
    """(name, scene, params, bones, weights, n_bones, upload the targets, pose, the CPU statement's vertices) for every pose call."""
    scene, params, bones, weights, n_bones, pose = _rigid_case(_c1)
    rest = _verts(scene)
    dense, mw = _targets(rest, 8)
    so, sv, sd, smw = _sparse_targets(rest, 8)
    bscene, bparams, bbones, bweights, bn, _ = _blended_case()
    brest = _verts(bscene)
    dq = rig.dualquat(_gentle_pose(bn, 4, (-2.2, 1.0, 0.0)))
    bo, bv, bd, bmw = _sparse_targets(brest, 9)
    rigid, blended = (scene, params, bones, weights, n_bones), (bscene, bparams, bbones, bweights, bn)
    return [
        ("pose",) + rigid + (lambda dv: None, lambda dv: dv.pose(pose), host.skin_vertices(rest, bones, weights, pose)),
        ("pose_morph dense",) + rigid + (lambda dv: dv.upload_morph_targets(dense), lambda dv: dv.pose_morph(pose, mw),
                                         host.deform_vertices(rest, bones, weights, pose, 0, dense, mw)),
        ("pose_morph sparse",) + rigid + (lambda dv: dv.upload_morph_targets_sparse(so, sv, sd), lambda dv: dv.pose_morph(pose, smw),
                                          host.deform_vertices_sparse(rest, bones, weights, pose, 0, so, sv, sd, smw)),
        ("pose_dualquat",) + blended + (lambda dv: None, lambda dv: dv.pose_dualquat(dq), host.deform_vertices(brest, bbones, bweights, dq, 1)),
        ("pose_dualquat sparse",) + blended + (lambda dv: dv.upload_morph_targets_sparse(bo, bv, bd), lambda dv: dv.pose_dualquat(dq, bmw),
                                               host.deform_vertices_sparse(brest, bbones, bweights, dq, 1, bo, bv, bd, bmw)),
    ]


def test_pose_switch(dev, other):
    """On: every pose call equals update_vertices(rebuild(deform)).  Off: byte for byte what the call leaves today, with and without a topology uploaded."""
    for name, scene, params, bones, weights, n_bones, targets, pose, deformed in _pose_cases():
        rest, tri = _verts(scene), scene["tri"]
        cls, flip, _ = host.normal_topology(rest, tri)
        rebuilt = host.rebuild_normals(deformed, tri, cls, flip)
        assert (_bits(rebuilt[:, 3:6]) != _bits(deformed[:, 3:6])).any() and (_bits(rebuilt[:, 0:3]) == _bits(deformed[:, 0:3])).all()
        _setup(dev, scene, params); _setup(other, scene, params)
        dev.upload_rig(rest, bones, weights, n_bones)
        targets(dev)
        other.update_vertices(deformed)
        today = _scene_bytes(other)
        pose(dev)
        _assert_same_scene(_scene_bytes(dev), today, name + " (no topology)")
        _refused(dev.set_pose_normals, True, message="no normal topology")
        dev.upload_normal_topology(rest, tri)
        pose(dev)
        _assert_same_scene(_scene_bytes(dev), today, name + " (topology, switch off)")
        dev.set_pose_normals(True)
        pose(dev)
        other.update_vertices(rebuilt)
        _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (switch on)")
        dev.upload_rig(rest, bones, weights, n_bones)  # upload_rig and the morph uploads keep the topology and the switch
        targets(dev)
        pose(dev)
        _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (switch on, after upload_rig)")
        dev.set_pose_normals(False)
        pose(dev)
        _assert_same_scene(_scene_bytes(dev), today, name + " (switch off again)")


# ---- 4. reprojection
def test_reprojection_sees_a_position_update_as_it_sees_a_vertex_update(dev, other):
    scene, params = _c1()
    rest, tri = _verts(scene), scene["tri"]
    pos = _sphere_lifted(scene)
    cls, flip, _ = host.normal_topology(rest, tri)
    V = host.rebuild_normals(host.positions_to_vertices(rest, pos), tri, cls, flip)
    out = []
    for d, move in ((dev, lambda: dev.update_positions(pos)), (other, lambda: other.update_vertices(V))):
        _setup(d, scene, params)
        d.track_motion(True)
        if d is dev:
            d.upload_normal_topology(rest, tri)
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
def test_refusals_and_what_upload_scene_forgets(dev):
    scene, params = _c1()
    rest, tri = _verts(scene), np.ascontiguousarray(np.asarray(scene["tri"], np.float32).reshape(-1, 4))
    n = rest.shape[0]
    pos = _sphere_lifted(scene)
    _refused(dev.upload_normal_topology, rest, tri, message="no scene")
    _refused(dev.update_positions, pos, message="no scene")
    _refused(dev.set_pose_normals, True)
    _setup(dev, scene, params)
    before = _scene_bytes(dev)
    _refused(dev.update_positions, pos, message="no normal topology")
    _refused(dev.normals_burst_ms, 2)
    _refused(dev.upload_normal_topology, rest[:-1], tri, message=f"{n - 1} vertices")
    _refused(dev.upload_normal_topology, rest, tri, 2, message="unknown flag")
    for bad in (float(n), -1.0, 0.5, np.nan):
        t = tri.copy(); t[7, 1] = bad
        _refused(dev.upload_normal_topology, rest, t, message="triangle 7, corner 1")
    L, fp = dev.L, lambda a: a.ctypes.data_as(device.C.POINTER(device.C.c_float))
    assert L.glrtx_upload_normal_topology(dev.h, None, n, fp(tri), tri.shape[0], 0) == -1
    assert L.glrtx_upload_normal_topology(dev.h, fp(rest), n, None, tri.shape[0], 0) == -1
    assert L.glrtx_upload_normal_topology(dev.h, fp(rest), n, fp(tri), 2 ** 31, 0) == -1
    _refused(dev.update_positions, pos, message="no normal topology")  # none of them left a topology behind
    _refused(dev.set_pose_normals, True)
    dev.upload_normal_topology(rest, tri)
    _refused(dev.update_positions, pos[:-1], message=f"{n - 1} vertices")
    assert L.glrtx_update_positions(dev.h, None, n) == -1 and L.glrtx_update_positions_device(dev.h, None, n) == -1
    t = tri.copy(); t[0, 0] = n
    _refused(dev.upload_normal_topology, rest, t)  # a refused upload keeps the topology that is there
    _assert_same_scene(_scene_bytes(dev), before, "after the refusals")
    dev.set_pose_normals(True)
    dev.update_positions(pos)  # with everything in place it goes through
    assert any((_scene_bytes(dev)[w] != before[w]).any() for w in ("nodes", "nrms"))
    assert dev.normals_burst_ms(2) > 0.0
    _refused(dev.normals_burst_ms, 0)
    dev.upload_scene(scene)  # the topology and the switch are forgotten
    _refused(dev.update_positions, pos, message="no normal topology")
    _refused(dev.set_pose_normals, True)
    dev.set_pose_normals(False)
    _assert_same_scene(_scene_bytes(dev), before, "after upload_scene")
    dev.upload_normal_topology(rest, tri)  # the switch did not survive: a pose is today's pose
    bones, weights = rig.rigid(np.zeros(n, np.int32))
    dev.upload_rig(rest, bones, weights, 1)
    dev.pose(rig.identity_pose(1))
    plain = _scene_bytes(dev)
    dev.update_vertices(host.skin_vertices(rest, bones, weights, rig.identity_pose(1)))
    _assert_same_scene(_scene_bytes(dev), plain, "the switch is off after upload_scene")
