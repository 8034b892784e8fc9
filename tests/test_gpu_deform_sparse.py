"""Sparse morph targets on the device (csrc/skin.hip.h: deform_sparse_kernel; glrtx_upload_morph_targets_sparse, glrtx_debug_deform_sparse, and glrtx_pose_morph /
glrtx_pose_dualquat on a rig that holds a sparse set): the kernel equals the CPU statement bit for bit on the hostile grid and every index pattern; a pose leaves
every device scene buffer byte for byte what update_vertices of the CPU-deformed vertices leaves, on a tree and on a chain, and frames rendered afterwards are
the oracle's; dense and sparse sets replace each other; the motion-aware reprojection sees a sparse pose as it sees an update; refusals change nothing."""
import numpy as np
import pytest

import deform_math as dm
import deform_sparse_math as ds
from glrt_amd import device, host, rig
from test_gpu_deform import _gentle_pose, _targets
from test_gpu_skin import (_assert_same_scene, _blended_case, _c1, _chain, _oracle_two_frames, _rigid_case, _scene_bytes, _setup, _two_frames, _verts)
from test_reproject_motion_host import moved_scene
from test_skin_host import BONES, SIZES

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
@pytest.mark.parametrize("mode", [0, 1], ids=["mat", "dq"])
@pytest.mark.parametrize("n_vert", SIZES)
def test_kernel_equals_the_cpu_statement_on_hostile_cases(gpu_device, n_vert, mode):
    """1 vertex is a partial wave; 63 / 64 / 65 cross a wave; 255 / 257 cross a workgroup and leave a last workgroup with one live lane behind the barrier; 1024
    targets is the full weight table; "one vertex listed by all targets" is the most divergent wave, one lane walking 1024 entries beside 63 empty rows."""
    for what, name, rest, bones, weights, data, o, v, d, w in ds.grid_cases(n_vert, mode, BONES):
        got = device.debug_deform_sparse(rest, bones, weights, data, mode, o, v, d, w)
        ref = host.deform_vertices_sparse(rest, bones, weights, data, mode, o, v, d, w)
        bad = _bits(got) != _bits(ref)
        assert not bad.any(), (f"{n_vert} vertices, {what}: {int(bad.any(1).sum())} vertices differ; first "
                               f"{np.argwhere(bad)[0].tolist()}: {got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}")


def test_all_1024_targets_active(gpu_device):
    """The full table, every weight active, ordinary deltas: each target a run of ten vertices, so rows hold tens of entries."""
    n = 257
    rest, bones, weights, mats = ds.hostile_rig(n, 5, 0, 3)
    rng = np.random.default_rng(4)
    dense = (rng.standard_normal((1024, n, 6)) * 0.01).astype(np.float32)
    first = rng.integers(0, n - 10, 1024)
    o, v, d = ds.from_mask(dense, (np.arange(n)[None, :] >= first[:, None]) & (np.arange(n)[None, :] < first[:, None] + 10))
    mw = rng.uniform(0.1, 1.0, 1024).astype(np.float32)
    for mode, data in ((0, mats), (1, dm.hostile_dualquats(5, 3)[0])):
        got = device.debug_deform_sparse(rest, bones, weights, data, mode, o, v, d, mw)
        assert (_bits(got) == _bits(host.deform_vertices_sparse(rest, bones, weights, data, mode, o, v, d, mw))).all(), mode


# ---- 2. the scene after a pose
def _sparse_targets(rest, seed):
    """test_gpu_deform's three targets made sparse: each lists a random half of the vertices; the middle one is never active and holds NaN."""
    dense, mw = _targets(rest, seed)
    mask = np.random.default_rng(seed + 1).random(dense.shape[0:2]) < 0.5
    return ds.from_mask(dense, mask) + (mw,)


def _morph_case(make):
    scene, params, bones, weights, n_bones, pose = _rigid_case(make)
    return (scene, params, bones, weights, n_bones, pose, 0) + _sparse_targets(_verts(scene), 8)


def _dualquat_case(make_rig, centre):
    scene, params, bones, weights, n_bones, _ = make_rig()
    return (scene, params, bones, weights, n_bones, rig.dualquat(_gentle_pose(n_bones, 4, centre)), 1) + _sparse_targets(_verts(scene), 9)


CASES = [("c1-mat", lambda: _morph_case(_c1)), ("chain-mat", lambda: _morph_case(_chain)),
         ("c1-dualquat", lambda: _dualquat_case(_blended_case, (-2.2, 1.0, 0.0))), ("chain-dualquat", lambda: _dualquat_case(lambda: _rigid_case(_chain), (0.0, 1.0, 0.0)))]


def _pose(d, mode, data, mw):
    (d.pose_dualquat if mode else d.pose_morph)(data, mw)


@pytest.mark.parametrize("name,make", CASES, ids=[c[0] for c in CASES])
def test_sparse_pose_leaves_what_an_update_of_the_deformed_vertices_leaves(dev, other, name, make):
    scene, params, bones, weights, n_bones, data, mode, o, v, d, mw = make()
    rest = _verts(scene)
    deformed = host.deform_vertices_sparse(rest, bones, weights, data, mode, o, v, d, mw)
    assert np.isfinite(deformed).all() and np.abs(deformed[:, 0:3] - rest[:, 0:3]).max() > 1e-2
    assert (_bits(deformed) != _bits(host.deform_vertices(rest, bones, weights, data, mode))).any()  # the targets do move something
    _setup(dev, scene, params); _setup(other, scene, params)
    dev.upload_rig(rest, bones, weights, n_bones)
    dev.upload_morph_targets_sparse(o, v, d)
    _pose(dev, mode, data, mw)
    other.update_vertices(deformed)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name)
    ref = _oracle_two_frames(moved_scene(scene, deformed), params)
    got = _two_frames(dev, params)
    assert (_bits(got) == _bits(ref)).all(), f"{name}: {int((_bits(got) != _bits(ref)).any(-1).sum())} pixels differ from the oracle"
    # all weights zero: what glrtx_pose leaves (matrices), or the deform without targets (dual quaternions)
    _pose(dev, mode, data, np.zeros_like(mw))
    if mode == 0:
        other.upload_rig(rest, bones, weights, n_bones)
        other.pose(data)
    else:
        other.update_vertices(host.deform_vertices(rest, bones, weights, data, mode))
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (zero weights)")
    # and update_vertices keeps the rig and the set
    dev.update_vertices(rest)
    _pose(dev, mode, data, mw)
    other.update_vertices(deformed)
    _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), name + " (after an update)")


# ---- 3. dense and sparse in turn
def test_dense_and_sparse_sets_replace_each_other(dev, other):
    scene, params, bones, weights, n_bones, pose, _, o, v, d, mw = _morph_case(_c1)
    rest = _verts(scene)
    n = rest.shape[0]
    dense, mw_dense = _targets(rest, 8)
    dense = np.concatenate([dense, dense[:1]])  # four dense targets against three sparse ones: the counts tell which set the rig holds
    mw_dense = np.concatenate([mw_dense, [0.2]]).astype(np.float32)
    sparse_out = host.deform_vertices_sparse(rest, bones, weights, pose, 0, o, v, d, mw)
    dense_out = host.deform_vertices(rest, bones, weights, pose, 0, dense, mw_dense)

    def refused(fn, *args):
        with pytest.raises(device.GlrtxError) as e:
            fn(*args)
        assert e.value.code == -1, e.value

    def same(vertices, what):
        other.update_vertices(vertices)
        _assert_same_scene(_scene_bytes(dev), _scene_bytes(other), what)

    _setup(dev, scene, params); _setup(other, scene, params)
    dev.upload_rig(rest, bones, weights, n_bones)
    dev.upload_morph_targets(dense)
    dev.pose_morph(pose, mw_dense); same(dense_out, "dense first")
    dev.upload_morph_targets_sparse(o, v, d)  # replaces the dense set
    refused(dev.pose_morph, pose, mw_dense)
    dev.pose_morph(pose, mw); same(sparse_out, "sparse after dense")
    dev.upload_morph_targets(dense)  # and back
    refused(dev.pose_morph, pose, mw)
    dev.pose_morph(pose, mw_dense); same(dense_out, "dense after sparse")
    dev.upload_morph_targets_sparse(o, v, d)
    dev.upload_morph_targets(None)  # the dense call with no targets drops a sparse set
    refused(dev.pose_morph, pose, mw)
    dev.pose_morph(pose); same(host.skin_vertices(rest, bones, weights, pose), "no set")
    dev.upload_morph_targets(dense)
    dev.upload_morph_targets_sparse(None)  # the sparse call with no targets drops a dense set
    refused(dev.pose_morph, pose, mw_dense)
    dev.pose_morph(pose)
    # 65 targets through the context call: target k moves vertex 3 k .. 3 k + 2
    rng = np.random.default_rng(65)
    big = np.zeros((65, n, 6), np.float32)
    for k in range(65):
        big[k, 3 * k:3 * k + 3, 0:3] = rng.normal(0, 0.03, (3, 3))
    ob, vb, db = host.morph_sparsify(big)
    assert int(ob[-1]) == 195
    wb = rng.uniform(-1, 1, 65).astype(np.float32)
    wb[7] = 0.0
    dev.upload_morph_targets_sparse(ob, vb, db)
    dev.pose_morph(pose, wb); same(host.deform_vertices_sparse(rest, bones, weights, pose, 0, ob, vb, db, wb), "65 targets")
    refused(dev.pose_morph, pose, wb[:64])
    # a set without entries, and weights for it: Posing
    dev.upload_morph_targets_sparse(np.zeros(4, np.uint64))
    dev.pose_morph(pose, mw); same(host.skin_vertices(rest, bones, weights, pose), "three empty targets")
    # upload_rig and upload_scene forget the set
    dev.upload_morph_targets_sparse(o, v, d)
    dev.upload_rig(rest, bones, weights, n_bones)
    refused(dev.pose_morph, pose, mw)
    dev.pose_morph(pose)
    dev.upload_morph_targets_sparse(o, v, d)
    dev.upload_scene(scene)
    refused(dev.pose_morph, pose, mw)
    refused(dev.upload_morph_targets_sparse, o, v, d)


# ---- 4. reprojection
def test_reprojection_sees_a_sparse_pose_as_it_sees_an_update(dev, other):
    """test_gpu_deform's sequence: track_motion, 4 frames, render_features, pose_morph, reproject_motion against update_vertices(deformed)."""
    scene, params, bones, weights, n_bones, pose, _, o, v, d, mw = _morph_case(_c1)
    rest = _verts(scene)
    deformed = host.deform_vertices_sparse(rest, bones, weights, pose, 0, o, v, d, mw)
    out = []
    for dv, move in ((dev, lambda: dev.pose_morph(pose, mw)), (other, lambda: other.update_vertices(deformed))):
        _setup(dv, scene, params)
        dv.track_motion(True)
        if dv is dev:
            dv.upload_rig(rest, bones, weights, n_bones)
            dv.upload_morph_targets_sparse(o, v, d)
        for f in range(4):
            dv.render(dict(params, seed=host.frame_seed(f)))
        dv.render_features(params)
        move()
        dv.reproject_motion(params)
        out.append((dv.read_accum(), dv.reproject_last(), dv.read_features_geom()))
    assert (_bits(out[0][0]) == _bits(out[1][0])).all()
    assert out[0][1] == out[1][1] and 0 < out[0][1][0] <= out[0][1][1]
    assert (_bits(out[0][2]) == _bits(out[1][2])).all()


# ---- 5. refusals
def test_refusals(dev):
    scene, params, bones, weights, n_bones, pose, _, o, v, d, mw = _morph_case(_c1)
    rest = _verts(scene)
    n = rest.shape[0]
    dq = rig.dualquat(_gentle_pose(n_bones, 4, (0.0, 1.0, 0.0)))

    def refused(fn, *args, message=None, **kw):
        with pytest.raises(device.GlrtxError) as e:
            fn(*args, **kw)
        assert e.value.code == -1, e.value
        if message:
            assert message in str(e.value), e.value

    refused(dev.upload_morph_targets_sparse, o, v, d, n_vert=n, message="no rig")  # no scene
    _setup(dev, scene, params)
    before = _scene_bytes(dev)
    refused(dev.upload_morph_targets_sparse, o, v, d, n_vert=n, message="no rig")  # a set before the rig
    dev.upload_rig(rest, bones, weights, n_bones)
    refused(dev.deform_burst_ms, 2)  # (the timing hook: nothing deformed yet)
    refused(dev.upload_morph_targets_sparse, o, v, d, n_vert=n - 1, message=f"{n - 1} vertices, the rig has {n}")
    refused(dev.upload_morph_targets_sparse, np.zeros(1026, np.uint64), message="1025 sparse morph targets")
    o2 = o.copy(); o2[0] = 1
    refused(dev.upload_morph_targets_sparse, o2, v, d, message="offsets[0] is 1")
    o2 = o.copy(); o2[2] = o[1] - 1
    refused(dev.upload_morph_targets_sparse, o2, v, d, message="target 1: offsets decrease")
    v2 = v.copy(); v2[int(o[2]) + 4] = n
    refused(dev.upload_morph_targets_sparse, o, v2, d, message=f"target 2, entry 4: vertex index {n} of {n}")
    v2 = v.copy(); v2[5] = v2[4]
    refused(dev.upload_morph_targets_sparse, o, v2, d, message="target 0, entry 5")
    u64, u32, fp = (dev.L.glrtx_upload_morph_targets_sparse.argtypes[k] for k in (1, 2, 3))
    assert dev.L.glrtx_upload_morph_targets_sparse(dev.h, o.ctypes.data_as(u64), None, d.ctypes.data_as(fp), 3, n) == -1
    assert dev.L.glrtx_upload_morph_targets_sparse(dev.h, o.ctypes.data_as(u64), v.ctypes.data_as(u32), None, 3, n) == -1
    assert dev.L.glrtx_upload_morph_targets_sparse(dev.h, None, v.ctypes.data_as(u32), d.ctypes.data_as(fp), 3, n) == -1
    big = np.array([0, 0, 0, 2 ** 31], np.uint64)
    assert dev.L.glrtx_upload_morph_targets_sparse(dev.h, big.ctypes.data_as(u64), v.ctypes.data_as(u32), d.ctypes.data_as(fp), 3, n) == -1
    refused(dev.pose_morph, pose, mw)  # none of them left a set behind
    dev.upload_morph_targets_sparse(o, v, d)
    refused(dev.pose_morph, pose, None)  # wrong n_targets
    refused(dev.pose_morph, pose, mw[:-1])
    refused(dev.pose_dualquat, dq, np.concatenate([mw, mw[:1]]))
    refused(dev.pose_morph, pose, np.zeros(1025, np.float32))
    refused(dev.pose_morph, pose[:-1], mw)  # wrong n_bones
    for bad_value in (np.nan, np.inf, -np.inf):
        bad = mw.copy(); bad[1] = bad_value
        refused(dev.pose_morph, pose, bad)
        refused(dev.pose_dualquat, dq, bad)
    o2 = o.copy(); o2[0] = 1
    refused(dev.upload_morph_targets_sparse, o2, v, d)  # a refused upload keeps the set that is there
    _assert_same_scene(_scene_bytes(dev), before, "after the refusals")
    refused(dev.deform_burst_ms, 2)  # still nothing deformed
    dev.pose_morph(pose, mw)  # with everything in place it goes through -- the set survived the refused upload
    posed = _scene_bytes(dev)
    assert any((posed[w] != before[w]).any() for w in ("nodes", "nrms"))
    assert dev.deform_burst_ms(2) > 0.0  # replays the sparse launch
    dev.pose_dualquat(dq, mw)
    assert dev.deform_burst_ms(2) > 0.0
    dev.pose_morph(pose, np.zeros_like(mw))  # no active weight: the dense kernel with no active target, replayed as such
    assert dev.deform_burst_ms(2) > 0.0
    dev.pose_morph(pose, mw)
    _assert_same_scene(_scene_bytes(dev), posed, "after the timing hook and other poses in between")
