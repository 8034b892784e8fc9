"""Every call that moves geometry, through the one move path (csrc/glrtx.hip: move_begin, move_commit; DESIGN.md "A geometry move"): what a shared path can lose
without any error, for all the movers at once.  Each mover takes the motion snapshot, once, of the feature pass's geometry; each seals an open launch and waits
for the slots; the timing hooks replay the last pose launch, leave the scene alone and refuse when there is nothing to replay.  The movers' vertices come from
the CPU statements; what a mover leaves in the scene buffers is pinned by the per-feature files."""
import numpy as np
import pytest

from glrt_amd import device, host, rig
from test_gpu_deform import _gentle_pose, _targets
from test_gpu_deform_sparse import _sparse_targets
from test_gpu_skin import _assert_same_scene, _c1, _rigid_case, _scene_bytes, _setup, _verts
from test_reproject_motion_host import lifted

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _refused(fn, *args):
    with pytest.raises(device.GlrtxError) as e:
        fn(*args)
    assert e.value.code == -1, e.value


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


@pytest.fixture(scope="module")
def other(gpu_device):
    d = device.Device()
    yield d
    d.close()


class World:
    """Config 1 at 64x48 with a rigid rig by material, a dense and a sparse set of three targets, the normal topology, and every mover's input."""

    def __init__(self):
        self.scene, self.params, self.bones, self.weights, self.n_bones, self.pose = _rigid_case(_c1)
        self.rest, self.tri = _verts(self.scene), self.scene["tri"]
        self.dq = rig.dualquat(_gentle_pose(self.n_bones, 4, (0.0, 1.0, 0.0)))
        self.dense, self.mw = _targets(self.rest, 8)
        self.so, self.sv, self.sd, self.smw = _sparse_targets(self.rest, 8)
        self.cls, self.flip, _ = host.normal_topology(self.rest, self.tri)
        self.pos = lifted(self.scene, 1, 0.4)[:, 0:3].copy()
        self._tensors = {}

    def rebuilt(self, v):
        return host.rebuild_normals(v, self.tri, self.cls, self.flip)

    def tensor(self, name):
        """The array `name` on the GPU, made once (and complete before any context reads it on its own stream)."""
        import torch
        if name not in self._tensors:
            self._tensors[name] = torch.from_numpy(getattr(self, name)).cuda().contiguous()
            torch.cuda.synchronize()
        return self._tensors[name]

    def rig(self, d):
        d.upload_rig(self.rest, self.bones, self.weights, self.n_bones)

    def topology(self, d):
        d.upload_normal_topology(self.rest, self.tri)


@pytest.fixture(scope="module")
def W():
    w = World()
    r, b, wt = w.rest, w.bones, w.weights
    w.skinned = host.skin_vertices(r, b, wt, w.pose)
    w.moved = w.rebuilt(host.positions_to_vertices(r, w.pos))
    w.morphed = host.deform_vertices(r, b, wt, w.pose, 0, w.dense, w.mw)
    w.morphed_sparse = host.deform_vertices_sparse(r, b, wt, w.pose, 0, w.so, w.sv, w.sd, w.smw)
    w.dualquat = host.deform_vertices(r, b, wt, w.dq, 1)
    for name in ("skinned", "moved", "morphed", "morphed_sparse", "dualquat"):
        assert (_bits(getattr(w, name)) != _bits(r)).any(), name
    return w


def _with_normals(prepare):
    def both(d, w):
        prepare(d, w)
        w.topology(d)
        d.set_pose_normals(True)
    return both


def _rig_dense(d, w):
    w.rig(d)
    d.upload_morph_targets(w.dense)


def _rig_sparse(d, w):
    w.rig(d)
    d.upload_morph_targets_sparse(w.so, w.sv, w.sd)


# (name, what the context needs before the frames, the move, the vertices the CPU statements give for it)
MOVERS = [
    ("update_vertices numpy", lambda d, w: None, lambda d, w: d.update_vertices(w.skinned), lambda w: w.skinned),
    ("update_vertices tensor", lambda d, w: w.tensor("skinned"), lambda d, w: d.update_vertices(w.tensor("skinned")), lambda w: w.skinned),
    ("update_positions numpy", lambda d, w: w.topology(d), lambda d, w: d.update_positions(w.pos), lambda w: w.moved),
    ("update_positions tensor", lambda d, w: (w.topology(d), w.tensor("pos")), lambda d, w: d.update_positions(w.tensor("pos")), lambda w: w.moved),
    ("pose", lambda d, w: w.rig(d), lambda d, w: d.pose(w.pose), lambda w: w.skinned),
    ("pose_morph dense", _rig_dense, lambda d, w: d.pose_morph(w.pose, w.mw), lambda w: w.morphed),
    ("pose_morph sparse", _rig_sparse, lambda d, w: d.pose_morph(w.pose, w.smw), lambda w: w.morphed_sparse),
    ("pose_dualquat", lambda d, w: w.rig(d), lambda d, w: d.pose_dualquat(w.dq), lambda w: w.dualquat),
    ("pose, normals rebuilt", _with_normals(lambda d, w: w.rig(d)), lambda d, w: d.pose(w.pose), lambda w: w.rebuilt(w.skinned)),
    ("pose_morph, normals rebuilt", _with_normals(_rig_dense), lambda d, w: d.pose_morph(w.pose, w.mw), lambda w: w.rebuilt(w.morphed)),
    ("pose_dualquat, normals rebuilt", _with_normals(lambda d, w: w.rig(d)), lambda d, w: d.pose_dualquat(w.dq), lambda w: w.rebuilt(w.dualquat)),
]
BY_NAME = {m[0]: m for m in MOVERS}


# ---- 1. the motion snapshot
def _reprojected(d, w, prepare, moves):
    """track_motion, 4 frames, render_features, the moves, reproject_motion: (accumulator, (carried, hit_pixels), G)."""
    _setup(d, w.scene, w.params)
    d.track_motion(True)
    prepare(d, w)
    for f in range(4):
        d.render(dict(w.params, seed=host.frame_seed(f)))
    d.render_features(w.params)
    for move in moves:
        move(d, w)
    d.reproject_motion(w.params)
    return d.read_accum(), d.reproject_last(), d.read_features_geom()


def _assert_same_reprojection(got, want, what):
    assert (_bits(got[0]) == _bits(want[0])).all(), f"{what}: {int((_bits(got[0]) != _bits(want[0])).any(-1).sum())} accumulator pixels differ"
    assert got[1] == want[1] and 0 < got[1][0] <= got[1][1], (what, got[1], want[1])
    assert (_bits(got[2]) == _bits(want[2])).all(), f"{what}: the G plane differs"


_updates = {}


def _after_updates(other, w, *vertices):
    """The sequence with update_vertices from numpy for each of `vertices`: computed once a set, shared by the movers that give the same vertices."""
    key = tuple(id(v) for v in vertices)
    if key not in _updates:
        _updates[key] = (vertices, _reprojected(other, w, lambda d, w: None, [lambda d, w, v=v: d.update_vertices(v) for v in vertices]))
    return _updates[key][1]


@pytest.fixture(scope="module")
def expected(W):
    """Each mover's vertices, made once: the reference sequences are keyed by them."""
    return {name: vertices(W) for name, _, _, vertices in MOVERS}


@pytest.mark.parametrize("name", [m[0] for m in MOVERS])
def test_every_mover_takes_the_snapshot(dev, other, W, expected, name):
    """The reprojection after the mover carries exactly what it carries after update_vertices of the mover's vertices: the previous geometry was kept, and
    something was carried (without the snapshot the moved object's samples are looked up against the new geometry and the counts differ)."""
    _, prepare, move, _ = BY_NAME[name]
    _assert_same_reprojection(_reprojected(dev, W, prepare, [move]), _after_updates(other, W, expected[name]), name)


def test_the_snapshot_is_the_feature_passes_geometry_taken_once(dev, other, W):
    """Two moves by different movers before the reprojection: the second one must not overwrite the previous geometry with the first one's."""
    def prepare(d, w):
        w.rig(d)
        w.topology(d)
    got = _reprojected(dev, W, prepare, [BY_NAME["pose"][2], BY_NAME["update_positions numpy"][2]])
    _assert_same_reprojection(got, _after_updates(other, W, W.skinned, W.moved), "pose, then update_positions")


# ---- 2. the feed seal and the wait for the slots
@pytest.mark.parametrize("name", ["update_vertices numpy", "update_vertices tensor", "update_positions numpy", "pose"])
def test_every_mover_seals_an_open_launch_and_waits_for_the_slots(dev, other, W, name):
    """6 frames of one camera with no sync in between leave a fed launch open; the mover comes at once, then 2 more frames.  The first six see the old
    geometry and the last two the new one, exactly as with a sync() in front of the mover.  One mover from each head."""
    _, prepare, move, _ = BY_NAME[name]
    out = []
    for d, wait in ((dev, False), (other, True)):
        _setup(d, W.scene, W.params)
        prepare(d, W)
        for f in range(6):
            d.render(dict(W.params, seed=host.frame_seed(f)))
        if wait:
            d.sync()
        move(d, W)
        for f in range(6, 8):
            d.render(dict(W.params, seed=host.frame_seed(f)))
        out.append(d.read_accum())
    bad = (_bits(out[0]) != _bits(out[1])).any(-1)
    assert not bad.any(), f"{name}: {int(bad.sum())} pixels differ from the sequence with a sync in front of the mover"


# ---- 3. the timing hooks and the record of the last pose launch
def test_burst_hooks_replay_the_last_pose_launch_and_leave_the_scene(dev, W):
    w = W
    _setup(dev, w.scene, w.params)
    _rig_dense(dev, w)
    _refused(dev.deform_burst_ms, 2)  # nothing deformed yet

    def replays(what):
        before = _scene_bytes(dev)
        assert dev.deform_burst_ms(2) > 0.0, what
        _assert_same_scene(_scene_bytes(dev), before, what + " (deform_burst_ms)")
        assert dev.skin_burst_ms(2) > 0.0, what
        _assert_same_scene(_scene_bytes(dev), before, what + " (skin_burst_ms)")

    dev.pose_morph(w.pose, w.mw)
    replays("after a dense pose")
    dev.upload_morph_targets_sparse(w.so, w.sv, w.sd)  # drops the dense set and the record with it
    _refused(dev.deform_burst_ms, 2)
    assert dev.skin_burst_ms(2) > 0.0  # (the rig and the vertex buffer are still there)
    dev.pose_morph(w.pose, w.smw)
    replays("after a sparse pose")
    dev.pose_morph(w.pose, np.zeros_like(w.smw))  # no active weight: the pose ran the dense kernel with no active target, and that is what is replayed
    replays("after a sparse set with all-zero weights")
    dev.pose(w.pose)  # glrtx_pose leaves the record: the deform hook still replays the last deform launch
    replays("after a pose behind a pose_morph")
    dev.upload_morph_targets(w.dense)  # an upload drops the record
    _refused(dev.deform_burst_ms, 2)
    # a new context that has only ever been moved from a tensor has no vertex buffer of its own (the module's contexts got theirs in the tests above): both
    # hooks refuse, before and after the move
    fresh = device.Device()
    try:
        _setup(fresh, w.scene, w.params)
        _rig_dense(fresh, w)
        fresh.upload_morph_targets(None)  # drops the set
        _refused(fresh.deform_burst_ms, 2)
        _refused(fresh.skin_burst_ms, 2)
        fresh.update_vertices(w.tensor("skinned"))
        _refused(fresh.deform_burst_ms, 2)
        _refused(fresh.skin_burst_ms, 2)
    finally:
        fresh.close()
