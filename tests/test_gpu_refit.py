"""glrtx_update_vertices on the device (csrc/refit.hip.h): the packed scene equals, byte for byte, an upload of the new vertices with the CPU-refitted tree
(glrt_bvh_refit); images after an update are the oracle's for that scene, in every kernel form; updates are ordered against launches still in flight (render_frames,
fed single-frame launches on the pipe slots, groups, a torch tensor produced on the context's stream); errors and same-vertex updates change nothing."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from fuzz_scenes import case_scene_and_params, fuzz_scene
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def other_device():
    d = device.Device()
    yield d
    d.close()


def _moved(scene, seed, scale=1.0):
    """Vertices rotated, translated, jittered (scale: of the motion), normals changed; light triangles move with their vertices."""
    rng = np.random.default_rng(seed)
    v = scene["vert"].reshape(-1, 15).copy()
    p = v[:, :3].astype(np.float64)
    a = scale * rng.uniform(0, 0.6)
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    p = p @ R.T + scale * rng.normal(0, 0.2, 3) + scale * rng.normal(0, 0.01, p.shape)
    v[:, :3] = p.astype(np.float32)
    n = v[:, 3:6] + scale * rng.normal(0, 0.2, (len(v), 3)).astype(np.float32)
    v[:, 3:6] = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-6).astype(np.float32)
    return v


def _refitted(scene, v):
    """The scene glrtx_upload_scene should end up equal to: the new vertices, the old tree refitted on the CPU."""
    return dict(scene, vert=np.ascontiguousarray(v.reshape(-1, 3)), bvh=host.refit_bvh(v, scene["tri"], scene["bvh"]))


def _denormal_scene():
    """Triangles of denormal size next to ordinary ones: edge vectors and box bounds that a flushed subtraction or comparison would change."""
    pos, nrm, _ = scenes.random_triangles(40, 5, 1.0, 0.5)
    pos[:20] *= np.float32(1e-39)
    pos[20:25, :, 0] = np.float32(-0.0)
    b = scenes.SceneBuilder()
    m0 = b.add_material(scenes.diffuse((0.5, 0.5, 0.5)))
    m1 = b.add_material(scenes.emitter((4.0, 4.0, 4.0)))
    b.add_mesh(pos, nrm, np.where(np.arange(40) % 9 == 0, m1, m0))
    return b.build("sah")


def _denormal_motion(scene, seed):
    v = scene["vert"].reshape(-1, 15).copy()
    rng = np.random.default_rng(seed)
    v[:60, :3] = (rng.normal(0, 1, (60, 3)) * 3e-39).astype(np.float32)  # denormal positions, denormal differences
    v[60:, :3] += rng.normal(0, 0.05, (len(v) - 60, 3)).astype(np.float32)
    return v


def _scene_bytes(d):
    return {w: d.read_scene(w) for w in device.SCENE_BUFFERS}


def _assert_same_scene(a, b, what):
    for w in device.SCENE_BUFFERS:
        assert a[w].size == b[w].size, (what, w, a[w].size, b[w].size)
        bad = np.flatnonzero(a[w] != b[w])
        assert bad.size == 0, f"{what}: {w} differs in {bad.size} bytes, first at byte {bad[0] if bad.size else -1}"


BYTE_CASES = [
    ("fuzz-sah", lambda: fuzz_scene(51, 150, "sah"), _moved),
    ("fuzz-reference", lambda: fuzz_scene(52, 120, "reference", duplicates=True), _moved),
    ("fuzz-lbvh-degenerate", lambda: fuzz_scene(53, 100, "lbvh", degenerate=True, duplicates=True), _moved),
    ("chain", lambda: fuzz_scene(54, 90, "chain"), _moved),
    ("chain-5000", lambda: scenes.config_c3(64, 64, n=5000)[0], _moved),
    ("c1-default", lambda: scenes.config_c1(64, 64, subdiv=2)[0], _moved),
    ("random-20000", lambda: scenes.config_c5(64, 64, n=20_000)[0], _moved),
    ("denormal", _denormal_scene, _denormal_motion),
]


@pytest.mark.parametrize("chains", [True, False], ids=["leaf-chains", "no-leaf-chains"])
@pytest.mark.parametrize("name,make,motion", BYTE_CASES, ids=[c[0] for c in BYTE_CASES])
def test_update_packs_what_an_upload_of_the_refitted_tree_packs(gpu_device, other_device, monkeypatch, name, make, motion, chains):
    if not chains:
        monkeypatch.setenv("GLRTX_NO_LEAF_CHAINS", "1")
    sc = make()
    v = motion(sc, 7)
    gpu_device.upload_scene(sc)
    gpu_device.update_vertices(v)
    other_device.upload_scene(_refitted(sc, v))
    _assert_same_scene(_scene_bytes(gpu_device), _scene_bytes(other_device), name)
    # a second update lands where an upload of the second refit lands (the boxes of the first one are not what the second starts from)
    v2 = motion(sc, 8)
    gpu_device.update_vertices(v2)
    other_device.upload_scene(_refitted(sc, v2))
    _assert_same_scene(_scene_bytes(gpu_device), _scene_bytes(other_device), name + " (second update)")


def test_update_with_the_same_vertices_changes_no_byte(gpu_device):
    sc, _ = scenes.config_c1(64, 64, subdiv=2)
    gpu_device.upload_scene(sc)
    before = _scene_bytes(gpu_device)
    gpu_device.update_vertices(sc["vert"].reshape(-1, 15))
    _assert_same_scene(_scene_bytes(gpu_device), before, "same vertices")


def test_errors_leave_the_scene_unchanged(gpu_device):
    d = device.Device()
    with pytest.raises(device.GlrtxError) as e:
        d.update_vertices(np.zeros((3, 15), np.float32))  # no scene
    assert e.value.code == -1
    d.close()
    sc = fuzz_scene(55, 40, "sah")
    gpu_device.upload_scene(sc)
    before = _scene_bytes(gpu_device)
    v = _moved(sc, 1)
    for bad in (v[:-1], np.concatenate([v, v[:1]])):
        with pytest.raises(device.GlrtxError) as e:
            gpu_device.update_vertices(bad)
        assert e.value.code == -1
    with pytest.raises(TypeError):
        gpu_device.update_vertices(v.astype(np.float64))
    _assert_same_scene(_scene_bytes(gpu_device), before, "after refused updates")


def _setup(d, scene, params, variant=2):
    d.upload_scene(scene)
    d.set_variant(variant)
    d.set_partition(0, 1, 16)
    d.resize(params["width"], params["height"])
    d.clear()
    d.reset_stats()
    d.count_rays(True)


FORMS = [(0, None, None), (1, None, None), (2, "0", "0"), (2, "0", "1"), (2, "1", None), (2, "2", None)]


@pytest.mark.parametrize("variant,fetch,compact", FORMS, ids=[f"v{v}-fetch{f}-compact{c}" for v, f, c in FORMS])
@pytest.mark.parametrize("case", [0, 2], ids=["sah", "chain"])
def test_image_after_an_update_is_the_oracles(gpu_device, monkeypatch, variant, fetch, compact, case):
    from fuzz_scenes import CASES
    from oracle import pt_oracle
    if fetch is not None:
        monkeypatch.setenv("GLRTX_PAIR_FETCH", fetch)
    if compact is not None:
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
    sc, params = case_scene_and_params(CASES[case])
    v = _moved(sc, 3)
    d = gpu_device
    _setup(d, sc, params, variant)
    d.update_vertices(v)
    d.render(params)
    d.sync()
    ref, rays = pt_oracle.render(_refitted(sc, v), params)
    st = d.stats()
    assert st.rays == rays
    assert_bit_equal(d.read_accum(), ref, f"variant {variant} fetch {fetch} compact {compact} after an update")
    d.set_variant(2)
    d.count_rays(False)


def test_render_frames_update_render_frames_is_old_then_new_frames(gpu_device):
    from oracle import pt_oracle
    sc, params = scenes.config_c1(160, 120, max_depth=4, subdiv=2)
    v = _moved(sc, 4)
    seeds = [host.frame_seed(i) for i in range(4)]
    d = gpu_device
    _setup(d, sc, params)
    d.render_frames(params, seeds[:2])
    d.update_vertices(v)  # no sync: the update must wait for the frames in flight
    d.render_frames(params, seeds[2:])
    d.sync()
    ref, rays = None, 0
    new = _refitted(sc, v)
    for k, sd in enumerate(seeds):
        ref, n = pt_oracle.render(sc if k < 2 else new, dict(params, seed=sd), accum=ref)
        rays += n
    assert d.stats().rays == rays
    assert_bit_equal(d.read_accum(), ref, "two old frames, the update, two new frames")
    d.count_rays(False)


def test_animation_loop_of_single_frame_renders_matches_frame_by_frame(gpu_device):
    """An update before every glrtx_render, no sync in the loop: fed launches and pipe-slot streams on both sides of every refit."""
    from oracle import pt_oracle
    sc, params = scenes.config_c1(160, 120, max_depth=4, subdiv=2)
    d = gpu_device
    _setup(d, sc, params)
    ref, rays = None, 0
    for f in range(8):
        v = _moved(sc, 100 + f, scale=0.3 * f)
        sd = host.frame_seed(f)
        d.update_vertices(v)
        d.render(dict(params, seed=sd))
        ref, n = pt_oracle.render(_refitted(sc, v), dict(params, seed=sd), accum=ref)
        rays += n
    d.sync()
    assert d.stats().rays == rays
    assert_bit_equal(d.read_accum(), ref, "animation loop")
    d.count_rays(False)


def test_group_update(gpu_device):
    from oracle import pt_oracle
    sc, params = scenes.config_c1(96, 80, max_depth=3, subdiv=2)
    v = _moved(sc, 6)
    g = device.Group([0, 0])
    try:
        g.upload_scene(sc)
        g.resize(params["width"], params["height"])
        g.clear()
        g.render(params)
        g.update_vertices(v)
        sd = host.frame_seed(1)
        g.render(dict(params, seed=sd))
        g.sync()
        ref, _ = pt_oracle.render(sc, params)
        ref, _ = pt_oracle.render(_refitted(sc, v), dict(params, seed=sd), accum=ref)
        assert_bit_equal(g.read_accum(), ref, "group: one old frame, the update, one new frame")
        with pytest.raises(device.GlrtxError):
            g.update_vertices(v[:-1])
    finally:
        g.close()


def test_torch_tensor_update_ordered_on_the_contexts_stream(gpu_device):
    import torch
    from oracle import pt_oracle
    sc, params = scenes.config_c1(96, 80, max_depth=3, subdiv=2)
    v = _moved(sc, 9)
    d = gpu_device
    _setup(d, sc, params)
    s = torch.cuda.Stream()
    d.set_stream(s.cuda_stream)
    try:
        with torch.cuda.stream(s):  # the deformation is computed on the context's stream: no sync before the update
            base = torch.from_numpy(sc["vert"].reshape(-1, 15).copy()).cuda()
            t = base + (torch.from_numpy(v).cuda() - base)
            t = t.contiguous()
        with pytest.raises(TypeError):
            d.update_vertices(t.double())
        with pytest.raises(ValueError):
            d.update_vertices(t[:, :14].contiguous())
        d.update_vertices(t)
        d.render(params)
        d.sync()
        ref, rays = pt_oracle.render(_refitted(sc, t.cpu().numpy()), params)  # (the tensor's own values are what the oracle is given)
        assert d.stats().rays == rays
        assert_bit_equal(d.read_accum(), ref, "torch tensor update")
    finally:
        d.set_stream(0)
        d.count_rays(False)
