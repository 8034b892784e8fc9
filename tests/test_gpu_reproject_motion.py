"""Reprojection across a geometry move on the GPU (csrc/reproject_motion.hip.h, csrc/features.hip.h): the kernel equals the CPU statement
(glrt_reproject_motion) on hostile arrays; the feature pass with the geometry plane equals glrt_render_features_geom in both node layouts, with the pair
fetch and on a vine, and leaves N and A what they are with tracking off; Device.reproject_motion after an update_vertices equals the CPU statement fed with
what the device held, with the previous geometry being the one of the last feature pass; every refusal is GLRTX_EINVAL and changes nothing; and tracking
changes nothing else."""
import ctypes as C

import numpy as np
import pytest

import reproject_math as rm
import reproject_motion_math as rmm
from glrt_amd import device, host, scenes
from test_reproject_motion_host import lifted, moved_scene

pytestmark = pytest.mark.gpu

CFG2 = dict(max_history=2, depth_tolerance=0.2, normal_tolerance=-1.0)
SPHERE, LIFT = 5, 0.3


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} of {bad.shape[0] * bad.shape[1]} pixels differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0][:2])].tolist()} vs {ref[tuple(np.argwhere(bad)[0][:2])].tolist()}"


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


def _accum_ptr(d):
    p, pitch = C.c_void_p(), C.c_size_t()
    d._ck(d.L.glrtx_accum_device_ptr(d.h, C.byref(p), C.byref(pitch)))
    return p.value, pitch.value


@pytest.fixture()
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, track=True):
    d.set_variant(2)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()
    d.track_motion(track)


def _verts(scene):
    return np.ascontiguousarray(np.asarray(scene["vert"], np.float32).reshape(-1, 15))


# ---- 5. device against CPU
@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (5, 130), (1, 1), (70, 49)])
def test_kernel_on_hostile_arrays(gpu_device, rows, width):
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, g1, a1, vert, tri = rmm.hostile_arrays(rows, width, rows * 1000 + width)
    cfgs = [{}, CFG2, dict(max_history=1000, depth_tolerance=1e3, normal_tolerance=-2.0), dict(max_history=1, depth_tolerance=1e-40, normal_tolerance=1e-40),
            dict(max_history=2 ** 31 - 1, depth_tolerance=3e38, normal_tolerance=-3e38)]
    some = 0
    for prev in (params, rm.move_camera(params, "pan", 1.0), rm.move_camera(params, "dolly", 0.3), rm.move_camera(params, "orbit", 2.0),
                 rm.move_camera(params, "pan", 180.0)):
        for cfg in cfgs:
            got, carried, hits = device.debug_reproject_motion(acc, n0, a0, g1, a1, vert, tri, prev, **cfg)
            ref, carried_ref, hits_ref = host.reproject_motion(acc, n0, a0, g1, a1, vert, tri, prev, **cfg)
            _same(got, ref, f"{width}x{rows} {cfg}")
            assert (carried, hits) == (carried_ref, hits_ref)
            some += carried
    assert carried == 0 and not got.any()  # (the last camera looks away)
    assert some > 0 or rows * width == 1
    for n_tri in (0, 1, tri.shape[0] // 2):  # a carried range that ends early
        got, carried, hits = device.debug_reproject_motion(acc, n0, a0, g1, a1, vert, tri[:n_tri], params, **CFG2)
        ref, carried_ref, hits_ref = host.reproject_motion(acc, n0, a0, g1, a1, vert, tri[:n_tri], params, **CFG2)
        _same(got, ref, f"{width}x{rows} {n_tri} triangles")
        assert (carried, hits) == (carried_ref, hits_ref)


def _planes_against_cpu(d, scene, params, what):
    _setup(d, scene, params)
    d.render_features(params)
    n, a = d.read_features()
    g = d.read_features_geom()
    rn, ra, rg = host.render_features_geom(scene, params)
    _same(n, rn, f"{what}: N"); _same(a, ra, f"{what}: A"); _same(g, rg, f"{what}: G")
    d.track_motion(False)
    d.render_features(params)
    n_off, a_off = d.read_features()
    _same(n, n_off, f"{what}: N with tracking on against off"); _same(a, a_off, f"{what}: A with tracking on against off")
    with pytest.raises(device.GlrtxError):
        d.read_features_geom()
    return g


@pytest.mark.parametrize("compact", ["0", "1"])
def test_planes_headline(dev, monkeypatch, compact):
    monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
    scene, params = scenes.config_headline(480, 270)
    g = _planes_against_cpu(dev, scene, params, f"headline compact={compact}")
    assert (g[..., 0].view(np.int32) >= 0).mean() > 0.5


def test_planes_config5_and_a_chain(dev):
    scene, params = scenes.config_c5(320, 180)  # (100,000 triangles: the layout the pair fetch walks)
    _planes_against_cpu(dev, scene, params, "config 5")
    scene, params = scenes.config_c3(96, 64, n=3000)
    _planes_against_cpu(dev, scene, params, "chain")
    scene, params = scenes.config_c2(61, 37)
    _planes_against_cpu(dev, scene, params, "c2 61x37")


# ---- 6. the whole sequence against the CPU statement
def _sequence(d, scene, pa, updates, cfg, what, tensor=False, adaptive=False, frames=4):
    """track, features, frames, the updates, reproject_motion: the accumulator against the CPU statement fed with what the device held before the call and the
    vertices of the last feature pass."""
    import torch
    _setup(d, scene, pa)
    d.render_features(pa)
    if adaptive:
        d.render_adaptive(pa, _seeds(frames), -1.0, 2)
        assert d.read_adaptive_half()[..., 3].max() > 0
    else:
        for sd in _seeds(frames):
            d.render(dict(pa, seed=sd))
    keep = []
    for v in updates:
        if tensor:
            t = torch.from_numpy(v).cuda()
            torch.cuda.synchronize()
            keep.append(t)
            d.update_vertices(t)
        else:
            d.update_vertices(v)
    acc0 = d.read_accum()
    n0, a0 = d.read_features()
    ptr0 = _accum_ptr(d)
    d.reproject_motion(pa, **cfg)
    out = d.read_accum()
    n1, a1 = d.read_features()
    g1 = d.read_features_geom()
    carried, hits = d.reproject_last()
    last = updates[-1] if updates else _verts(scene)
    rn, ra, rg = host.render_features_geom(moved_scene(scene, last), pa)
    _same(n1, rn, f"{what}: N1"); _same(a1, ra, f"{what}: A1"); _same(g1, rg, f"{what}: G1")
    ref, carried_ref, hits_ref = host.reproject_motion(acc0, n0, a0, g1, a1, _verts(scene), scene["tri"], pa, **cfg)
    _same(out, ref, what)
    assert (carried, hits) == (carried_ref, hits_ref), (what, carried, hits, carried_ref, hits_ref)
    assert _accum_ptr(d)[0] != ptr0[0] and _accum_ptr(d)[1] == ptr0[1], f"{what}: the accumulators were not swapped"
    if adaptive:
        assert not d.read_adaptive_half().any(), f"{what}: the half buffer was not zeroed"
    return out, carried, hits, ptr0


@pytest.mark.parametrize("size", [(192, 108), (1920, 1080)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_one_sphere_moves(dev, size):
    scene, pa = scenes.config_headline(*size)
    v1 = lifted(scene, SPHERE, LIFT)
    for cfg in ({}, CFG2):
        out, carried, hits, _ = _sequence(dev, scene, pa, [v1], cfg, f"lift {size} {cfg}", frames=4)
        assert carried > 0.9 * hits
    # the sphere's pixels carry what the static call, looking where the sphere is now, would not find
    on = dev.read_features()[1][..., 3].view(np.int32) == SPHERE
    assert (out[..., 3][on] != 0).mean() > 0.9


def test_two_updates_keep_the_first_ones_input(dev):
    scene, pa = scenes.config_headline(192, 108)
    v1, v2 = lifted(scene, SPHERE, 0.15), lifted(scene, SPHERE, LIFT)
    _sequence(dev, scene, pa, [v1, v2], {}, "two updates")
    # and the next move starts from v2: the planes inside the call were a feature pass
    dev.render(dict(pa, seed=host.frame_seed(50)))
    acc0, (n0, a0) = dev.read_accum(), dev.read_features()
    v3 = rmm.rotate_vertices(v2, -1.0)
    dev.update_vertices(v3)
    dev.reproject_motion(pa)
    ref, carried, hits = host.reproject_motion(acc0, n0, a0, dev.read_features_geom(), dev.read_features()[1], v2, scene["tri"], pa)
    _same(dev.read_accum(), ref, "a second move, from the first move's geometry")
    assert dev.reproject_last() == (carried, hits) and carried > 0.5 * hits


def test_no_update_at_all(dev):
    scene, pa = scenes.config_headline(192, 108)
    out, carried, hits, _ = _sequence(dev, scene, pa, [], {}, "no update")
    assert carried == hits


def test_update_from_a_device_tensor(dev):
    scene, pa = scenes.config_headline(192, 108)
    _sequence(dev, scene, pa, [lifted(scene, SPHERE, LIFT)], {}, "torch tensor", tensor=True)


def test_half_buffer_is_zeroed_and_the_accumulators_alternate(dev):
    scene, pa = scenes.config_c1(64, 48, max_depth=4, subdiv=1)
    v1 = _verts(scene).copy()
    v1[:, 1] += np.float32(0.05)
    _, _, _, ptr0 = _sequence(dev, scene, pa, [v1], {}, "adaptive", adaptive=True)
    ptr1 = _accum_ptr(dev)
    dev.update_vertices(_verts(scene))
    dev.reproject_motion(pa)
    assert _accum_ptr(dev) == ptr0 != ptr1


def test_camera_and_geometry_move_together(dev):
    scene, pa = scenes.config_headline(192, 108)
    pb = rm.move_camera(pa, "orbit", 2.0)
    v1 = lifted(scene, SPHERE, LIFT)
    _setup(dev, scene, pa)
    dev.render_features(pa)
    for sd in _seeds(3):
        dev.render(dict(pa, seed=sd))
    acc0, (n0, a0) = dev.read_accum(), dev.read_features()
    dev.update_vertices(v1)
    dev.reproject_motion(pb)
    rn, ra, rg = host.render_features_geom(moved_scene(scene, v1), pb)
    ref, carried, hits = host.reproject_motion(acc0, n0, a0, rg, ra, _verts(scene), scene["tri"], pa)
    _same(dev.read_accum(), ref, "camera and geometry")
    assert dev.reproject_last() == (carried, hits) and carried > 0.8 * hits


# ---- 7. refusals
def test_refusals_change_nothing():
    import torch
    scene, pa = scenes.config_c1(64, 40, max_depth=4, subdiv=1)

    def refused(d, what, needle):
        with pytest.raises(device.GlrtxError) as e:
            d.reproject_motion(pa)
        assert e.value.code == -1, what
        assert needle in str(e.value), (what, str(e.value))

    d = device.Device()
    try:
        d.upload_scene(scene); d.resize(64, 40)
        for sd in _seeds(2):
            d.render(dict(pa, seed=sd))
        d.render_features(pa)
        acc0, (n0, a0), ptr0 = d.read_accum(), d.read_features(), _accum_ptr(d)
        g0 = [None]

        def unchanged(what):
            assert np.array_equal(_bits(d.read_accum()), _bits(acc0)) and _accum_ptr(d) == ptr0, what
            n, a = d.read_features()
            assert np.array_equal(_bits(n), _bits(n0)) and np.array_equal(_bits(a), _bits(a0)), what
            if g0[0] is not None:
                assert np.array_equal(_bits(d.read_features_geom()), _bits(g0[0])), what

        refused(d, "tracking off", "tracking")
        unchanged("tracking off")
        d.track_motion(True)
        refused(d, "no geometry plane yet", "geometry plane")
        unchanged("no geometry plane")
        with pytest.raises(device.GlrtxError):
            d.read_features_geom()
        d.render_features(pa)
        g0[0] = d.read_features_geom()
        d.upload_scene(scene)
        refused(d, "after an upload", "previous geometry")
        unchanged("after an upload")
        d.render_features(pa)
        t = torch.zeros((40, 64, 4), dtype=torch.float32, device="cuda")
        d.bind_accum(t.data_ptr(), 64 * 16, 40)
        try:
            for sd in _seeds(2):  # (binding resized: frames and planes again, into the bound tensor)
                d.render(dict(pa, seed=sd))
            d.render_features(pa)
            acc_b, (n_b, a_b), g_b, ptr_b, t_b = d.read_accum(), d.read_features(), d.read_features_geom(), _accum_ptr(d), t.clone()
            assert ptr_b[0] == t.data_ptr() and acc_b[..., 3].max() == 2
            refused(d, "bound accumulator", "bound")
            assert torch.equal(t.view(torch.int32), t_b.view(torch.int32)) and np.array_equal(_bits(d.read_accum()), _bits(acc_b)) and _accum_ptr(d) == ptr_b
            n, a = d.read_features()
            assert np.array_equal(_bits(n), _bits(n_b)) and np.array_equal(_bits(a), _bits(a_b)) and np.array_equal(_bits(d.read_features_geom()), _bits(g_b))
        finally:
            d.bind_accum(0, 0, 0)  # (unbinding resizes: the planes go)
        for sd in _seeds(2):
            d.render(dict(pa, seed=sd))
        d.render_features(pa)
        d.resize(64, 40)  # a resize to the same size: the accumulator is cleared, the planes and the counts are released

        def no_planes():
            for read in (d.read_features, d.read_features_geom, d.reproject_last):
                with pytest.raises(device.GlrtxError):
                    read()

        acc_r, ptr_r = d.read_accum(), _accum_ptr(d)
        no_planes()
        refused(d, "after the resize", "feature")
        assert np.array_equal(_bits(d.read_accum()), _bits(acc_r)) and _accum_ptr(d) == ptr_r
        no_planes()
        d.set_partition(1, 2, 8)
        d.render_features(pa)
        acc_p, (n_p, a_p), g_p = d.read_accum(), d.read_features(), d.read_features_geom()
        refused(d, "partitioned", "partition")
        assert np.array_equal(_bits(d.read_accum()), _bits(acc_p)) and np.array_equal(_bits(d.read_features_geom()), _bits(g_p))
        assert np.array_equal(_bits(d.read_features()[0]), _bits(n_p)) and np.array_equal(_bits(d.read_features()[1]), _bits(a_p))
        d.set_partition(0, 1, 16)
        d.render_features(pa)
        for sd in _seeds(2):
            d.render(dict(pa, seed=sd))
        d.reproject_motion(pa)  # and with everything in place it goes through
        assert d.reproject_last()[0] > 0
        assert d.L.glrtx_reproject_motion(d.h, None, C.byref(device.ReprojectCfg.default())) == -1
        assert d.L.glrtx_track_motion(None, 1) == -1 and d.L.glrtx_read_features_geom(d.h, None, 0) == -1
    finally:
        d.close()


# ---- 8. nothing else moved
def test_tracking_changes_no_other_result(gpu_device):
    from oracle import pt_oracle
    scene, pa = scenes.config_c1(128, 96, max_depth=4, subdiv=1)
    pb = rm.move_camera(pa, "orbit", 3.0)
    v1 = _verts(scene).copy()
    v1[:, 0] += np.float32(0.1)
    results = []
    for track in (False, True):
        d = device.Device()
        try:
            _setup(d, scene, pa, track)
            for sd in _seeds(3):
                d.render(dict(pa, seed=sd))
            acc = d.read_accum()
            d.render_features(pa)
            d.denoise()
            den = d.read_denoised()
            d.reproject(pb)
            rep, counts = d.read_accum(), d.reproject_last()
            d.update_vertices(v1)
            blobs = [d.read_scene(k) for k in device.SCENE_BUFFERS]
            d.clear()
            d.render(dict(pb, seed=host.frame_seed(7)))
            results.append((acc, den, rep, counts, blobs, d.read_accum()))
        finally:
            d.close()
    off, on = results
    ref = None
    for sd in _seeds(3):
        ref, _ = pt_oracle.render(scene, dict(pa, seed=sd), accum=ref)
    _same(on[0], ref, "render with tracking on against the oracle")
    _same(on[0], off[0], "render"); _same(on[1], off[1], "denoise"); _same(on[2], off[2], "reproject")
    assert on[3] == off[3]
    for k, (a, b) in enumerate(zip(on[4], off[4])):
        assert np.array_equal(np.asarray(a).view(np.uint8), np.asarray(b).view(np.uint8)), f"scene buffer {k} after update_vertices"
    _same(on[5], off[5], "render after update_vertices")
    moved, _ = pt_oracle.render(moved_scene(scene, v1), dict(pb, seed=host.frame_seed(7)))
    _same(on[5], moved, "render after update_vertices against the oracle")
