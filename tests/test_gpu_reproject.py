"""Temporal reprojection on the GPU (csrc/reproject.hip.h): Device.reproject equals the CPU statement (glrt_reproject) on the read-back inputs bit for bit -- in
both node layouts, on a vine, at an odd size and at 1080p --, the kernel equals it on hostile arrays, the swapped accumulator is the one rendered into, a call
between two bursts of frames is ordered like synchronised calls and counts no rays, the adaptive half buffer is zeroed, a denoise straight after it uses the new
planes, and every refusal is GLRTX_EINVAL and changes nothing."""
import ctypes as C

import numpy as np
import pytest

import reproject_math as rm
from fuzz_scenes import CASES, case_scene_and_params
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

CFG2 = dict(max_history=2, depth_tolerance=0.2, normal_tolerance=-1.0)


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


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, count=False):
    d.set_variant(2); d.count_rays(count)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _render_reproject_compare(d, scene, pa, pb, frames, what, cfgs=({},)):
    """frames at camera A, the planes of A, a reprojection to B: accumulator, planes and counts against the CPU statement on what the device held before."""
    out = None
    for cfg in cfgs:
        _setup(d, scene, pa)
        for sd in _seeds(frames):
            d.render(dict(pa, seed=sd))
        d.render_features(pa)
        acc0 = d.read_accum()
        n0, a0 = d.read_features()
        ptr0 = _accum_ptr(d)
        d.reproject(pb, **cfg)
        out = d.read_accum()
        n1, a1 = d.read_features()
        carried, hits = d.reproject_last()
        ref, carried_ref, hits_ref = host.reproject(acc0, n0, a0, n1, a1, pa, pb, **cfg)
        _same(out, ref, f"{what} {cfg}")
        assert (carried, hits) == (carried_ref, hits_ref), (what, cfg, carried, hits, carried_ref, hits_ref)
        assert _accum_ptr(d)[0] != ptr0[0] and _accum_ptr(d)[1] == ptr0[1], f"{what}: the accumulators were not swapped"
    return out, n1, a1


def _both_layouts(d, monkeypatch, scene, pa, pb, frames, what, cfgs=({}, CFG2)):
    ref_n, ref_a = host.render_features(scene, pb)
    carried_any = 0
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        out, n1, a1 = _render_reproject_compare(d, scene, pa, pb, frames, f"{what} compact={compact}", cfgs)
        _same(n1, ref_n, f"{what} compact={compact}: new normal/depth plane")
        _same(a1, ref_a, f"{what} compact={compact}: new albedo/id plane")
        carried_any += int((out[..., 3] != 0).sum())
    monkeypatch.delenv("GLRTX_COMPACT_NODES")
    return carried_any


# ---- 1. the call against the CPU statement
@pytest.mark.parametrize("kind,amount", [("pan", 2.0), ("dolly", 0.5), ("orbit", 3.0), ("orbit", 0.0)])
def test_reproject_c1(dev, monkeypatch, kind, amount):
    scene, pa = scenes.config_c1(256, 256, max_depth=4, subdiv=2)
    assert _both_layouts(dev, monkeypatch, scene, pa, rm.move_camera(pa, kind, amount), 3, f"c1 {kind}") > 0.5 * 2 * 256 * 256 * 0.5


@pytest.mark.parametrize("case", [0, 1, 4, 5, 7, 10], ids=lambda c: f"fuzz{CASES[c][0]}-{CASES[c][2]}")
def test_reproject_fuzz(dev, monkeypatch, case):
    scene, pa = case_scene_and_params(CASES[case])
    for kind, amount in (("pan", 2.0), ("orbit", 3.0)):
        _both_layouts(dev, monkeypatch, scene, pa, rm.move_camera(pa, kind, amount), 2, f"case {CASES[case][0]} {kind}")


def test_reproject_vine(dev, monkeypatch):
    scene, pa = scenes.config_c3(96, 64, n=3000)
    _both_layouts(dev, monkeypatch, scene, pa, rm.move_camera(pa, "orbit", 2.0), 2, "c3 vine")
    scene, pa = case_scene_and_params(CASES[2])  # a chain tree of a fuzz scene
    _both_layouts(dev, monkeypatch, scene, pa, rm.move_camera(pa, "pan", 1.0), 2, "fuzz vine")


def test_reproject_odd_size(dev, monkeypatch):
    scene, pa = scenes.config_c2(61, 37)
    assert _both_layouts(dev, monkeypatch, scene, pa, rm.move_camera(pa, "orbit", 3.0), 2, "c2 61x37") > 0


def test_reproject_headline_1080p(dev):
    scene, pa = scenes.config_headline(1920, 1080)
    out, _, a1 = _render_reproject_compare(dev, scene, pa, rm.move_camera(pa, "orbit", 3.0), 1, "headline 1080p")
    assert (out[..., 3] != 0).sum() >= 0.8 * (a1[..., 3].view(np.int32) >= 0).sum()


def test_two_moves_in_a_row(dev):
    """The second call starts from the first call's camera, planes and accumulator (the buffers alternate)."""
    scene, pa = scenes.config_c1(128, 96, max_depth=4, subdiv=1)
    pb, pc = rm.move_camera(pa, "orbit", 2.0), rm.move_camera(pa, "orbit", 4.0)
    _render_reproject_compare(dev, scene, pa, pb, 3, "first move")
    ptr_b = _accum_ptr(dev)
    dev.render(dict(pb, seed=host.frame_seed(9)))
    acc_b = dev.read_accum()
    n_b, a_b = dev.read_features()
    dev.reproject(pc)
    n_c, a_c = dev.read_features()
    ref, carried, hits = host.reproject(acc_b, n_b, a_b, n_c, a_c, pb, pc)
    _same(dev.read_accum(), ref, "second move")
    assert dev.reproject_last() == (carried, hits) and carried > 0 and _accum_ptr(dev) != ptr_b


# ---- 2. the kernel on hostile arrays
@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (5, 130), (1, 1), (70, 49)])
def test_kernel_on_hostile_arrays(gpu_device, rows, width):
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, n1, a1 = rm.hostile_arrays(rows, width, rows * 1000 + width)
    cfgs = [{}, CFG2, dict(max_history=1000, depth_tolerance=1e3, normal_tolerance=-2.0), dict(max_history=1, depth_tolerance=1e-40, normal_tolerance=1e-40),
            dict(max_history=2 ** 31 - 1, depth_tolerance=3e38, normal_tolerance=-3e38)]
    cams = [(params, params), (params, rm.move_camera(params, "pan", 1.0)), (params, rm.move_camera(params, "dolly", 0.3)), (params, rm.move_camera(params, "orbit", 2.0)),
            (rm.move_camera(params, "pan", 180.0), params)]  # the last: the old camera looks away, s.w <= 0 everywhere
    for prev, cur in cams:
        for cfg in cfgs:
            got, carried, hits = device.debug_reproject(acc, n0, a0, n1, a1, prev, cur, **cfg)
            ref, carried_ref, hits_ref = host.reproject(acc, n0, a0, n1, a1, prev, cur, **cfg)
            _same(got, ref, f"{width}x{rows} {cfg}")
            assert (carried, hits) == (carried_ref, hits_ref)
    assert carried == 0 and not got.any()


# ---- 3. the swapped accumulator is the one rendered into
def test_frames_after_a_reproject_go_into_the_new_accumulator(dev):
    from oracle import pt_oracle
    scene, pa = scenes.config_c1(128, 96, max_depth=4, subdiv=1)
    pb = rm.move_camera(pa, "orbit", 3.0)
    out, _, _ = _render_reproject_compare(dev, scene, pa, pb, 4, "before the frames")
    for sd in _seeds(8, 100):
        dev.render(dict(pb, seed=sd))
    ref = out
    for sd in _seeds(8, 100):
        ref, _ = pt_oracle.render(scene, dict(pb, seed=sd), accum=ref)
    got = dev.read_accum()
    _same(got, ref, "8 frames after the reproject")
    assert got[..., 3].max() == 12 and got[..., 3].min() == 8


# ---- 4. ordering against bursts of frames, and the ray count
def test_between_two_fed_bursts(dev, gpu_device):
    """features, a burst at A, a reproject, a burst -- nothing synchronises in between.  The result is the CPU statement applied to the first burst's accumulator
    (rendered on a second context) with the oracle's frames of the second burst added, once for a moved and once for an unmoved camera (where only the seal keeps
    the second burst out of the first burst's launch); the ray count is that of the frames alone."""
    from oracle import pt_oracle
    scene, pa = scenes.config_c1(128, 96, max_depth=4, subdiv=1)
    seeds = _seeds(12)
    for pb in (rm.move_camera(pa, "orbit", 3.0), pa):
        _setup(dev, scene, pa, count=True); _setup(gpu_device, scene, pa)
        dev.read_accum()  # (a blocking copy: the counters' reset has landed before the first frame counts)
        dev.render_features(pa)
        for sd in seeds[:6]:
            dev.render(dict(pa, seed=sd)); gpu_device.render(dict(pa, seed=sd))
        dev.reproject(pb)
        for sd in seeds[6:]:
            dev.render(dict(pb, seed=sd))
        acc_a = gpu_device.read_accum()
        assert (acc_a[..., 3] == 6).all()
        n0, a0 = host.render_features(scene, pa)
        n1, a1 = host.render_features(scene, pb)
        ref, carried, hits = host.reproject(acc_a, n0, a0, n1, a1, pa, pb)
        rays = sum(pt_oracle.render(scene, dict(pa, seed=sd))[1] for sd in seeds[:6])
        for sd in seeds[6:]:
            ref, r = pt_oracle.render(scene, dict(pb, seed=sd), accum=ref)
            rays += r
        _same(dev.read_accum(), ref, "two bursts around a reproject")
        assert dev.reproject_last() == (carried, hits) and carried > 0
        st = dev.stats()
        assert st.rays == rays and st.launches == 12, (st.rays, rays, st.launches)


def test_the_call_counts_no_rays_and_leaves_the_denoised_image(dev):
    scene, pa = scenes.config_c1(64, 48, max_depth=4, subdiv=1)
    _setup(dev, scene, pa, count=True)
    for sd in _seeds(2):
        dev.render(dict(pa, seed=sd))
    dev.render_features(pa); dev.denoise()
    D0, st0 = dev.read_denoised(), dev.stats()
    dev.reproject(rm.move_camera(pa, "pan", 2.0)); dev.sync()
    st1 = dev.stats()
    assert (st1.rays, st1.launches, st1.paths) == (st0.rays, st0.launches, st0.paths)
    assert np.array_equal(_bits(dev.read_denoised()), _bits(D0))


# ---- 5. the adaptive half buffer
def test_half_buffer_is_zeroed_and_every_tile_is_active_again(dev):
    scene, pa = scenes.config_c1(64, 48, max_depth=4, subdiv=1)
    _setup(dev, scene, pa)
    dev.render_features(pa)
    dev.render_adaptive(pa, _seeds(4), -1.0, 2)
    assert dev.read_adaptive_half()[..., 3].max() == 2
    dev.render_adaptive(pa, [], 3e38, 2)
    assert dev.adaptive_active_tiles() == (0, 48)  # everything has retired under this threshold
    dev.reproject(rm.move_camera(pa, "orbit", 2.0))
    assert not dev.read_adaptive_half().any()
    assert dev.read_accum()[..., 3].max() == 4
    dev.render_adaptive(pa, [], 3e38, 2)
    assert dev.adaptive_active_tiles() == (48, 48)  # H.w = 0 everywhere


# ---- 6. denoise straight after reproject
def test_denoise_after_reproject_uses_the_new_planes(dev):
    scene, pa = scenes.config_c1(128, 96, max_depth=4, subdiv=1)
    pb = rm.move_camera(pa, "orbit", 3.0)
    out, n1, a1 = _render_reproject_compare(dev, scene, pa, pb, 3, "before the denoise")
    dev.denoise()
    k = device.denoise_cfg()
    _same(dev.read_denoised(), host.denoise_atrous(out, n1, a1, k.iterations, k.sigma_color, k.sigma_normal, k.sigma_depth, k.demodulate), "denoise after reproject")
    ref_n, ref_a = host.render_features(scene, pb)
    _same(n1, ref_n, "planes after reproject"); _same(a1, ref_a, "planes after reproject")


# ---- 7. refusals
def test_refusals_change_nothing(dev):
    import torch
    scene, pa = scenes.config_c1(64, 40, max_depth=4, subdiv=1)
    pb = rm.move_camera(pa, "orbit", 2.0)

    def refused(d, what, needle=None, **cfg):
        with pytest.raises(device.GlrtxError) as e:
            d.reproject(pb, **cfg)
        assert e.value.code == -1, what
        assert needle is None or needle in str(e.value), (what, str(e.value))

    d = device.Device()
    try:
        refused(d, "no scene", "scene")
        d.upload_scene(scene)
        refused(d, "no size", "size")
        d.resize(64, 40)
        refused(d, "no planes", "feature")
        with pytest.raises(device.GlrtxError):
            d.reproject_last()
        for sd in _seeds(2):
            d.render(dict(pa, seed=sd))
        d.render_features(pa)
        acc0, (n0, a0), ptr0 = d.read_accum(), d.read_features(), _accum_ptr(d)

        def unchanged(what):
            assert np.array_equal(_bits(d.read_accum()), _bits(acc0)) and _accum_ptr(d) == ptr0, what
            n, a = d.read_features()
            assert np.array_equal(_bits(n), _bits(n0)) and np.array_equal(_bits(a), _bits(a0)), what
            with pytest.raises(device.GlrtxError):
                d.reproject_last()

        for bad in (dict(max_history=0), dict(depth_tolerance=0.0), dict(depth_tolerance=float("inf")), dict(depth_tolerance=float("nan")), dict(normal_tolerance=float("nan")),
                    dict(normal_tolerance=float("inf"))):
            refused(d, str(bad), **bad)
        unchanged("bad cfgs")
        assert d.L.glrtx_reproject(d.h, None, C.byref(device.ReprojectCfg.default())) == -1 and d.L.glrtx_reproject(d.h, C.byref(device.make_params(pb)), None) == -1
        unchanged("NULL arguments")
        t = torch.zeros((40, 64, 4), dtype=torch.float32, device="cuda")
        d.bind_accum(t.data_ptr(), 64 * 16, 40)
        try:
            refused(d, "bound accumulator", "bound")
        finally:
            d.bind_accum(0, 0, 0)  # (unbinding resizes: the planes go)
        refused(d, "no planes after the resize", "feature")
        d.set_partition(1, 2, 8)
        d.render_features(pa)
        refused(d, "partitioned", "partition")
        d.set_partition(0, 1, 16)
        d.render_features(dict(pa, c2w=np.zeros(16, np.float32)))
        refused(d, "singular previous c2w", "singular")
        d.render_features(dict(pa, s2c=np.zeros(16, np.float32)))
        refused(d, "singular previous s2c", "singular")
        d.render_features(pa)
        for sd in _seeds(2):  # (the resizes above cleared the accumulator)
            d.render(dict(pa, seed=sd))
        d.reproject(pb)  # and with everything in place it goes through
        assert d.reproject_last()[0] > 0
        d.resize(48, 32)
        with pytest.raises(device.GlrtxError):
            d.reproject_last()  # the counts went with the old shape
        refused(d, "planes of the old shape", "feature")
        d.render_features(pa)
        d.upload_spheres(np.array([[0, 0, 0, 0.5, 0]], np.float32))
        refused(d, "spheres", "sphere")
    finally:
        d.close()
