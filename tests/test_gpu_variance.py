"""Variance guidance on the GPU (csrc/variance.hip.h, denoise_atrous_var in csrc/denoise.hip.h), all bit for bit against the CPU statements (host/variance.cpp):
the variance pass and the filter on hostile arrays; glrtx_render_moments' accumulator is glrtx_render_frames' and its M is glrt_fold_moments of the frames; the
filter after real renders, on the spatial and on the temporal branch; M carried through both reprojections, and the filter on the image that then mixes the
branches; what the calls leave alone; M's lifecycle; the refusals."""
import numpy as np
import pytest

import variance_math as vm
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    bad = _bits(got) != _bits(ref)
    if bad.ndim == 3:
        bad = bad.any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])].tolist()} vs {ref[tuple(np.argwhere(bad)[0])].tolist()}"


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, track=True, count=False):
    d.set_variant(2); d.count_rays(count)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()
    d.track_moments(track)


# ---- 1. the kernels on hostile arrays: (16, 16) and (17, 33) put pixels on both sides of a tile edge for the 3-pixel and the 2 * 2^i halos; (1, 1) has no neighbour
@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (17, 33), (5, 130), (1, 1), (70, 49)])
def test_debug_denoise_variance_on_hostile_arrays(gpu_device, rows, width):
    acc, M, N, A = vm.hostile_arrays(rows, width, rows * 1000 + width)
    for iterations in range(1, 7):
        for demodulate in (0, 1):
            for sl in (0.5, 4.0):
                got, v0 = device.debug_denoise_variance(acc, M, N, A, return_v0=True, iterations=iterations, sigma_lum=sl, sigma_normal=0.1, sigma_depth=0.01,
                                                        demodulate=demodulate)
                ref, rv = host.denoise_variance(acc, M, N, A, iterations, sl, 0.1, 0.01, demodulate, return_v0=True)
                _same(v0, rv, f"V0 {width}x{rows} it={iterations} demod={demodulate} sl={sl}")
                _same(got, ref, f"D {width}x{rows} it={iterations} demod={demodulate} sl={sl}")
    got = device.debug_denoise_variance(acc, M, N, A, iterations=6, sigma_lum=1e-38, sigma_normal=1e-30, sigma_depth=1e-30, demodulate=1)
    _same(got, host.denoise_variance(acc, M, N, A, 6, 1e-38, 1e-30, 1e-30, 1), "tiny sigmas")


# ---- 2. render_moments
def test_accumulator_parity_and_the_fold(dev, gpu_device):
    scene, params = scenes.config_c1(64, 48, max_depth=4, subdiv=1)
    seeds = _seeds(8)
    _setup(dev, scene, params)
    dev.render_moments(params, seeds[:5]); dev.render_moments(params, seeds[5:])
    acc, M = dev.read_accum(), dev.read_moments()
    _setup(gpu_device, scene, params, track=False)
    gpu_device.render_frames(params, seeds)
    _same(acc, gpu_device.read_accum(), "render_moments' accumulator against render_frames'")
    frames = []
    for sd in seeds:
        gpu_device.clear(); gpu_device.render(dict(params, seed=sd))
        frames.append(gpu_device.read_accum())
    assert all((f[..., 3] == 1).all() for f in frames)
    _same(M, host.fold_moments(np.zeros_like(acc), np.stack(frames)), "M against glrt_fold_moments of the eight frames")
    assert (M[..., 3] == 8).all() and not M[..., 2].any()


# ---- 3. the filter after real renders
def _render_and_denoise(d, scene, params, frames, what, cfgs):
    from oracle import pt_oracle
    _setup(d, scene, params, count=True)
    d.render_moments(params, _seeds(frames))
    d.render_adaptive(params, _seeds(2, 100), -1.0, 2)  # (a half buffer to watch; these two samples M does not see)
    d.render_features(params)
    acc0, M0, half0, rays0 = d.read_accum(), d.read_moments(), d.read_adaptive_half(), d.stats().rays
    assert (M0[..., 3] == frames).all() and (acc0[..., 3] == frames + 2).all()
    n, a = d.read_features()
    for cfg in cfgs:
        d.denoise_variance(**cfg)
        D = d.read_denoised()
        k = device.denoise_var_cfg(**cfg)
        _same(D, host.denoise_variance(acc0, M0, n, a, k.iterations, k.sigma_lum, k.sigma_normal, k.sigma_depth, k.demodulate), f"{what} {cfg}")
        for flip in (True, False):
            assert np.array_equal(d.resolve_denoised_rgba8(2.2, flip), pt_oracle.resolve(D, 2.2, flip)), f"{what}: resolve of D, flip {flip}"
    assert np.array_equal(_bits(d.read_accum()), _bits(acc0)) and np.array_equal(_bits(d.read_moments()), _bits(M0)), f"{what}: the accumulator or M moved"
    assert np.array_equal(_bits(d.read_adaptive_half()), _bits(half0)) and d.stats().rays == rays0, f"{what}: the half buffer or the ray count moved"


def test_spatial_branch_after_one_frame(dev):
    scene, params = scenes.config_c1(100, 75, max_depth=4, subdiv=1)
    _render_and_denoise(dev, scene, params, 1, "c1 100x75, 1 frame", [dict(), dict(iterations=2, sigma_lum=1.0, demodulate=0), dict(iterations=6, sigma_lum=16.0)])


def test_temporal_branch_after_six_frames(dev):
    scene, params = scenes.config_c2(61, 37)
    _render_and_denoise(dev, scene, params, 6, "c2 61x37, 6 frames", [dict(), dict(iterations=3, sigma_lum=0.5, sigma_normal=0.5, demodulate=0)])


# ---- 4. M through the two reprojections
def _orbit(params, deg):
    import reproject_math as rm
    return rm.move_camera(params, "orbit", deg)


@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (1, 1)])
def test_debug_reproject_moments_on_hostile_arrays(gpu_device, rows, width):
    import reproject_math as rm
    import reproject_motion_math as rmm
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, n1, a1 = rm.hostile_arrays(rows, width, rows * 1000 + width)
    M = vm.hostile_moments(acc, rows + width)
    cfgs = [dict(), dict(max_history=3, depth_tolerance=0.5, normal_tolerance=-1.0), dict(max_history=1000, depth_tolerance=1e3, normal_tolerance=-2.0)]
    for cur in (params, _orbit(params, 2.0)):
        for cfg in cfgs:
            out, mo, carried, hits = device.debug_reproject_moments(acc, M, n0, a0, n1, a1, params, cur, **cfg)
            ref, rmo, c2, h2 = host.reproject_moments(acc, M, n0, a0, n1, a1, params, cur, **cfg)
            _same(mo, rmo, f"M {width}x{rows} {cfg}"); _same(out, ref, f"accumulator {width}x{rows} {cfg}")
            assert (carried, hits) == (c2, h2)
            _same(device.debug_reproject(acc, n0, a0, n1, a1, params, cur, **cfg)[0], ref, "the plain debug entry")
    acc, n0, a0, g1, a1, vert, tri = rmm.hostile_arrays(rows, width, rows * 1000 + width)
    for prev in (params, _orbit(params, 2.0)):
        for cfg in cfgs:
            out, mo, carried, hits = device.debug_reproject_motion_moments(acc, M, n0, a0, g1, a1, vert, tri, prev, **cfg)
            ref, rmo, c2, h2 = host.reproject_motion_moments(acc, M, n0, a0, g1, a1, vert, tri, prev, **cfg)
            _same(mo, rmo, f"motion M {width}x{rows} {cfg}"); _same(out, ref, f"motion accumulator {width}x{rows} {cfg}")
            assert (carried, hits) == (c2, h2)


def _move_and_check(dev, other, scene, params, cur, motion, moved=None):
    """6 frames with render_moments, features, [a vertex update,] the reprojection to `cur`: the new M equals the CPU statement, the accumulator and the counts
    equal a context's with tracking off; then one more frame and denoise_variance on an image that mixes M.w = 7 and M.w = 1."""
    seeds = _seeds(6)
    for d, track in ((dev, True), (other, False)):
        _setup(d, scene, params, track=track)
        d.track_motion(motion)
    dev.render_moments(params, seeds); other.render_frames(params, seeds)
    for d in (dev, other):
        d.render_features(params)
    acc0, M0 = dev.read_accum(), dev.read_moments()
    n0, a0 = dev.read_features()
    for d in (dev, other):
        if motion:
            d.update_vertices(moved)
            d.reproject_motion(cur)
        else:
            d.reproject(cur)
    acc, M = dev.read_accum(), dev.read_moments()
    _same(acc, other.read_accum(), "the reprojected accumulator with tracking on against tracking off")
    assert dev.reproject_last() == other.reproject_last()
    n1, a1 = dev.read_features()
    if motion:
        g1 = dev.read_features_geom()
        ref, rmo, carried, hits = host.reproject_motion_moments(acc0, M0, n0, a0, g1, a1, scene["vert"], scene["tri"], params)
    else:
        ref, rmo, carried, hits = host.reproject_moments(acc0, M0, n0, a0, n1, a1, params, cur)
    _same(M, rmo, "the carried M against the CPU statement"); _same(acc, ref, "the accumulator against the CPU statement")
    assert dev.reproject_last() == (carried, hits) and (M[..., 3] == 6).any()
    dev.render_moments(cur, _seeds(1, 6))
    acc, M = dev.read_accum(), dev.read_moments()
    assert (M[..., 3] == 7).any() and (M[..., 3] == 1).any()  # both branches of the variance pass in one image
    n, a = dev.read_features()
    dev.denoise_variance()
    _same(dev.read_denoised(), host.denoise_variance(acc, M, n, a), "D after the move and one new frame")
    for d in (dev, other):
        d.track_motion(False)


def test_camera_move_carries_m(dev, gpu_device):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    _move_and_check(dev, gpu_device, scene, params, _orbit(params, 3.0), False)


def test_geometry_move_carries_m(dev, gpu_device):
    import reproject_motion_math as rmm
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    vert = np.array(np.asarray(scene["vert"], np.float32).reshape(-1, 15), copy=True)
    tri = np.asarray(scene["tri"], np.float32).reshape(-1, 4)
    idx = max((rmm.vertices_of_material(scene, m) for m in (1, 2)), key=len)  # one of the two objects on the floor
    vert[idx, 1] += np.float32(0.3)  # one mesh lifted
    _move_and_check(dev, gpu_device, scene, params, params, True, moved=vert)


# ---- 5. with tracking off nothing changes
def test_with_tracking_off_reproject_and_denoise_are_what_they_were(gpu_device):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    cur = _orbit(params, 3.0)
    _setup(gpu_device, scene, params, track=False)
    gpu_device.render_frames(params, _seeds(4))
    gpu_device.render_features(params)
    acc0 = gpu_device.read_accum(); n0, a0 = gpu_device.read_features()
    gpu_device.denoise()
    _same(gpu_device.read_denoised(), host.denoise_atrous(acc0, n0, a0), "denoise")
    gpu_device.reproject(cur)
    n1, a1 = gpu_device.read_features()
    ref, carried, hits = host.reproject(acc0, n0, a0, n1, a1, params, cur)
    _same(gpu_device.read_accum(), ref, "reproject")
    assert gpu_device.reproject_last() == (carried, hits)


# ---- 6. M's lifecycle
def test_lifecycle_of_m(dev):
    scene, params = scenes.config_c1(40, 24, max_depth=4, subdiv=1)
    _setup(dev, scene, params)
    assert not dev.read_moments().any()  # first use: zeros
    dev.render_moments(params, _seeds(2))
    assert (dev.read_moments()[..., 3] == 2).all()
    dev.clear()
    assert not dev.read_moments().any() and not dev.read_accum().any()
    dev.render_moments(params, _seeds(1))
    dev.track_moments(False); dev.track_moments(True)
    assert not dev.read_moments().any() and (dev.read_accum()[..., 3] == 1).all()
    dev.render_moments(params, _seeds(1))
    dev.resize(24, 40)  # releases M: the next use allocates a plane of the new shape
    dev.render_features(dict(params, width=24, height=40))
    with pytest.raises(device.GlrtxError) as e:
        dev.denoise_variance()
    assert e.value.code == -1 and "moments" in str(e.value)
    assert dev.read_moments().shape == (40, 24, 4) and not dev.read_moments().any()


# ---- 7. refusals
def test_refusals():
    scene, params = scenes.config_c1(32, 32, max_depth=4, subdiv=1)
    d = device.Device()

    def refused(fn, *a, **k):
        with pytest.raises(device.GlrtxError) as e:
            fn(*a, **k)
        assert e.value.code == -1, str(e.value)
        return str(e.value)

    try:
        d.set_variant(2); d.upload_scene(scene); d.resize(32, 32)
        d.render_features(params)
        assert "track" in refused(d.render_moments, params, _seeds(1))  # tracking off
        assert "track" in refused(d.denoise_variance)
        refused(d.read_moments)
        assert not d.read_accum().any()
        d.track_moments(True)
        assert "moments" in refused(d.denoise_variance)  # no M yet
        d.resize(32, 32)
        d.render_moments(params, _seeds(1))
        assert "feature" in refused(d.denoise_variance)  # the resize took the planes
        d.render_features(params)
        d.denoise_variance(); d.read_denoised()
        for bad in (dict(iterations=0), dict(iterations=7), dict(sigma_lum=0.0), dict(sigma_lum=float("nan")), dict(sigma_depth=float("inf")),
                    dict(sigma_normal=0.0)):
            refused(d.denoise_variance, **bad)
        d.resize(40, 24)
        refused(d.denoise_variance)  # after a resize: neither planes nor M
        d.present_enable(2)
        assert "presentation" in refused(d.render_moments, params, _seeds(1))
        d.present_enable(0)
        d.set_variant(1)
        assert "variant" in refused(d.render_moments, params, _seeds(1))
        d.set_variant(2)
        d.upload_spheres(np.array([[0, 0, 0, 0.5, 0]], np.float32))
        assert "sphere" in refused(d.render_moments, params, _seeds(1))
    finally:
        d.close()


# ---- 8. glrt_main --denoise-variance
def test_glrt_main_denoise_variance_writes_the_bindings_image(tmp_path, dev):
    """tests/test_gpu_denoise.py's facade test with the new flag: the scene and frames of tests/test_gpu_adaptive.py, 96x64, 3 frames.  glrt_main
    --denoise-variance writes the binding's resolve of the variance-guided D (features before the first frame, render_moments, the default configuration or
    --denoise-iters), whatever the burst size; and it is refused with --adaptive, with --denoise, and with more frames in flight than a burst takes."""
    import subprocess
    from PIL import Image
    from conftest import PKG
    from test_gpu_adaptive import _c1_builder
    w, h, depth, frames = 96, 64, 4, 3
    b = _c1_builder()
    js = scenes.export_json_obj(b, tmp_path, w, h, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)
    exe = str(PKG / "lib" / "glrt_main")

    def glrt_main(extra, name, in_flight="1"):
        out = tmp_path / name
        r = subprocess.run([exe, "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--frames-in-flight", in_flight, "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.asarray(Image.open(out))

    b2 = scenes.SceneBuilder()
    for pos, nrm, mid in zip(b._pos, b._nrm, b._mid):
        b2.add_mesh(pos, nrm, b2.add_material(b.materials[int(mid[0])]))
    scene = b2.build()
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, w, h)
    params = dict(scenes.make_params(c2w, s2c, w, h, depth, 1), focal=0.0)  # (absent focalLength parses as 0)
    _setup(dev, scene, params)
    dev.render_features(params)
    dev.render_moments(params, _seeds(frames))
    plain = dev.resolve_rgba8(2.2, True)
    dev.denoise_variance()
    ref = dev.resolve_denoised_rgba8(2.2, True)
    for in_flight in ("1", "2", "16"):
        img = glrt_main(["--denoise-variance"], f"var{in_flight}.png", in_flight)
        assert np.array_equal(img, ref), (in_flight, int((img != ref).any(-1).sum()))
    assert not np.array_equal(ref, plain)
    dev.denoise()
    assert not np.array_equal(ref, dev.resolve_denoised_rgba8(2.2, True))  # (and it is not the fixed-sigma filter's image)
    dev.denoise_variance(iterations=2)
    # --denoise-iters is honoured.  The facade forms its camera matrices in C++ (the inverse of view x model), the binding takes scenes.camera's: the two agree
    # to the last ulp or so, not bit for bit, and an ulp in a feature plane can carry a resolved value across ONE 8-bit rounding step in an isolated pixel
    # (measured on the CPU statement: a 1-ulp camera change flips 0 or 1 of these 6144 pixels, in either filter).  So: at most 1 step, in at most 0.1 % of the pixels.
    it2, ref2 = glrt_main(["--denoise-variance", "--denoise-iters", "2"], "var_it2.png").astype(np.int32), dev.resolve_denoised_rgba8(2.2, True).astype(np.int32)
    assert np.abs(it2 - ref2).max() <= 1 and (it2 != ref2).any(-1).sum() <= 6 and not np.array_equal(it2, ref.astype(np.int32))
    for extra, word in ((["--denoise-variance", "--adaptive", "0.05"], "--adaptive"), (["--denoise-variance", "--denoise"], "--denoise"),
                        (["--denoise-variance", "--frames-in-flight", "1025"], "--frames-in-flight"), (["--denoise-variance", "--save-every-frame"], "--save-every-frame")):
        r = subprocess.run([exe, "-i", str(js)] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--denoise-variance" in r.stderr and word in r.stderr, (extra, r.stderr)
