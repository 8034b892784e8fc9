"""Adaptive sampling by variance on the GPU (glrtx_render_adaptive_moments; csrc/variance.hip.h: adaptive_moments::select_kernel, accumulate.hip.h: the
MomentsMasked sink).  The selection is pinned bit for bit against its numpy statement (tests/adaptive_moments_math.py), the rendered pixels and M against the
oracle's full frames, and the rest of the call against glrtx_render_moments on a second context: nothing retiring, everything retiring, H left alone, the
selection after both reprojections (what the call is for), the refusals, an unsynchronised train, and glrt_main --adaptive-variance."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import adaptive_math as am
import adaptive_moments_cases as cases
import adaptive_moments_math as amm
import variance_math as vm
from conftest import PKG, assert_bit_equal
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu
INF = float("inf")


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


@pytest.fixture(scope="module")
def devices(gpu_device):
    """Two contexts of this module's own, closed at its end; gpu_device first: torch's runtime is set up before libglrtx's."""
    ds = (device.Device(), device.Device())
    yield ds
    for d in ds:
        d.close()


def _setup(d, scene, params, track=True, count=False):
    d.set_variant(2); d.count_rays(count)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()
    d.track_moments(track)


# ---- 1. the selection kernels against the numpy statement
@pytest.mark.parametrize("size", cases.SIZES, ids=[f"{w}x{h}" for w, h in cases.SIZES])
def test_selection_matches_the_numpy_statement(gpu_device, size):
    planes = [p for p in cases.planes() if p[0].startswith(f"{size[0]}x{size[1]}-")]
    planes.append(("zeros", np.zeros((size[1], size[0], 4), np.float32)))
    assert len(planes) >= 3
    for what, M in planes:
        e_np = amm.tile_error(M)
        for thr in cases.thresholds(e_np):
            for ms in (2, cases.MIN_SAMPLES):
                mask, err, lst = device.adaptive_select_moments(M, thr, ms)
                m_ref, e_ref, l_ref = amm.select(M, thr, ms)
                assert np.array_equal(mask, m_ref), (what, thr, ms, int((mask != m_ref).sum()))
                assert np.array_equal(err.view(np.uint32), e_ref.view(np.uint32)), (what, thr, ms, np.argwhere(err.view(np.uint32) != e_ref.view(np.uint32))[:4])
                assert np.array_equal(lst, l_ref) and np.all(np.diff(lst) > 0), (what, thr, ms)
        assert device.adaptive_select_moments(M, -1.0, 2)[0].all()
    assert device.adaptive_select_moments(planes[-1][1], INF, 2)[0].all()  # (an M of zeros: every tile is active at any threshold)


# ---- 2. parity with the oracle's full frames
def oracle_chain(cfg, w, h, first=4, calls=(1, 3, 2), min_samples=2):
    """What the device must hold after `first` frames of render_moments and then the adaptive calls, from the oracle's frames and the numpy statements alone (no
    GPU): [(seeds, threshold, mask, acc, M)] per call, the first entry (threshold None) for render_moments.  The threshold is the median of the positive tile errors after
    the first frames: some tiles retire, some do not."""
    from oracle import pt_oracle
    scene, params = scenes.CONFIGS[cfg](width=w, height=h, n_samples=1)

    def frames(seeds):
        s = np.stack([pt_oracle.render(scene, dict(params, seed=sd))[0] for sd in seeds])
        assert np.all(s[..., 3] == 1)
        return s

    everything = np.ones(am.tiles_of(h, w), np.uint8)
    acc, M = amm.accumulate(np.zeros((h, w, 4), np.float32), np.zeros((h, w, 4), np.float32), frames(_seeds(first)), everything)
    steps = [(_seeds(first), None, everything, acc, M)]
    e = amm.tile_error(M)
    thr = float(np.median(e[e > 0]))  # (tiles that see no light at all have E = 0 and retire at any threshold)
    f0 = first
    for n in calls:
        mask = amm.select(M, thr, min_samples)[0]
        acc, M = amm.accumulate(acc, M, frames(_seeds(n, f0)), mask)
        steps.append((_seeds(n, f0), thr, mask, acc, M))
        f0 += n
    return scene, params, steps


@pytest.mark.parametrize("cfg,w,h", [("c1", 64, 48), ("c2", 50, 38)])
def test_adaptive_calls_equal_the_oracles_frames_on_active_tiles(gpu_device, cfg, w, h):
    scene, params, steps = oracle_chain(cfg, w, h)
    d = gpu_device
    _setup(d, scene, params)
    for k, (seeds, thr, mask, acc, M) in enumerate(steps):
        before_acc, before_M = d.read_accum(), d.read_moments()
        if thr is None:
            d.render_moments(params, seeds)
        else:
            assert 0 < int(mask.sum()) < mask.size, (k, int(mask.sum()), mask.size)
            d.render_adaptive_moments(params, seeds, thr, 2)
            assert d.adaptive_active_tiles() == (int(mask.sum()), mask.size), k
            assert np.array_equal(d.tile_mask(), mask), k
            off = ~am.expand_mask(mask, h, w)
            assert_bit_equal(d.read_accum()[off], before_acc[off], f"{cfg} accumulator of inactive tiles, call {k}")
            assert_bit_equal(d.read_moments()[off], before_M[off], f"{cfg} M of inactive tiles, call {k}")
        assert_bit_equal(d.read_accum(), acc, f"{cfg} accumulator after call {k}")
        assert_bit_equal(d.read_moments(), M, f"{cfg} M after call {k}")
    assert d.stats().device_error_pending == 0


# ---- 3. nothing retires: glrtx_render_moments bit for bit
def _nothing_retires(d, d2, scene, params, calls):
    _setup(d, scene, params, count=True); _setup(d2, scene, params, count=True)
    f0 = 0
    for n in calls:
        d.render_adaptive_moments(params, _seeds(n, f0), -1.0, 2)
        d2.render_moments(params, _seeds(n, f0))
        f0 += n
    d.sync(); d2.sync()  # (before anything is read: the ray counters are final once the device is idle)
    active, total = d.adaptive_active_tiles()
    assert active == total and d.tile_mask().all()
    assert_bit_equal(d.read_accum(), d2.read_accum(), "adaptive by variance (threshold -1) vs render_moments: accumulator")
    assert_bit_equal(d.read_moments(), d2.read_moments(), "adaptive by variance (threshold -1) vs render_moments: M")
    assert (d.read_moments()[..., 3] == f0).all()
    assert d.stats().rays == d2.stats().rays > 0
    d.count_rays(False); d2.count_rays(False)


def test_nothing_retires_equals_render_moments_headline(devices):
    scene, params = scenes.CONFIGS["headline"](width=200, height=108)
    _nothing_retires(*devices, scene, params, [1, 3, 2])


def test_nothing_retires_equals_render_moments_vine_tree(devices):
    scene, params = scenes.config_c3(width=96, height=72, n=2000)
    _nothing_retires(*devices, scene, params, [2, 1, 3])


# ---- 4. everything retires
def test_everything_retired_leaves_both_buffers_and_the_ray_count_alone(gpu_device):
    scene, params = scenes.config_c1(width=72, height=40, max_depth=2)
    d = gpu_device
    _setup(d, scene, params, count=True)
    d.render_moments(params, _seeds(3))
    d.sync()  # (glrtx_sync collects the ray counters)
    acc, M, rays = d.read_accum(), d.read_moments(), d.stats().rays
    assert rays > 0
    for n in (1, 5):
        d.render_adaptive_moments(params, _seeds(n, 3), INF, 2)  # (every count is 3 >= 2 and no E is a NaN: nothing is active)
        assert d.adaptive_active_tiles() == (0, 45)
        assert not d.tile_mask().any()
        assert_bit_equal(d.read_accum(), acc, "accumulator under an all-retired call")
        assert_bit_equal(d.read_moments(), M, "M under an all-retired call")
        d.sync()
        assert d.stats().rays == rays
    assert d.stats().device_error_pending == 0
    d.render_moments(params, _seeds(1, 9))  # the context goes on working
    assert np.all(d.read_accum()[..., 3] == 4) and np.all(d.read_moments()[..., 3] == 4)
    d.count_rays(False)


# ---- 5. H is never created or written
def test_the_half_buffer_is_neither_created_nor_written():
    scene, params = scenes.config_c1(width=40, height=24, max_depth=2)
    d = device.Device()  # (a context that never had a half buffer)
    try:
        _setup(d, scene, params)
        d.render_moments(params, _seeds(2))
        d.render_adaptive_moments(params, _seeds(2, 2), -1.0, 2)
        d.render_adaptive_moments(params, _seeds(1, 4), 0.05, 2)
        d.clear()
        d.render_adaptive_moments(params, _seeds(2), 0.05, 2)
        with pytest.raises(device.GlrtxError) as e:
            d.read_adaptive_half()
        assert e.value.code == device.GLRTX_EINVAL and "no half buffer" in str(e.value)
        d.render_adaptive(params, _seeds(3, 2), -1.0, 2)  # the H form: now there is one
        half = d.read_adaptive_half()
        assert half[..., 3].max() == 1
        acc = d.read_accum()
        d.render_adaptive_moments(params, _seeds(2, 5), -1.0, 2)
        assert (d.read_accum()[..., 3] == acc[..., 3] + 2).all()
        assert_bit_equal(d.read_adaptive_half(), half, "H under the M form")
    finally:
        d.close()


# ---- 6. what the call is for: after a move the H form renders everything again, the M form the disoccluded and the noisy tiles
def _after_the_move(d, cur, min_samples=4):
    d.render_adaptive(cur, [], 3e38, 2)  # n_frames = 0: selects only.  Both reprojections zero H: every tile is active, at any threshold
    active, total = d.adaptive_active_tiles()
    assert active == total > 0
    acc, M = d.read_accum(), d.read_moments()
    d.render_adaptive_moments(cur, [], INF, min_samples)
    active, total_m = d.adaptive_active_tiles()
    assert total_m == total and 0 < active < total, (active, total)
    mask = d.tile_mask()
    assert np.array_equal(mask, amm.select(M, INF, min_samples)[0])
    with np.errstate(invalid="ignore"):
        short = am.to_tiles(~(M[..., 3] >= min_samples), False).any(-1)
    assert short.any() and mask[short].all()  # every tile holding a pixel whose carried count is below min_samples (the disoccluded ones: no moments) is active
    assert_bit_equal(d.read_accum(), acc, "a selection alone changes nothing"); assert_bit_equal(d.read_moments(), M, "a selection alone changes nothing")
    return mask, M


def test_after_a_camera_move_only_some_tiles_are_active(devices):
    import reproject_math as rm
    scene, params = scenes.CONFIGS["headline"](width=96, height=54)
    d = devices[0]
    _setup(d, scene, params)
    d.render_moments(params, _seeds(8))
    d.render_features(params)
    cur = rm.move_camera(params, "orbit", 3.0)
    d.reproject(cur)
    mask, M = _after_the_move(d, cur)
    # ... and the frames that follow go to those tiles only
    d.render_adaptive_moments(cur, _seeds(2, 8), INF, 4)
    on = am.expand_mask(mask, 54, 96)
    M2 = d.read_moments()
    assert (M2[on][:, 3] == M[on][:, 3] + 2).all()
    assert_bit_equal(M2[~on], M[~on], "M of inactive tiles")


def test_after_a_geometry_move_only_some_tiles_are_active(devices):
    import reproject_motion_math as rmm
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    vert = np.array(np.asarray(scene["vert"], np.float32).reshape(-1, 15), copy=True)
    idx = max((rmm.vertices_of_material(scene, m) for m in (1, 2)), key=len)  # one of the two objects on the floor
    vert[idx, 1] += np.float32(0.3)  # one mesh lifted
    d = devices[0]
    _setup(d, scene, params)
    d.track_motion(True)
    try:
        d.render_moments(params, _seeds(8))
        d.render_features(params)
        d.update_vertices(vert)
        d.reproject_motion(params)
        _after_the_move(d, params)
    finally:
        d.track_motion(False)


# ---- 7. refusals
def test_refusals_change_nothing(gpu_device):
    scene, params = scenes.config_c1(width=40, height=24, max_depth=2)
    d = gpu_device
    _setup(d, scene, params)
    d.render_moments(params, _seeds(2))
    d.render_adaptive_moments(params, _seeds(1, 2), -1.0, 2)
    acc, M, counts = d.read_accum(), d.read_moments(), d.adaptive_active_tiles()

    def refused(fn, undo=None, word=None):
        with pytest.raises(device.GlrtxError) as ei:
            fn()
        assert ei.value.code == device.GLRTX_EINVAL, str(ei.value)
        assert "glrtx_render_adaptive_moments" in str(ei.value) and (word is None or word in str(ei.value)), str(ei.value)
        if undo:
            undo()
        assert_bit_equal(d.read_accum(), acc, "accumulator after a refused call")
        assert_bit_equal(d.read_moments(), M, "M after a refused call")
        assert d.adaptive_active_tiles() == counts

    call = lambda p=params, ms=2: d.render_adaptive_moments(p, _seeds(2, 3), 0.01, ms)  # noqa: E731
    refused(lambda: call(ms=1), word="min_samples")
    refused(lambda: call(ms=0), word="min_samples")
    d.present_enable(2)
    refused(call, lambda: d.present_enable(0), "presentation")
    d.set_extensions(device.EXT_DIELECTRIC)
    refused(call, lambda: d.set_extensions(0), "extensions")
    d.set_extensions(device.EXT_VOLUME)
    refused(call, lambda: d.set_extensions(0), "volume")
    d.upload_spheres([[0.0, 1.0, 0.0, 0.5, 0.0]])
    refused(call, lambda: d.upload_spheres(None), "sphere")
    d.set_variant(1)
    refused(call, lambda: d.set_variant(2), "variant")
    refused(lambda: call(p=dict(params, max_depth=256)))
    # NULL arguments, through the C ABI itself
    p, sd, cfg = device._adaptive_args(params, _seeds(2, 3), 0.01, 2)
    fp = sd.ctypes.data_as(C.POINTER(C.c_float))
    L = d.L
    for args in ((None, fp, 2, C.byref(cfg)), (C.byref(p), fp, 2, None), (C.byref(p), None, 2, C.byref(cfg)), (C.byref(p), fp, -1, C.byref(cfg))):
        refused(lambda a=args: d._ck(L.glrtx_render_adaptive_moments(d.h, *a)))
    assert L.glrtx_render_adaptive_moments(None, C.byref(p), fp, 2, C.byref(cfg)) == device.GLRTX_EINVAL
    # tracking off (switching it off releases M: last, and M is a plane of zeros afterwards)
    d.track_moments(False)
    with pytest.raises(device.GlrtxError) as ei:
        call()
    assert ei.value.code == device.GLRTX_EINVAL and "track" in str(ei.value)
    assert_bit_equal(d.read_accum(), acc, "accumulator after the call with tracking off")
    assert d.adaptive_active_tiles() == counts
    d.track_moments(True)
    d.render_adaptive_moments(params, _seeds(1, 3), INF, 2)  # and the context still renders: M is new, so every tile is active
    assert np.all(d.read_accum()[..., 3] == 4) and np.all(d.read_moments()[..., 3] == 1)


# ---- 8. an unsynchronised train
def test_unsynchronised_train_equals_the_synchronised_one(devices):
    scene, params = scenes.config_c2(width=160, height=96)
    s = _seeds(9)
    out = []
    for d, sync in zip(devices, (False, True)):
        _setup(d, scene, params)
        d.render_features(params)
        d.render_moments(params, s[0:4])
        d.sync()
        thr = float(np.median(amm.tile_error(d.read_moments())))
        step = d.sync if sync else (lambda: None)
        d.render_adaptive_moments(params, s[4:9], thr, 2); step()
        d.denoise_variance(); step()
        img = d.resolve_denoised_rgba8(2.2, True)
        active = d.adaptive_active_tiles()
        assert 0 < active[0] < active[1], active
        out.append((img, active, d.read_accum(), d.read_moments(), d.read_denoised()))
    assert out[0][1] == out[1][1] and np.array_equal(out[0][0], out[1][0])
    for a, b, what in zip(out[0][2:], out[1][2:], ("accumulator", "M", "D")):
        assert_bit_equal(a, b, f"unsynchronised vs synchronised: {what}")


# ---- 9. glrt_main --adaptive-variance
def test_glrt_main_adaptive_variance_writes_the_bindings_image(tmp_path, gpu_device):
    """The scene and frames of tests/test_gpu_adaptive.py's facade test (96x64, depth 4, three frames: the JSON scene and the binding's scene give the same samples there), one per burst: glrt_main --adaptive-variance T
    --denoise-variance prints the binding's active counts after each burst and writes the binding's resolve of the variance-guided D; with a negative threshold
    its PNG is the one glrt_main writes without the flag, which is the binding's render_frames image; the combinations the flag refuses are refused."""
    from PIL import Image
    from test_gpu_adaptive import _c1_builder
    w, h, depth, frames, thr = 96, 64, 4, 3, 0.05  # (bursts 1 and 2 find counts below min_samples everywhere; the third retires most tiles)
    b = _c1_builder()
    js = scenes.export_json_obj(b, tmp_path, w, h, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)
    exe = str(PKG / "lib" / "glrt_main")

    def glrt_main(extra, name):
        out = tmp_path / name
        r = subprocess.run([exe, "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--frames-in-flight", "1", "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.asarray(Image.open(out)), [ln for ln in r.stdout.splitlines() if "Adaptive:" in ln]

    img, lines = glrt_main(["--adaptive-variance", str(thr), "--min-spp", "2", "--denoise-variance"], "adaptive_var.png")
    raw, lines_raw = glrt_main(["--adaptive-variance", str(thr)], "adaptive_raw.png")
    b2 = scenes.SceneBuilder()
    for pos, nrm, mid in zip(b._pos, b._nrm, b._mid):
        b2.add_mesh(pos, nrm, b2.add_material(b.materials[int(mid[0])]))
    scene = b2.build()
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, w, h)
    params = dict(scenes.make_params(c2w, s2c, w, h, depth, 1), focal=0.0)  # (absent focalLength parses as 0)
    d = gpu_device
    _setup(d, scene, params)
    d.render_features(params)
    expect = []
    for f in range(frames):
        d.render_adaptive_moments(params, _seeds(1, f), thr, 2)
        a, t = d.adaptive_active_tiles()
        expect.append(f"[INFO] Adaptive: frame {f + 1}, active tiles {a}/{t}")
        if a == 0:
            break
    assert lines == expect and lines_raw == expect, (lines, lines_raw, expect)
    assert len(expect) == frames and 0 < a < t, expect
    assert np.array_equal(raw, d.resolve_rgba8(2.2, True))
    d.denoise_variance()
    ref = d.resolve_denoised_rgba8(2.2, True)
    assert np.array_equal(img, ref), int((img != ref).any(-1).sum())
    assert not np.array_equal(img, raw)
    every, lines_all = glrt_main(["--adaptive-variance", "-1"], "all.png")
    plain, lines_plain = glrt_main([], "plain.png")
    assert np.array_equal(every, plain) and len(lines_all) == frames and lines_plain == []
    _setup(d, scene, params, track=False)
    d.render_frames(params, _seeds(frames))
    d.sync()
    assert np.array_equal(plain, d.resolve_rgba8(2.2, True))  # without the flag the PNG is what it was
    for extra, word in ((["--adaptive", "0.05"], "--adaptive"), (["--save-every-frame"], "--save-every-frame"), (["--gpus", "2"], "one device"),
                        (["--min-spp", "1"], "--min-spp")):
        r = subprocess.run([exe, "-i", str(js), "--adaptive-variance", "0.1"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--adaptive-variance" in r.stderr and word in r.stderr, (extra, r.stderr)
