"""The volume branch on the wavefront kernel (glrtx_set_volume_wavefront: pt_render_wgwf's V form, csrc/pt_kernel.hip.h: wf_vol_trial).  Bit for bit
the llvmpipe goldens of tests/golden/volume and the persistent megakernel's volume instantiation -- images and ray counts -- through every way a
launch is made: frames in flight, fed single calls, adaptive calls, the present ring, a group; and the routing back to the megakernel where the V
form does not apply."""
import subprocess

import numpy as np
import pytest

import adaptive_math as am
from conftest import GOLDEN, PKG, assert_bit_equal, load_golden
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

VOLUME = GOLDEN / "volume"
FIXTURES = sorted(p.stem for p in VOLUME.glob("vol_*.npz"))
NO_VOLUME = (None, None, (0, 0, 0), (1, 1, 1))


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    monkeypatch.delenv("GLRTX_VOLUME_WAVEFRONT", raising=False)


@pytest.fixture(scope="module")
def devices(gpu_device):
    """Two contexts of this module's own (gpu_device first: torch's runtime is set up before libglrtx's)."""
    ds = (device.Device(), device.Device())
    yield ds
    for d in ds:
        d.close()


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


def load_volume(name):
    scene, params, rows, frames, rgb, cnt = load_golden(f"volume/{name}")
    z = np.load(VOLUME / f"{name}.npz")
    vol = dict(density=z["density"], temperature=z["temperature"], bbox_min=z["bbox"][:3], bbox_max=z["bbox"][3:], density_max=float(z["density_max"]))
    return scene, params, frames, vol, rgb, cnt


def _setup(d, scene, params, vol, wavefront, count=False):
    d.set_variant(2)
    d.count_rays(count)
    d.upload_scene(scene)
    d.upload_volume(**vol)
    d.set_extensions(device.EXT_VOLUME)
    d.set_volume_wavefront(wavefront)
    d.set_partition(0, 1, 16)
    d.resize(params["width"], params["height"])
    d.clear()
    d.reset_stats()


def _teardown(*ds):
    for d in ds:
        d.set_volume_wavefront(False)
        d.set_extensions(0)
        d.upload_spheres(None)
        d.upload_volume(*NO_VOLUME)
        d.count_rays(False)


def _render(d, params, frames):
    if frames:
        d.render_frames(params, frames)
    else:
        d.render(params)
    d.sync()
    return d.read_accum(), d.stats()


def _hot_dense(width=96, height=72):
    """A small, hot and dense medium at depth 16: many scatter events per trial chain (the eight-trial fall-through) and deep paths (Russian roulette)."""
    scene, params, vol = scenes.config_fire(width=width, height=height, max_depth=16, grid=16, temperature=30.0)
    vol = dict(vol, density=(vol["density"] * np.float32(60.0)).astype(np.float32))
    return scene, params, vol


# ---- 1. the goldens, both instantiations; ray counts equal the megakernel's
@pytest.mark.parametrize("count_rays", [True, False], ids=["counting", "timed"])
@pytest.mark.parametrize("name", FIXTURES)
def test_goldens_on_the_wavefront_kernel(devices, name, count_rays):
    d, d2 = devices
    scene, params, frames, vol, rgb, cnt = load_volume(name)
    try:
        _setup(d, scene, params, vol, True, count_rays)
        acc, st = _render(d, params, frames)
        assert st.variant_last == 2 and st.fallback_last == 0, (st.variant_last, st.fallback_last)
        assert st.device_error_pending == 0
        assert_bit_equal(acc[..., :3], rgb, f"{name} rgb")
        assert_bit_equal(acc[..., 3], cnt, f"{name} count")
        if count_rays:
            _setup(d2, scene, params, vol, False, True)
            acc2, st2 = _render(d2, params, frames)
            assert st2.variant_last == 1
            assert st.rays == st2.rays > 0 and st.rays_untraced == st2.rays_untraced
    finally:
        _teardown(d, d2)


# ---- 2. frames in flight and fed single calls against the megakernel
@pytest.mark.parametrize("case", ["fire_1080p", "hot_dense_depth16"])
def test_frames_in_flight_and_fed_calls_equal_the_megakernel(devices, case):
    d, d2 = devices
    if case == "fire_1080p":
        scene, params, vol = scenes.config_fire()
    else:
        scene, params, vol = _hot_dense()
    seeds = _seeds(24)
    try:
        _setup(d2, scene, params, vol, False, True)
        ref = []
        for k, sd in enumerate(seeds):
            d2.render(dict(params, seed=sd))
            if k + 1 in (20, 24):
                d2.sync()
                ref.append((d2.read_accum(), d2.stats().rays))
        assert d2.stats().variant_last == 1

        _setup(d, scene, params, vol, True, True)
        acc, st = _render(d, params, seeds[:20])
        assert st.variant_last == 2 and st.fallback_last == 0 and st.device_error_pending == 0
        assert_bit_equal(acc, ref[0][0], f"{case}: 20-frame render_frames vs 20 megakernel launches")
        assert st.rays == ref[0][1]

        _setup(d, scene, params, vol, True, True)
        for sd in seeds:
            d.render(dict(params, seed=sd))
        d.sync()
        st = d.stats()
        assert st.feed_appended > 0 and st.variant_last == 2 and st.device_error_pending == 0
        assert_bit_equal(d.read_accum(), ref[1][0], f"{case}: 24 fed calls vs 24 megakernel launches")
        assert st.rays == ref[1][1]
    finally:
        _teardown(d, d2)


# ---- 3. adaptive calls with the volume on
def test_adaptive_nothing_retires_equals_render_frames(devices):
    d, d2 = devices
    scene, params, vol = _hot_dense(80, 56)
    try:
        _setup(d, scene, params, vol, True, True)
        _setup(d2, scene, params, vol, False, True)
        f0 = 0
        for n in (1, 4, 2):
            d.render_adaptive(params, _seeds(n, f0), -1.0, 2)
            d2.render_frames(params, _seeds(n, f0))
            f0 += n
        active, total = d.adaptive_active_tiles()
        assert active == total
        d2.sync()
        assert d.stats().variant_last == 2 and d2.stats().variant_last == 1
        assert_bit_equal(d.read_accum(), d2.read_accum(), "adaptive (threshold -1) vs render_frames")
        assert d.stats().rays == d2.stats().rays > 0
    finally:
        _teardown(d, d2)


def test_adaptive_median_threshold_equals_the_megakernels_frames_on_active_tiles(devices):
    d, d2 = devices
    scene, params, vol = scenes.config_fire(width=72, height=56, max_depth=8, grid=16)
    try:
        _setup(d, scene, params, vol, True)
        _setup(d2, scene, params, vol, False)
        h, w = params["height"], params["width"]
        acc = np.zeros((h, w, 4), np.float32)
        half = np.zeros_like(acc)
        thr, f0 = None, 0
        for k, n in enumerate([1, 5, 1, 5]):
            if k == 2:
                thr = float(np.median(am.tile_error(acc, half)))
            t = -1.0 if thr is None else thr
            mask, _, _ = am.select(acc, half, t, 2)
            samples = []
            for sd in _seeds(n, f0):  # one frame of one sample per launch on the megakernel, in a context of its own
                d2.clear()
                d2.render(dict(params, seed=sd))
                d2.sync()
                samples.append(d2.read_accum())
            samples = np.stack(samples)
            assert np.all(samples[..., 3] == 1)
            acc, half = am.accumulate(acc, half, samples, mask)
            d.render_adaptive(params, _seeds(n, f0), t, 2)
            active, total = d.adaptive_active_tiles()
            assert total == mask.size and active == int(mask.sum()), (k, active, total)
            if k == 2:
                assert 0 < active < total, (active, total)
            assert d.stats().variant_last == 2
            assert_bit_equal(d.read_accum(), acc, f"accumulator after call {k}")
            assert_bit_equal(d.read_adaptive_half(), half, f"half buffer after call {k}")
            f0 += n
        assert d.stats().device_error_pending == 0
    finally:
        _teardown(d, d2)


# ---- 4. the present ring
def test_present_ring_images_equal_the_resolve(devices):
    d, _ = devices
    scene, params, vol = _hot_dense(64, 48)
    try:
        _setup(d, scene, params, vol, True)
        d.present_enable(4)
        try:
            for f in range(3):
                d.render(dict(params, seed=host.frame_seed(f)))
                img = d.present_acquire(True)
                ref = d.resolve_rgba8(2.2, True)
                assert np.array_equal(img.rgba, ref), f
                d.present_release(img)
            d.render_frames(params, _seeds(3, 3))
            imgs = [d.present_acquire(True) for _ in range(3)]
            ref = d.resolve_rgba8(2.2, True)
            assert np.array_equal(imgs[-1].rgba, ref)
            for img in imgs:
                d.present_release(img)
            assert d.stats().variant_last == 2
        finally:
            d.present_enable(0)
    finally:
        _teardown(d)


# ---- 5. a group of two on one device
@pytest.mark.parametrize("name", ["vol_fire16", "vol_frames3"])
def test_group_of_two_on_one_device_equals_one_context(devices, name):
    d, _ = devices
    scene, params, frames, vol, rgb, cnt = load_volume(name)
    try:
        _setup(d, scene, params, vol, True)
        one, st = _render(d, params, frames)
        assert st.variant_last == 2
    finally:
        _teardown(d)
    g = device.Group([0, 0])
    try:
        g.upload_scene(scene)
        g.upload_volume(**vol)
        g.member_call(g.L.glrtx_set_extensions, device.EXT_VOLUME)
        g.member_call(g.L.glrtx_set_volume_wavefront, 1)
        g.resize(params["width"], params["height"])
        two, _ = _render(g, params, frames)
    finally:
        g.close()
    assert_bit_equal(two, one, f"{name}: group vs context")
    assert_bit_equal(two[..., :3], rgb, f"{name}: group vs reference")


# ---- 6. where the V form does not apply
@pytest.mark.parametrize("other", ["dielectric", "spheres"])
def test_other_extensions_still_run_on_the_megakernel(devices, other):
    d, _ = devices
    scene, params, frames, vol, _, _ = load_volume("vol_fire16")
    try:
        _setup(d, scene, params, vol, True)
        if other == "dielectric":
            d.set_extensions(device.EXT_VOLUME | device.EXT_DIELECTRIC)
        else:
            d.upload_spheres([[0.0, 5.0, 0.0, 0.25, 0.0]])
        d.render(dict(params, seed=host.frame_seed(0)))
        d.sync()
        st = d.stats()
        assert st.variant_last == 1 and st.fallback_last & device.FALLBACK_EXTENSIONS
        with pytest.raises(device.GlrtxError, match="tile list") as e:
            d.render_adaptive(params, _seeds(1), -1.0, 2)
        assert e.value.code == device.GLRTX_EINVAL
    finally:
        _teardown(d)


def test_switch_off_keeps_the_megakernel_and_the_refusal(devices):
    d, _ = devices
    scene, params, frames, vol, _, _ = load_volume("vol_fire16")
    try:
        _setup(d, scene, params, vol, False)
        d.render(dict(params, seed=host.frame_seed(0)))
        d.sync()
        assert d.stats().variant_last == 1
        with pytest.raises(device.GlrtxError, match="extensions or volume are on"):
            d.render_adaptive(params, _seeds(1), -1.0, 2)
    finally:
        _teardown(d)


# ---- 7. the façade
def test_glrt_main_volume_wavefront_and_adaptive(tmp_path, gpu_device):
    """glrt_main --enable-volume --adaptive T (a fatal error before the V form) exits 0 and writes the image the binding's adaptive calls produce;
    --volume-wavefront writes the PNG of the default --enable-volume run."""
    from PIL import Image
    w, h, depth, frames, thr = 64, 48, 8, 3, 0.05
    lo, hi = (-1.0, 0.05, -1.0), (1.0, 2.05, 1.0)
    dens, temp = scenes.fire_grids((16, 16, 16), 10.0)
    b = scenes.SceneBuilder()
    b.add_mesh(*scenes.box(lo, hi), b.add_material(scenes.media({"density": "d.vol", "temperature": "t.vol", "bboxMin": lo, "bboxMax": hi})))
    b.add_mesh(*scenes.quad((-6, 0, 6), (12, 0, 0), (0, 0, -12)), b.add_material(scenes.diffuse((0.7, 0.7, 0.7))))
    b.add_mesh(*scenes.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2)), b.add_material(scenes.emitter((6.0, 6.0, 6.0))))
    eye = (0.4, 2.4, 5.5)
    js = scenes.export_json_obj(b, tmp_path, w, h, eye, (0, 1, 0), (0, 1, 0), 42.0)
    scenes.write_vol(tmp_path / "d.vol", dens, (0, 0, 0), (1, 1, 1))
    scenes.write_vol(tmp_path / "t.vol", temp, (0, 0, 0), (1, 1, 1))

    def glrt_main(extra, name):
        out = tmp_path / name
        r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--frames-in-flight", "1",
                            "--out", str(out), "--enable-volume"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.asarray(Image.open(out)), [ln for ln in r.stdout.splitlines() if "Adaptive:" in ln]

    plain, _ = glrt_main([], "plain.png")
    vwf, _ = glrt_main(["--volume-wavefront"], "vwf.png")
    assert np.array_equal(plain, vwf)
    img, lines = glrt_main(["--adaptive", str(thr), "--min-spp", "2"], "adaptive.png")

    c2w, s2c = scenes.camera(eye, (0, 1, 0), (0, 1, 0), 42.0, w, h)
    params = dict(scenes.make_params(c2w, s2c, w, h, depth, 1), focal=0.0)  # (absent focalLength parses as 0)
    d = gpu_device
    try:
        _setup(d, b.build(), params, dict(density=dens, temperature=temp, bbox_min=lo, bbox_max=hi), True)
        expect = []
        for f in range(frames):
            d.render_adaptive(params, _seeds(1, f), thr, 2)
            a, t = d.adaptive_active_tiles()
            expect.append(f"[INFO] Adaptive: frame {f + 1}, active tiles {a}/{t}")
            if a == 0:
                break
        assert lines == expect, (lines, expect)
        ref = d.resolve_rgba8(2.2, True)
    finally:
        _teardown(d)
    assert np.array_equal(img, ref), int((img != ref).any(-1).sum())
