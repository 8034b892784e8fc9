"""Presentation (glrtx_present_*): every frame's image out of the context's pinned ring, without a sync.  Every image is compared byte for byte -- with the oracle's
resolve of the oracle's accumulator after that frame, or with glrtx_resolve_rgba8 of a context that syncs after every frame -- across every launch form, the ring's
GLRTX_EBUSY semantics, partitions, groups and the facade's --save-every-frame loop."""
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, assert_bit_equal
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


def _setup(d, scene, params):
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _take(d, n):
    """n images in frame order, copied out and released."""
    out = []
    for _ in range(n):
        img = d.present_acquire(wait=True)
        out.append((img.frame, img.rgba.copy()))
        d.present_release(img)
    return out


@pytest.fixture
def dev(gpu_device):
    yield gpu_device
    gpu_device.present_enable(0)
    gpu_device.set_variant(2)
    gpu_device.set_stream(None)


@pytest.mark.parametrize("cfg,size,flip", [("c1", (64, 48), True), ("c2", (50, 38), False), ("c2", (64, 64), True)])
@pytest.mark.parametrize("form", ["singles", "frames", "mixed"])
def test_every_image_is_the_oracles_resolve_after_that_frame(dev, cfg, size, flip, form):
    from oracle import pt_oracle
    w, h = size
    scene, params = scenes.CONFIGS[cfg](width=w, height=h, max_depth=4)
    seeds = _seeds(12)
    d = dev
    _setup(d, scene, params)
    d.present_enable(16, 2.2, flip)
    if form == "singles":
        for sd in seeds:
            d.render(dict(params, seed=sd))
    elif form == "frames":
        d.render_frames(params, seeds)
    else:
        for sd in seeds[:3]:
            d.render(dict(params, seed=sd))
        d.render_frames(params, seeds[3:9])
        for sd in seeds[9:]:
            d.render(dict(params, seed=sd))
    imgs = _take(d, 12)
    ref = None
    for k, sd in enumerate(seeds):
        ref, _ = pt_oracle.render(scene, dict(params, seed=sd), accum=ref)
        frame, rgba = imgs[k]
        assert frame == k + 1
        assert np.array_equal(rgba, pt_oracle.resolve(ref, 2.2, flip)), (cfg, size, form, k)
    assert_bit_equal(d.read_accum(), ref, "accumulator")
    ps = d.present_stats()
    assert ps.pending == 0 and ps.held == 0 and ps.copies_last == 1


def test_1080p_headline_burst_presents_every_frame_and_stays_fed(dev):
    """48 glrtx_render calls back to back with a ring of 48: images equal a syncing context's glrtx_resolve_rgba8 after every frame, the accumulators are bit-equal,
    and the burst was fed (presentation does not seal the open launch)."""
    scene, params = scenes.CONFIGS["headline"]()
    seeds = _seeds(48)
    d = dev
    _setup(d, scene, params)
    d.present_enable(48, 2.2, True)
    for sd in seeds:
        d.render(dict(params, seed=sd))
    imgs = [d.present_acquire(wait=True) for _ in range(48)]
    acc = d.read_accum()
    st = d.stats()
    assert st.feed_appended >= 40 and st.kernel_launches < 10, (st.feed_appended, st.kernel_launches)
    ref = device.Device()
    try:
        _setup(ref, scene, params)
        for k, sd in enumerate(seeds):
            ref.render(dict(params, seed=sd))
            ref.sync()
            assert imgs[k].frame == k + 1
            assert np.array_equal(imgs[k].rgba, ref.resolve_rgba8(2.2, True)), k
        assert ref.stats().feed_appended == 0
        assert_bit_equal(acc, ref.read_accum(), "accumulator")
    finally:
        ref.close()
    for img in imgs:
        d.present_release(img)
    assert d.present_stats().pass_ms_last > 0.0


@pytest.mark.parametrize("form", ["variant0", "variant1", "variant2", "plain", "stream", "spp4", "extension"])
@pytest.mark.parametrize("flip", [0, 1])
def test_every_launch_form_presents_its_own_resolve(dev, monkeypatch, form, flip):
    """plain: GLRTX_NO_PIPELINE=1, single frames accumulate inside the wavefront kernel (no planes: the resolve kernel follows the launch)."""
    import torch
    d = dev
    if form == "plain":
        monkeypatch.setenv("GLRTX_NO_PIPELINE", "1")
        d = device.Device()
    if form == "extension":
        scene, params, spheres = scenes.config_spheres(48, 40, max_depth=4, n_samples=2, glass=True)
    else:
        scene, params = scenes.CONFIGS["c2"](width=72, height=40, max_depth=4, n_samples=4 if form == "spp4" else 1)
    _setup(d, scene, params)
    stream = None
    if form.startswith("variant"):
        d.set_variant(int(form[-1]))
    if form == "stream":
        stream = torch.cuda.Stream()
        d.set_stream(stream.cuda_stream)
    if form == "extension":
        d.upload_spheres(spheres); d.set_extensions(device.EXT_DIELECTRIC)
    try:
        d.present_enable(4, 2.2, flip)
        seeds = _seeds(6)
        for sd in seeds[:3]:  # one frame at a time: image == the context's own resolve after it
            d.render(dict(params, seed=sd))
            img = d.present_acquire(wait=True)
            assert np.array_equal(img.rgba, d.resolve_rgba8(2.2, flip)), form
            d.present_release(img)
        d.render_frames(params, seeds[3:])  # and a call of several frames
        imgs = _take(d, 3)
        assert [f for f, _ in imgs] == [4, 5, 6]
        assert np.array_equal(imgs[-1][1], d.resolve_rgba8(2.2, flip)), form
    finally:
        d.present_enable(0)
        if form == "extension":
            d.set_extensions(0); d.upload_spheres(None)
        if stream is not None:
            d.set_stream(None)
        if form == "plain":
            d.close()


def test_ring_semantics(dev):
    scene, params = scenes.CONFIGS["c2"](width=64, height=48, max_depth=4)
    seeds = _seeds(4)
    d = dev
    _setup(d, scene, params)
    ps0 = d.present_stats()  # (the counters run over the context's life)
    d.present_enable(2, 2.2, True)
    assert d.present_acquire(wait=False) is None  # nothing rendered: GLRTX_EBUSY
    d.render(dict(params, seed=seeds[0]))
    d.render(dict(params, seed=seeds[1]))
    d.sync()
    before = d.stats()
    with pytest.raises(device.GlrtxError) as e:
        d.render(dict(params, seed=seeds[2]))
    assert e.value.code == device.GLRTX_EBUSY
    with pytest.raises(device.GlrtxError) as e:
        d.render_frames(params, seeds[2:4])
    assert e.value.code == device.GLRTX_EBUSY
    after = d.stats()
    for f in ("launches", "kernel_launches", "paths", "feed_appended", "feed_launches"):
        assert getattr(before, f) == getattr(after, f), f
    with pytest.raises(device.GlrtxError) as e:
        d.render_frames(params, _seeds(3))  # more frames than the ring holds
    assert e.value.code == device.GLRTX_EINVAL
    first = _take(d, 1)
    d.render(dict(params, seed=seeds[2]))  # the refused call again, now that an image is free
    imgs = first + _take(d, 2)
    assert [f for f, _ in imgs] == [1, 2, 3]
    ref = device.Device()
    try:
        _setup(ref, scene, params)
        for k in range(3):
            ref.render(dict(params, seed=seeds[k]))
            assert np.array_equal(imgs[k][1], ref.resolve_rgba8(2.2, True)), k
    finally:
        ref.close()
    ps = d.present_stats()
    assert ps.busy_returns - ps0.busy_returns == 3 and ps.delivered - ps0.delivered == 3 and ps.images - ps0.images == 3
    # frame numbers restart after clear; resize fails while an image is held
    d.clear()
    d.render(dict(params, seed=seeds[0]))
    img = d.present_acquire(wait=True)
    assert img.frame == 1
    with pytest.raises(device.GlrtxError) as e:
        d.resize(32, 32)
    assert e.value.code == device.GLRTX_EINVAL
    d.present_release(img)
    d.resize(64, 48)
    # disable drops what was not acquired
    d.render(dict(params, seed=seeds[0]))
    d.render(dict(params, seed=seeds[1]))
    d.present_enable(0)
    ps = d.present_stats()
    assert ps.dropped - ps0.dropped == 2 and ps.ring_images == 0


def test_partition_rank_images_are_its_own_resolve(dev):
    scene, params = scenes.CONFIGS["c2"](width=80, height=60, max_depth=4)
    d = dev
    d.upload_scene(scene); d.set_partition(1, 3, 16); d.resize(80, 60); d.clear()
    try:
        d.present_enable(4, 2.2, True)
        for sd in _seeds(3):
            d.render(dict(params, seed=sd))
            img = d.present_acquire(wait=True)
            assert img.rgba.shape == (d.stats().owned_rows, 80, 4)
            assert np.array_equal(img.rgba, d.resolve_rgba8(2.2, True))
            d.present_release(img)
    finally:
        d.present_enable(0)
        d.set_partition(0, 1, 16)


@pytest.mark.parametrize("h", [48, 45])
@pytest.mark.parametrize("flip", [True, False])
def test_group_images_are_the_full_frame(gpu_device, h, flip):
    """A [0, 0, 0] group: every member lands its stripes in the shared pinned image with at most two copies; the image is a one-context render's resolve."""
    scene, params = scenes.CONFIGS["c2"](width=72, height=h, max_depth=4)
    seeds = _seeds(5)
    d = gpu_device
    _setup(d, scene, params)
    refs = []
    for sd in seeds:
        d.render(dict(params, seed=sd))
        refs.append(d.resolve_rgba8(2.2, flip))
    g = device.Group([0, 0, 0])
    try:
        g.upload_scene(scene); g.resize(72, h); g.clear()
        g.present_enable(3, 2.2, flip)
        got = []
        for sd in seeds[:2]:
            g.render(dict(params, seed=sd))
        for _ in range(2):
            img = g.present_acquire(wait=True)
            got.append((img.frame, img.rgba.copy())); g.present_release(img)
        g.render_frames(params, seeds[2:3])
        g.render_frames(params, seeds[3:5])
        for _ in range(3):
            img = g.present_acquire(wait=True)
            got.append((img.frame, img.rgba.copy())); g.present_release(img)
        assert [f for f, _ in got] == [1, 2, 3, 4, 5]
        for k in range(5):
            assert got[k][1].shape == (h, 72, 4)
            assert np.array_equal(got[k][1], refs[k]), k
        ps = g.present_stats()
        assert 3 <= ps.copies_last <= 6
        assert g.present_acquire(wait=False) is None
    finally:
        g.close()


def _c1_json(tmp_path, w, h):
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    red = b.add_material(scenes.diffuse((0.8, 0.3, 0.3)))
    lamp = b.add_material(scenes.emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*scenes.quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*scenes.icosphere(1, 1.0, (-1.2, 1.0, 0.0)), red)
    b.add_mesh(*scenes.icosphere(1, 1.0, (1.2, 1.0, 0.0)), grey)
    b.add_mesh(*scenes.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    return scenes.export_json_obj(b, tmp_path, w, h, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)


@pytest.mark.parametrize("devices", [[], ["--devices", "0,0"]])
def test_glrt_main_save_every_frame_presents_fed_frames(tmp_path, gpu_device, devices):
    js = _c1_json(tmp_path, 1280, 720)
    outs = {}
    for name, extra in (("last", []), ("every", ["--save-every-frame"])):
        out = tmp_path / f"{name}.png"
        r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", "8", "--frames", "16", "--out", str(out)] + devices + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert r.stdout.count("Save:") == (16 if name == "every" else 1)
        outs[name] = (out.read_bytes(), r.stdout)
    assert outs["last"][0] == outs["every"][0]
    m = re.search(r"Presented: (\d+) frames, (\d+) images, (\d+) render kernel launches", outs["every"][1])
    assert m, outs["every"][1]
    frames, images, launches = (int(v) for v in m.groups())
    assert frames == images == 16 and launches < 16, outs["every"][1]
