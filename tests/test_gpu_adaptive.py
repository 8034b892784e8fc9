"""Adaptive sampling on the GPU (glrtx_render_adaptive; csrc/pt_kernel.hip.h: adaptive_select_kernel, adaptive_compact_kernel, pt_render_wgwf<..., ADAPT>,
accumulate_adaptive_kernel).  The selection is pinned bit for bit against its numpy statement (tests/adaptive_math.py), the rendered pixels against the
oracle's full frames, and the rest of the call against glrtx_render_frames on a second context: nothing retiring, everything retiring, ordering behind a
fed launch, partitions and groups, the refusals, and glrt_main --adaptive."""
import subprocess

import numpy as np
import pytest

import adaptive_math as am
from conftest import PKG, assert_bit_equal
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


@pytest.fixture(scope="module")
def devices(gpu_device):
    """Two contexts of this module's own, closed at its end (what they allocate at 1080p is given back); gpu_device first: torch's runtime is set up
    before libglrtx's."""
    ds = (device.Device(), device.Device())
    yield ds
    for d in ds:
        d.close()


def _setup(d, scene, params, rank=0, world=1, stripe=16):
    d.set_variant(2); d.count_rays(False)
    d.upload_scene(scene); d.set_partition(rank, world, stripe); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _random_buffers(rng, rows, width):
    acc = rng.uniform(0.0, 6.0, (rows, width, 4)).astype(np.float32)
    acc[..., 3] = rng.integers(2, 40, (rows, width)).astype(np.float32)
    half = (acc * np.float32(0.5) * rng.uniform(0.6, 1.4, acc.shape)).astype(np.float32)
    half[..., 3] = np.floor(acc[..., 3] / 2)
    return acc, half


# ---- 1. the selection kernels against the numpy statement
@pytest.mark.parametrize("rows,width", [(48, 64), (38, 50), (5, 3), (8, 8), (135, 241), (1, 1)])
def test_selection_matches_the_numpy_statement(gpu_device, rows, width):
    rng = np.random.default_rng(rows * 1000 + width)
    acc, half = _random_buffers(rng, rows, width)
    e_all = am.tile_error(acc, half)
    cases = [("random", acc, half, float(np.median(e_all)), 2)]
    hostile_a, hostile_h = acc.copy(), half.copy()
    flat_a, flat_h = hostile_a.reshape(-1, 4), hostile_h.reshape(-1, 4)
    n = flat_a.shape[0]
    pick = lambda k: rng.choice(n, size=max(1, n // k), replace=False)  # noqa: E731
    flat_a[pick(13), 0] = np.nan
    flat_a[pick(17), 1] = np.inf
    flat_h[pick(19), 2] = -np.inf
    flat_a[pick(11), 2] = -rng.uniform(0, 5, max(1, n // 11)).astype(np.float32)
    flat_a[pick(23), 3] = 0.0          # zero counts: 0 / 0, x / 0
    flat_h[pick(29), 3] = 0.0          # H.w == 0
    flat_a[pick(31), 0] = np.float32(3e38)
    flat_a[pick(37), 3] = np.float32(0.5)
    cases.append(("hostile", hostile_a, hostile_h, 0.05, 3))
    cases.append(("zero", np.zeros_like(acc), np.zeros_like(half), 1.0, 2))
    cases.append(("nothing retires", acc, half, -1.0, 2))
    cases.append(("everything retires", acc, half, 3e38, 2))
    for what, a, h, thr, ms in cases:
        mask, err, lst = device.adaptive_select(a, h, thr, ms)
        m_ref, e_ref, l_ref = am.select(a, h, thr, ms)
        assert np.array_equal(mask, m_ref), (what, int((mask != m_ref).sum()))
        assert np.array_equal(err.view(np.uint32), e_ref.view(np.uint32)), (what, np.argwhere(err.view(np.uint32) != e_ref.view(np.uint32))[:4])
        assert np.array_equal(lst, l_ref), what
    assert not device.adaptive_select(acc, half, 3e38, 2)[0].any()
    assert device.adaptive_select(acc, half, -1.0, 2)[0].all()


# ---- 2. parity with the oracle's full frames
@pytest.mark.parametrize("cfg,w,h", [("c1", 64, 48), ("c2", 50, 38)])
def test_adaptive_calls_equal_the_oracles_frames_on_active_tiles(gpu_device, cfg, w, h):
    from oracle import pt_oracle
    scene, params = scenes.CONFIGS[cfg](width=w, height=h, n_samples=1)
    d = gpu_device
    _setup(d, scene, params)
    calls = [1, 5, 1, 5]
    acc = np.zeros((h, w, 4), np.float32)
    half = np.zeros_like(acc)
    thr, f0 = None, 0
    for k, n in enumerate(calls):
        if k == 2:  # from here on some tiles retire: the median tile error after the second call
            thr = float(np.median(am.tile_error(acc, half)))
        t = -1.0 if thr is None else thr
        mask, _, _ = am.select(acc, half, t, 2)
        seeds = _seeds(n, f0)
        samples = np.stack([pt_oracle.render(scene, dict(params, seed=sd))[0] for sd in seeds])
        assert np.all(samples[..., 3] == 1)
        acc, half = am.accumulate(acc, half, samples, mask)
        d.render_adaptive(params, seeds, t, 2)
        active, total = d.adaptive_active_tiles()
        assert total == mask.size and active == int(mask.sum()), (k, active, total)
        if k == 2:
            assert 0 < active < total, (active, total)
        assert np.array_equal(d.tile_mask(), mask), k
        assert_bit_equal(d.read_accum(), acc, f"{cfg} accumulator after call {k}")
        assert_bit_equal(d.read_adaptive_half(), half, f"{cfg} half buffer after call {k}")
        f0 += n
    assert d.stats().device_error_pending == 0


# ---- 3. nothing retires: glrtx_render_frames bit for bit
def _nothing_retires(d, d2, scene, params, calls, count=False):
    _setup(d, scene, params); _setup(d2, scene, params)
    d.count_rays(count); d2.count_rays(count)
    f0 = 0
    for n in calls:
        d.render_adaptive(params, _seeds(n, f0), -1.0, 2)
        d2.render_frames(params, _seeds(n, f0))
        f0 += n
    active, total = d.adaptive_active_tiles()
    assert active == total
    d2.sync()
    assert_bit_equal(d.read_accum(), d2.read_accum(), "adaptive (threshold -1) vs render_frames")
    hf = d.read_adaptive_half()
    assert np.all(hf[..., 3] == np.floor(d2.read_accum()[..., 3] / 2))
    if count:
        assert d.stats().rays == d2.stats().rays > 0
    d.count_rays(False); d2.count_rays(False)


def test_nothing_retires_equals_render_frames_headline_1080p(devices):
    scene, params = scenes.CONFIGS["headline"]()
    _nothing_retires(*devices, scene, params, [1, 4, 2], count=True)


def test_nothing_retires_equals_render_frames_vine_tree(devices):
    scene, params = scenes.config_c3(width=96, height=72, n=2000)
    _nothing_retires(*devices, scene, params, [2, 1, 3])


@pytest.mark.parametrize("fetch", ["0", "1", "2"])
def test_nothing_retires_equals_render_frames_each_pair_fetch(devices, monkeypatch, fetch):
    monkeypatch.setenv("GLRTX_PAIR_FETCH", fetch)
    scene, params = scenes.config_c2(width=120, height=88)
    _nothing_retires(*devices, scene, params, [3, 1], count=fetch == "1")
    assert devices[0].stats().node_fetch_last == int(fetch)


# ---- 4. everything retires
def test_everything_retired_leaves_the_accumulator_alone(gpu_device):
    scene, params = scenes.config_c1(width=72, height=40, max_depth=2)
    d = gpu_device
    _setup(d, scene, params)
    d.render_adaptive(params, _seeds(3), -1.0, 2)
    before, half_before = d.read_accum(), d.read_adaptive_half()
    for n in (1, 5):
        d.render_adaptive(params, _seeds(n, 3), 3e38, 2)  # (returns GLRTX_OK: an error would raise)
        assert d.adaptive_active_tiles() == (0, 45)
        assert not d.tile_mask().any()
        assert_bit_equal(d.read_accum(), before, "accumulator under an all-retired call")
        assert_bit_equal(d.read_adaptive_half(), half_before, "half buffer under an all-retired call")
    d.sync()
    assert d.stats().device_error_pending == 0
    d.render(dict(params, seed=host.frame_seed(99)))  # the context goes on working
    d.sync()
    assert np.all(d.read_accum()[..., 3] == 4)


# ---- 5. ordering behind a fed launch
def test_adaptive_call_after_a_fed_burst_is_ordered_like_synced_calls(devices):
    scene, params = scenes.config_c2(width=160, height=96)
    s = _seeds(12)
    d, ref = devices
    _setup(ref, scene, params)
    ref.render_adaptive(params, s[0:2], -1.0, 2); ref.sync()
    ref.render_frames(params, s[2:6]); ref.sync()
    thr = float(np.median(am.tile_error(ref.read_accum(), ref.read_adaptive_half())))
    ref.render_adaptive(params, s[6:11], thr, 2); ref.sync()
    active_ref = ref.adaptive_active_tiles()
    ref.render(dict(params, seed=s[11])); ref.sync()
    assert 0 < active_ref[0] < active_ref[1], active_ref
    _setup(d, scene, params)
    d.render_adaptive(params, s[0:2], -1.0, 2)
    d.render_frames(params, s[2:6])  # (several frames, own stream: a fed launch, left open)
    d.render_adaptive(params, s[6:11], thr, 2)
    d.render(dict(params, seed=s[11]))
    d.sync()
    assert d.stats().feed_launches >= 1
    assert d.adaptive_active_tiles() == active_ref
    assert_bit_equal(d.read_accum(), ref.read_accum(), "fed burst + adaptive + render")
    assert_bit_equal(d.read_adaptive_half(), ref.read_adaptive_half(), "half buffer")


# ---- 6. partitions and groups
def test_group_members_equal_partitioned_single_contexts(devices):
    scene, params = scenes.config_c1(width=88, height=70, max_depth=3)
    w, h = params["width"], params["height"]
    singles = list(devices)
    for i, d in enumerate(singles):
        _setup(d, scene, params, i, 2, 8)  # (glrtx_group partitions into 8-row stripes)
    g = device.Group([0, 0])
    try:
        g.upload_scene(scene); g.resize(w, h); g.clear()
        s = _seeds(9)
        g.render_adaptive(params, s[0:3], -1.0, 2)
        for d in singles:
            d.render_adaptive(params, s[0:3], -1.0, 2)
        thr = float(np.median(am.tile_error(singles[0].read_accum(), singles[0].read_adaptive_half())))
        for sl, n_min in ((slice(3, 8), 2), (slice(8, 9), 3)):
            g.render_adaptive(params, s[sl], thr, n_min)
            for d in singles:
                d.render_adaptive(params, s[sl], thr, n_min)
            per = [d.adaptive_active_tiles() for d in singles]
            assert g.adaptive_active_tiles() == (sum(a for a, _ in per), sum(t for _, t in per))
        assert 0 < g.adaptive_active_tiles()[0] < g.adaptive_active_tiles()[1]
        full = g.read_accum()
        for i, d in enumerate(singles):
            ys = d.local_rows_y()
            assert_bit_equal(full[ys], d.read_accum(), f"member {i} accumulator")
            assert_bit_equal(g.read_adaptive_half()[i], d.read_adaptive_half(), f"member {i} half buffer")
            assert np.array_equal(g.tile_mask()[i], d.tile_mask()), i
    finally:
        g.close()


# ---- 7. refusals
def test_refusals_change_nothing(gpu_device):
    scene, params = scenes.config_c1(width=40, height=24, max_depth=2)
    d = gpu_device
    _setup(d, scene, params)
    d.render_adaptive(params, _seeds(2), -1.0, 2)
    acc, half, counts = d.read_accum(), d.read_adaptive_half(), d.adaptive_active_tiles()

    def refused(fn, undo=None, **kw):
        with pytest.raises(device.GlrtxError) as ei:
            fn()
        assert ei.value.code == device.GLRTX_EINVAL, str(ei.value)
        if undo:
            undo()
        assert_bit_equal(d.read_accum(), acc, "accumulator after a refused call")
        assert_bit_equal(d.read_adaptive_half(), half, "half buffer after a refused call")
        assert d.adaptive_active_tiles() == counts

    call = lambda p=params, ms=2: d.render_adaptive(p, _seeds(2, 2), 0.01, ms)  # noqa: E731
    refused(lambda: call(ms=1))
    d.present_enable(2)
    refused(call, lambda: d.present_enable(0))
    d.set_extensions(device.EXT_DIELECTRIC)
    refused(call, lambda: d.set_extensions(0))
    d.set_extensions(device.EXT_VOLUME)
    refused(call, lambda: d.set_extensions(0))
    d.upload_spheres([[0.0, 1.0, 0.0, 0.5, 0.0]])
    refused(call, lambda: d.upload_spheres(None))
    d.set_variant(1)
    refused(call, lambda: d.set_variant(2))
    refused(lambda: call(p=dict(params, max_depth=256)))
    d.render_adaptive(params, _seeds(1, 2), -1.0, 2)  # and the context still renders
    assert np.all(d.read_accum()[..., 3] == 3)


# ---- 8. glrt_main --adaptive
def _c1_builder(subdiv=1):
    b = scenes.SceneBuilder()  # (the scene of tests/test_gpu_facade.py)
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    red = b.add_material(scenes.diffuse((0.8, 0.3, 0.3)))
    cu = b.add_material(scenes.conductor(scenes.COPPER["eta"], scenes.COPPER["kappa"], 0.2))
    lamp = b.add_material(scenes.emitter((10.0, 10.0, 10.0)))
    b.add_mesh(*scenes.quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*scenes.icosphere(subdiv, 1.0, (-2.2, 1.0, 0.0)), red)
    b.add_mesh(*scenes.icosphere(subdiv, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*scenes.icosphere(subdiv, 1.0, (2.2, 1.0, 0.0)), grey)
    b.add_mesh(*scenes.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    return b


def test_glrt_main_adaptive_writes_the_bindings_image(tmp_path, gpu_device):
    """The frames of tests/test_gpu_facade.py (96x64, depth 4, three frames: the JSON scene and the binding's scene give the same samples there), one frame
    per burst: glrt_main --adaptive prints the binding's active counts after each burst and writes the binding's resolve; with a negative threshold its
    PNG is the one glrt_main writes without --adaptive."""
    from PIL import Image
    w, h, depth, frames, thr = 96, 64, 4, 3, 0.05
    b = _c1_builder()
    js = scenes.export_json_obj(b, tmp_path, w, h, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)

    def glrt_main(extra, name):
        out = tmp_path / name
        r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--frames-in-flight", "1",
                            "--out", str(out)] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return np.asarray(Image.open(out)), [ln for ln in r.stdout.splitlines() if "Adaptive:" in ln]

    img, lines = glrt_main(["--adaptive", str(thr), "--min-spp", "2"], "adaptive.png")
    b2 = scenes.SceneBuilder()
    for pos, nrm, mid in zip(b._pos, b._nrm, b._mid):
        b2.add_mesh(pos, nrm, b2.add_material(b.materials[int(mid[0])]))
    scene = b2.build()
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, w, h)
    params = dict(scenes.make_params(c2w, s2c, w, h, depth, 1), focal=0.0)  # (absent focalLength parses as 0)
    d = gpu_device
    _setup(d, scene, params)
    expect = []
    for f in range(frames):
        d.render_adaptive(params, _seeds(1, f), thr, 2)
        a, t = d.adaptive_active_tiles()
        expect.append(f"[INFO] Adaptive: frame {f + 1}, active tiles {a}/{t}")
        if a == 0:
            break
    assert lines == expect, (lines, expect)
    ref = d.resolve_rgba8(2.2, True)
    assert np.array_equal(img, ref), int((img != ref).any(-1).sum())
    every, lines_all = glrt_main(["--adaptive", "-1"], "all.png")
    plain, lines_plain = glrt_main([], "plain.png")
    assert np.array_equal(every, plain) and len(lines_all) == frames and lines_plain == []


# ---- 9. shape changes and a rebound accumulator
def test_tile_mask_of_another_shape_is_refused(gpu_device):
    """The binding sizes the mask by the context's current shape: after a resize or a repartition the last selection's mask is refused (GLRTX_EINVAL),
    not copied past the caller's buffer; H is zeroed at the new shape; the next adaptive call selects on the new shape."""
    scene, params = scenes.config_c1(width=120, height=96, max_depth=2)
    d = gpu_device
    _setup(d, scene, params)
    d.render_adaptive(params, _seeds(2), -1.0, 2)
    assert d.tile_mask().shape == (12, 15)
    for change in (lambda: d.resize(40, 24), lambda: d.set_partition(1, 2, 8)):
        change()
        with pytest.raises(device.GlrtxError) as ei:
            d.tile_mask()
        assert ei.value.code == device.GLRTX_EINVAL
        half = d.read_adaptive_half()  # (H follows the accumulator: zeroed at the new shape)
        assert half.shape == (d.stats().owned_rows, d.stats().width, 4) and not half.any()
    small = dict(params, width=40, height=24)
    d.set_partition(0, 1, 16); d.resize(40, 24)
    d.render_adaptive(small, _seeds(1), -1.0, 2)
    assert d.tile_mask().shape == (3, 5) and d.tile_mask().all()
    assert d.adaptive_active_tiles() == (15, 15)


def test_binding_another_accumulator_zeroes_the_half_buffer(gpu_device):
    import torch
    scene, params = scenes.config_c1(width=64, height=40, max_depth=2)
    d = gpu_device
    _setup(d, scene, params)
    d.render_adaptive(params, _seeds(3), -1.0, 2)
    assert d.read_adaptive_half()[..., 3].max() == 1
    t = torch.zeros((40, 64, 4), dtype=torch.float32, device="cuda")
    try:
        d.bind_accum(t.data_ptr(), 64 * 16, 40)
        assert not d.read_adaptive_half().any()
        d.render_adaptive(params, _seeds(2, 3), 3e38, 2)  # (an empty accumulator and H: every tile is active)
        assert d.adaptive_active_tiles() == (40, 40)
        torch.cuda.synchronize()
        assert np.all(t.cpu().numpy()[..., 3] == 2)
    finally:
        d.bind_accum(0, 0, 0)
