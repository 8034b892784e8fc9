"""The denoiser on the GPU (csrc/features.hip.h, csrc/denoise.hip.h): the feature planes equal the CPU statement (glrt_render_features) bit for bit in both
node layouts, on a vine and on a partitioned context; the filter equals glrt_denoise_atrous bit for bit on hostile arrays and after real renders; the 8-bit
image of D is the oracle's resolve of D; and none of the calls touches the accumulator, the half buffer, the ray counts or an interrupted run of fed launches."""
import numpy as np
import pytest

import denoise_math as dm
from fuzz_scenes import CASES, case_scene_and_params
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} of {bad.shape[0] * bad.shape[1]} pixels differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0][:2])].tolist()} vs {ref[tuple(np.argwhere(bad)[0][:2])].tolist()}"


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, rank=0, world=1, stripe=16, count=False):
    d.set_variant(2); d.count_rays(count)
    d.upload_scene(scene); d.set_partition(rank, world, stripe); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _check_features(d, monkeypatch, scene, params, what, **part):
    _setup(d, scene, params, **part)
    ref_n, ref_a = host.render_features(scene, params, **part)
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        d.render_features(params)
        n, a = d.read_features()
        _same(n, ref_n, f"{what} compact={compact} normal/depth")
        _same(a, ref_a, f"{what} compact={compact} albedo/id")
    monkeypatch.delenv("GLRTX_COMPACT_NODES")
    return ref_n, ref_a


# ---- 1. feature planes
def test_features_c1(dev, monkeypatch):
    scene, params = scenes.config_c1(256, 256, max_depth=4, subdiv=2)
    _check_features(dev, monkeypatch, scene, params, "c1")


@pytest.mark.parametrize("case", [0, 1, 4, 5, 7, 10], ids=lambda c: f"fuzz{CASES[c][0]}-{CASES[c][2]}")
def test_features_fuzz(dev, monkeypatch, case):
    scene, params = case_scene_and_params(CASES[case])
    _check_features(dev, monkeypatch, scene, params, f"case {CASES[case][0]}")


def test_features_vine(dev, monkeypatch):
    scene, params = scenes.config_c3(96, 64, n=3000)
    _check_features(dev, monkeypatch, scene, params, "c3 vine")
    scene, params = case_scene_and_params(CASES[2])  # a chain tree of a fuzz scene
    _check_features(dev, monkeypatch, scene, params, "fuzz vine")


def test_features_partitioned(dev, monkeypatch):
    scene, params = scenes.config_c1(100, 75, max_depth=4, subdiv=1)
    for rank in range(3):
        _check_features(dev, monkeypatch, scene, params, f"rank {rank}/3", rank=rank, world=3, stripe=8)
    dev.set_partition(0, 1, 16)


# ---- 2. the filter
@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (17, 33), (5, 130), (1, 1), (70, 49)])
def test_filter_on_hostile_arrays(gpu_device, rows, width):
    acc, N, A = dm.hostile_arrays(rows, width, rows * 1000 + width)
    for iterations in range(1, 7):
        for demodulate in (0, 1):
            for sc in (1.0, 1e3):
                got = device.debug_denoise(acc, N, A, iterations=iterations, sigma_color=sc, sigma_normal=0.1, sigma_depth=0.01, demodulate=demodulate)
                ref = host.denoise_atrous(acc, N, A, iterations, sc, 0.1, 0.01, demodulate)
                _same(got, ref, f"{width}x{rows} it={iterations} demod={demodulate} sc={sc}")
    got = device.debug_denoise(acc, N, A, iterations=6, sigma_color=1e-38, sigma_normal=1e-30, sigma_depth=1e-30, demodulate=1)
    _same(got, host.denoise_atrous(acc, N, A, 6, 1e-38, 1e-30, 1e-30, 1), "tiny sigmas")


def _render_and_denoise(d, scene, params, frames, what, cfgs=((None, None),), **part):
    from oracle import pt_oracle
    _setup(d, scene, params, count=True, **part)
    for sd in _seeds(frames):
        d.render(dict(params, seed=sd))
    d.render_features(params)
    acc0 = d.read_accum()
    rays0 = d.stats().rays
    n, a = d.read_features()
    for it, demod in cfgs:
        d.denoise(iterations=it, demodulate=demod)
        D = d.read_denoised()
        k = device.denoise_cfg(iterations=it, demodulate=demod)
        ref = host.denoise_atrous(acc0, n, a, k.iterations, k.sigma_color, k.sigma_normal, k.sigma_depth, k.demodulate)
        _same(D, ref, f"{what} it={k.iterations} demod={k.demodulate}")
        for flip in (True, False):
            img = d.resolve_denoised_rgba8(2.2, flip)
            assert np.array_equal(img, pt_oracle.resolve(D, 2.2, flip)), f"{what}: resolve of D, flip {flip}"
    assert np.array_equal(_bits(d.read_accum()), _bits(acc0)) and d.stats().rays == rays0, f"{what}: the accumulator or the ray count moved"
    return acc0, D


def test_denoise_after_renders_c1(dev):
    scene, params = scenes.config_c1(256, 256, max_depth=4, subdiv=2)
    _render_and_denoise(dev, scene, params, 2, "c1 256^2", cfgs=((None, None), (1, 0), (2, 1), (3, 1), (6, 0)))


def test_denoise_after_renders_odd_size(dev):
    scene, params = scenes.config_c2(61, 37)
    _render_and_denoise(dev, scene, params, 1, "c2 61x37", cfgs=((None, None), (4, 0)))


def test_denoise_headline_1080p(dev):
    scene, params = scenes.config_headline(1920, 1080)
    _render_and_denoise(dev, scene, params, 1, "headline 1080p")


def test_denoise_partitioned(dev):
    scene, params = scenes.config_c1(100, 75, max_depth=4, subdiv=1)
    _render_and_denoise(dev, scene, params, 2, "rank 1/2", rank=1, world=2, stripe=8)
    dev.set_partition(0, 1, 16)


# ---- 3. what the calls leave alone, and what they refuse
def test_half_buffer_is_untouched(dev):
    scene, params = scenes.config_c1(64, 48, max_depth=4, subdiv=1)
    _setup(dev, scene, params)
    dev.render_adaptive(params, _seeds(4), -1.0, 2)
    half0, acc0 = dev.read_adaptive_half(), dev.read_accum()
    dev.render_features(params); dev.denoise(); dev.read_denoised(); dev.resolve_denoised_rgba8()
    assert np.array_equal(_bits(dev.read_adaptive_half()), _bits(half0)) and np.array_equal(_bits(dev.read_accum()), _bits(acc0))


def test_between_two_fed_bursts(dev, gpu_device):
    """A burst, features + denoise, a second burst: the accumulator is what the two bursts alone give (on a second context)."""
    scene, params = scenes.config_c1(128, 96, max_depth=4, subdiv=1)
    seeds = _seeds(12)
    _setup(dev, scene, params); _setup(gpu_device, scene, params)
    for sd in seeds[:6]:
        dev.render(dict(params, seed=sd)); gpu_device.render(dict(params, seed=sd))
    dev.render_features(params); dev.denoise()
    for sd in seeds[6:]:
        dev.render(dict(params, seed=sd)); gpu_device.render(dict(params, seed=sd))
    a, b = dev.read_accum(), gpu_device.read_accum()
    assert np.array_equal(_bits(a), _bits(b)) and (a[..., 3] == 12).all()
    D = dev.read_denoised()  # the image of the first burst's six frames
    assert (D[..., 3] == 1).all()


def test_refusals(dev):
    scene, params = scenes.config_c1(32, 32, max_depth=4, subdiv=1)
    d = device.Device()
    try:
        with pytest.raises(device.GlrtxError) as e:
            d.render_features(params)  # no scene
        assert e.value.code == -1
        d.upload_scene(scene)
        with pytest.raises(device.GlrtxError):
            d.render_features(params)  # no size
        d.resize(32, 32)
        with pytest.raises(device.GlrtxError) as e:
            d.denoise()  # no features yet
        assert e.value.code == -1 and "feature" in str(e.value)
        with pytest.raises(device.GlrtxError):
            d.read_denoised()
        d.render_features(params)
        with pytest.raises(device.GlrtxError):
            d.read_denoised()  # no result yet
        for bad in (dict(iterations=0), dict(iterations=7), dict(sigma_color=0.0), dict(sigma_depth=float("nan")), dict(sigma_normal=float("inf"))):
            with pytest.raises(device.GlrtxError):
                d.denoise(**bad)
        d.denoise(); d.read_denoised()
        d.resize(40, 24)  # the planes go with the old shape
        with pytest.raises(device.GlrtxError):
            d.denoise()
        d.upload_spheres(np.array([[0, 0, 0, 0.5, 0]], np.float32))
        with pytest.raises(device.GlrtxError) as e:
            d.render_features(params)
        assert e.value.code == -1 and "sphere" in str(e.value)
    finally:
        d.close()


# ---- 4. glrt_main --denoise
def test_glrt_main_denoise_writes_the_bindings_image(tmp_path, dev):
    """The scene and frames of tests/test_gpu_adaptive.py's facade test: glrt_main --denoise writes the binding's resolve of D (features before the first
    frame, the default configuration, or --denoise-iters), and without the flag it writes what the binding's plain resolve gives."""
    import subprocess
    from PIL import Image
    from conftest import PKG
    from test_gpu_adaptive import _c1_builder
    w, h, depth, frames = 96, 64, 4, 3
    b = _c1_builder()
    js = scenes.export_json_obj(b, tmp_path, w, h, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)

    def glrt_main(extra, name):
        out = tmp_path / name
        r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--frames-in-flight", "1",
                            "--out", str(out)] + extra, capture_output=True, text=True, timeout=120)
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
    for sd in _seeds(frames):
        dev.render(dict(params, seed=sd))
    plain = dev.resolve_rgba8(2.2, True)
    assert np.array_equal(glrt_main([], "plain.png"), plain)
    dev.denoise()
    ref = dev.resolve_denoised_rgba8(2.2, True)
    img = glrt_main(["--denoise"], "denoised.png")
    assert np.array_equal(img, ref), int((img != ref).any(-1).sum())
    assert not np.array_equal(img, plain)
    dev.denoise(iterations=2)
    assert np.array_equal(glrt_main(["--denoise", "--denoise-iters", "2"], "denoised2.png"), dev.resolve_denoised_rgba8(2.2, True))
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--denoise-iters", "3"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--denoise" in r.stderr
