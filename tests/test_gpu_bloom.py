"""Bloom on the GPU (csrc/bloom.hip.h; include/glrtx.h "Bloom"), every word against the CPU statement (host/bloom.cpp) and the numpy statement
(tests/bloom_math.py): the kernels on hostile arrays whose levels lie inside one partial tile, and on one that crosses tile edges at several levels; the three
properties the header derives; the context calls after a real render, from the accumulator and from the denoised image; B through the tone curve; a measure /
bloom / resolve train without syncs; what the calls leave alone; the refusals."""
import numpy as np
import pytest

import bloom_math as bm
import tonemap_math as tm
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

# The host test's sizes, plus 150 x 70: its level 1 is 75 x 35, five by three of the down pass's 16 x 16 tiles and two by nine of the up pass's 64 x 4 ones, and
# levels 2 (38 x 18) and 3 (19 x 9) cross a down tile's edge again; level 0 crosses the up pass's 64-column edge twice.
SIZES = bm.SIZES + [(70, 150)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


@pytest.fixture(scope="module")
def arrays():
    return {s: bm.hostile(s[0], s[1], 19 + i) for i, s in enumerate(SIZES)}


@pytest.fixture(scope="module")
def statements(arrays):
    """The CPU statement's (d, B) per (shape, levels, threshold, strength), computed once; the numpy statement is checked against it where it is computed."""
    cache = {}

    def get(shape, levels, threshold, strength):
        key = (shape, levels, threshold, strength)
        if key not in cache:
            cache[key] = host.bloom(arrays[shape], threshold, strength, levels)
        return cache[key]
    return get


# ---- 1. the kernels on host arrays
@pytest.mark.parametrize("levels", bm.LEVELS)
@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_debug_bloom_on_hostile_arrays(gpu_device, arrays, statements, shape, levels):
    a = arrays[shape]
    for threshold, strength in ((1.0, 0.25), (0.0, 4.0)):
        d, B = device.debug_bloom(a, threshold=threshold, strength=strength, levels=levels)
        rd, rB = statements(shape, levels, threshold, strength)
        what = f"{shape[1]}x{shape[0]} levels={levels} threshold={threshold} strength={strength}"
        assert d.shape == rd.shape
        assert np.array_equal(_bits(d), _bits(rd)), f"{what}: D differs from glrt_bloom on {int((_bits(d) != _bits(rd)).any(-1).sum())} texels"
        assert np.array_equal(_bits(B), _bits(rB)), f"{what}: B differs from glrt_bloom on {int((_bits(B) != _bits(rB)).any(-1).sum())} pixels"
    nd, nB = bm.bloom(a, threshold, strength, levels)  # (the last pair: the host test holds glrt_bloom to the numpy statement on every pair)
    assert np.array_equal(_bits(d), _bits(nd)) and np.array_equal(_bits(B), _bits(nB)), f"{what}: differs from the numpy statement"


# ---- 2. the three properties, on the device
@pytest.mark.parametrize("shape", SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_properties_on_the_device(gpu_device, arrays, shape):
    flat = np.empty(shape + (4,), np.float32)
    flat[...] = (0.5, 0.5, 0.5, 1.0)
    for levels in (1, 2, 4, 8):
        d, B = device.debug_bloom(flat, threshold=0.0, strength=1.0, levels=levels)
        assert (_bits(d[:, :3]) == _bits(np.float32(0.5))).all() and (d[:, 3] == 0).all(), f"levels={levels}: a level is not 0.5 everywhere"
        assert (_bits(B) == _bits(np.float32(1.0))).all(), f"levels={levels}: B is not 1.0f on {int((B != 1).any(-1).sum())} pixels"
    a = arrays[shape]
    x = bm.pixel_value(a)
    _, B = device.debug_bloom(a, threshold=1.0, strength=0.0, levels=5)
    assert np.array_equal(_bits(B[..., :3]), _bits(x)) and (B[..., 3] == 1).all()
    d, B = device.debug_bloom(a, threshold=1.0e5, strength=4.0, levels=5)
    assert not d.any() and np.array_equal(_bits(B[..., :3]), _bits(x))
    h = a.copy()
    h[0, 0] = (3e38, np.nan, np.inf, 1.0)
    d, B = device.debug_bloom(h, threshold=0.0, strength=4.0, levels=8)
    assert np.isfinite(d).all() and np.isfinite(B).all() and (B[..., :3] >= 0).all()


# ---- 3. the context calls after a real render of the headline, from both sources
def _setup(d, scene, params):
    d.set_variant(2); d.count_rays(True)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()
    d.exposure_reset()


@pytest.fixture(scope="module")
def headline(dev):
    scene, params = scenes.config_headline(192, 108)
    _setup(dev, scene, params)
    dev.render_frames(params, _seeds(2))
    dev.render_features(params)
    dev.denoise()
    return dict(params=params, acc=dev.read_accum(), D=dev.read_denoised(), rays=dev.stats().rays)


def test_context_calls_after_the_headline(dev, headline):
    acc0, D0 = headline["acc"], headline["D"]
    assert acc0.shape == (108, 192, 4) and np.isfinite(acc0).all()
    assert (bm.lum(bm.pixel_value(acc0)) > 1.0).any()  # (the headline's emitters: something glows at the default threshold)
    plain = {flip: dev.resolve_tonemapped_rgba8(op=2, exposure=1.3, flip_y=flip) for flip in (1, 0)}
    for source, src in ((0, acc0), (1, D0)):
        bcfg = dict(source=source, threshold=0.8, strength=0.5, levels=5)
        dev.exposure_reset()
        dev.exposure_measure(source=source)
        E = tm.measure(src)["exposure"]
        dev.bloom(**bcfg)
        B = dev.read_bloomed()
        _, want = bm.bloom(src, **bcfg)
        assert np.array_equal(_bits(B), _bits(want)), f"source={source}: B differs from the numpy statement on {int((_bits(B) != _bits(want)).any(-1).sum())} pixels"
        assert (B[..., :3] > bm.pixel_value(src)).any()
        for op in (0, 1, 2):
            tcfg = dict(op=op, auto_exposure=1, exposure=1.3, source=2)  # (the source is not read: 2 is refused everywhere else)
            dev.tonemap_bloomed(**tcfg)
            T = dev.read_tonemapped()
            assert np.array_equal(_bits(T), _bits(tm.tonemap(B, E=E, **tcfg))), f"source={source} op={op}: T"
            for flip in (1, 0):
                b = dev.resolve_bloomed_rgba8(flip_y=flip, **tcfg)
                assert np.array_equal(b, pt_oracle.resolve(T, 2.2, bool(flip))), f"source={source} op={op} flip={flip}: bytes"
    # strength 0: B is x, and the bloomed resolve is the tone-mapping resolve of the source
    dev.bloom(source=0, strength=0.0)
    for flip in (1, 0):
        assert np.array_equal(dev.resolve_bloomed_rgba8(op=2, exposure=1.3, flip_y=flip), plain[flip]), "strength 0 is not glrtx_resolve_tonemapped_rgba8's image"
    assert np.array_equal(_bits(dev.read_accum()), _bits(acc0)) and np.array_equal(_bits(dev.read_denoised()), _bits(D0)), "the accumulator or D moved"
    assert dev.stats().rays == headline["rays"], "the ray count moved"


def test_bloom_leaves_t_and_the_moments_alone(dev):
    scene, params = scenes.config_headline(192, 108)
    _setup(dev, scene, params)
    dev.track_moments(True)
    try:
        dev.render_moments(params, _seeds(2))
        dev.tonemap(op=1)
        acc0, M0, T0, rays0 = dev.read_accum(), dev.read_moments(), dev.read_tonemapped(), dev.stats().rays
        dev.bloom(levels=8, strength=1.0, threshold=0.5)
        B = dev.read_bloomed()
        assert np.array_equal(_bits(B), _bits(bm.bloom(acc0, levels=8, strength=1.0, threshold=0.5)[1]))
        assert np.array_equal(_bits(dev.read_accum()), _bits(acc0)) and np.array_equal(_bits(dev.read_moments()), _bits(M0))
        assert np.array_equal(_bits(dev.read_tonemapped()), _bits(T0)) and dev.stats().rays == rays0
    finally:
        dev.track_moments(False)


# ---- 4. measure, bloom, resolve back to back
def test_a_train_without_syncs_is_the_train_with_them(dev):
    scene, params = scenes.config_headline(192, 108)
    tcfg, bcfg = dict(op=2, auto_exposure=1, adapt=0.25), dict(threshold=0.8, strength=0.5, levels=5)
    out = {}
    for synced in (False, True):
        _setup(dev, scene, params)
        step = (lambda: dev.sync()) if synced else (lambda: None)
        dev.render_frames(params, _seeds(1)); step()
        dev.exposure_measure(**tcfg); step()
        dev.bloom(**bcfg); step()
        dev.render_frames(params, _seeds(1, 1)); step()
        dev.exposure_measure(**tcfg); step()
        dev.bloom(**bcfg); step()
        out[synced] = (dev.resolve_bloomed_rgba8(**tcfg), dev.read_bloomed(), dev.read_exposure(), dev.read_accum())
    assert np.array_equal(out[False][0], out[True][0])
    assert np.array_equal(_bits(out[False][1]), _bits(out[True][1]))
    assert bytes(out[False][2]) == bytes(out[True][2]) and out[True][2].measurements == 2
    acc = out[True][3]
    B = bm.bloom(acc, **bcfg)[1]
    assert np.array_equal(_bits(out[True][1]), _bits(B))
    assert np.array_equal(out[True][0], pt_oracle.resolve(tm.tonemap(B, E=np.float32(out[True][2].exposure), **tcfg), 2.2, True))


# ---- 5. refusals
def test_b_is_refused_after_a_resize_until_bloom_runs_again(dev):
    scene, params = scenes.config_headline(192, 108)
    _setup(dev, scene, params)
    dev.render_frames(params, _seeds(1))
    dev.bloom()
    assert dev.read_bloomed().shape == (108, 192, 4)
    dev.resize(96, 64)
    for call in (dev.read_bloomed, dev.tonemap_bloomed, dev.resolve_bloomed_rgba8):
        with pytest.raises(device.GlrtxError) as e:
            call()
        assert e.value.code == device.GLRTX_EINVAL and "glrtx_bloom first" in str(e.value)
    dev.clear()
    dev.bloom()
    assert dev.read_bloomed().shape == (64, 96, 4)
    assert dev.resolve_bloomed_rgba8().shape == (64, 96, 4)


def test_refusals_leave_the_context_usable(dev):
    scene, params = scenes.config_headline(192, 108)
    _setup(dev, scene, params)  # (the resize released every denoised image, and B)
    dev.render_frames(params, _seeds(1))
    with pytest.raises(device.GlrtxError):
        dev.read_bloomed()  # (no glrtx_bloom yet at this shape)
    dev.bloom()
    before = dev.read_bloomed()
    bad = [dict(source=1), dict(source=2), dict(source=-1), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(strength=-1.0),
           dict(strength=2.0e4), dict(strength=float("nan")), dict(levels=0), dict(levels=9)]
    for b in bad:
        with pytest.raises(device.GlrtxError) as e:
            dev.bloom(**b)
        assert e.value.code == device.GLRTX_EINVAL and "glrtx_bloom" in str(e.value), b
    for b in (dict(op=3), dict(exposure=0.0), dict(gamma=0.0), dict(white=0.0)):  # the tone-mapping cfg's own checks stand
        for call in (dev.tonemap_bloomed, dev.resolve_bloomed_rgba8):
            with pytest.raises(device.GlrtxError):
                call(**b)
    with pytest.raises(device.GlrtxError):
        dev.tonemap(source=2)  # (still a refusal: the bloomed calls are the way to B)
    assert np.array_equal(_bits(dev.read_bloomed()), _bits(before))
    # a partitioned context: a seam per stripe would be wrong
    dev.set_partition(1, 3, 8)
    try:
        dev.clear()
        dev.render_frames(params, _seeds(1))
        with pytest.raises(device.GlrtxError) as e:
            dev.bloom()
        assert e.value.code == device.GLRTX_EINVAL and "partitioned" in str(e.value)
    finally:
        dev.set_partition(0, 1, 16)
    dev.clear()
    dev.render_frames(params, _seeds(1))
    dev.render_features(params); dev.denoise()
    dev.bloom(source=1)
    assert np.array_equal(_bits(dev.read_bloomed()), _bits(bm.bloom(dev.read_denoised())[1]))
