"""Tone mapping on the GPU (csrc/tonemap.hip.h; include/glrtx.h "Tone mapping"), every word and byte against the CPU statement (host/tonemap.cpp) and the numpy
statement (tests/tonemap_math.py): the kernels on hostile arrays; the flat image that puts a wave on one LDS counter; the context calls after real renders, from the
accumulator and from the denoised image; op 0 as the plain resolve; a measure / render / measure / resolve train without syncs; what the calls leave alone; a
partitioned context; the refusals."""
import numpy as np
import pytest

import tonemap_math as tm
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

OPS = (0, 1, 2)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


def _same_exposure(e, want, what):
    assert np.array_equal(np.ctypeslib.as_array(e.hist), want["hist"]), f"{what}: histogram"
    assert (int(e.counted), int(e.kept)) == (want["counted"], want["kept"]), f"{what}: counted / kept"
    for k in ("mean_log2", "target", "exposure"):
        assert _bits(np.float32(getattr(e, k))) == _bits(want[k]), f"{what}: {k} {getattr(e, k)} vs {want[k]}"


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, rank=0, world=1, stripe=16):
    d.set_variant(2); d.count_rays(True)
    d.upload_scene(scene); d.set_partition(rank, world, stripe); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()
    d.exposure_reset()


# ---- 1. the kernels on host arrays.  67 x 13: the hostile array of the host tests; 131 x 9: a row ends inside a wave, and 131 is no multiple of 64 * PER for
# the resolve's PER = 2 or the histogram's 4; 300 x 5: more than one histogram segment a row.
@pytest.fixture(scope="module")
def arrays():
    return {(13, 67): tm.hostile_array(13, 67, 19), (9, 131): tm.hostile_array(9, 131, 23), (5, 300): tm.hostile_array(5, 300, 29)}


@pytest.mark.parametrize("shape", [(13, 67), (9, 131), (5, 300)])
def test_debug_tonemap_on_hostile_arrays(gpu_device, arrays, shape):
    a = arrays[shape]
    for prev, low, high, adapt in ((None, 500, 950, 1.0), (0.37, 0, 1000, 0.25), (2.5, 999, 1000, 0.5)):
        want = host.exposure_measure(a, prev, key=0.18, low_permille=low, high_permille=high, adapt=adapt)
        for op in OPS:
            for auto in (0, 1):
                for flip in (0, 1):
                    kw = dict(op=op, auto_exposure=auto, exposure=1.7, white=3.0, gamma=2.2, flip_y=flip)
                    e, T, b = device.debug_tonemap(a, prev, low_permille=low, high_permille=high, adapt=adapt, **kw)
                    what = f"{shape} prev={prev} window={low}/{high} op={op} auto={auto} flip={flip}"
                    _same_exposure(e, want, what)
                    assert e.measurements == 1
                    rT, rb = host.tonemap(a, E=want["exposure"], **kw)
                    assert np.array_equal(_bits(T), _bits(rT)), f"{what}: T differs on {int((_bits(T) != _bits(rT)).any(-1).sum())} pixels"
                    assert np.array_equal(b, rb), f"{what}: bytes differ on {int((b != rb).any(-1).sum())} pixels"


# ---- 2. one flat colour: every lane of every wave on one LDS counter
def test_a_flat_image_fills_one_bin(gpu_device):
    a = np.empty((64, 256, 4), np.float32)
    a[...] = (0.9, 0.6, 0.3, 2.0)
    e, _, _ = device.debug_tonemap(a)
    h = np.ctypeslib.as_array(e.hist)
    assert np.count_nonzero(h) == 1 and int(h.max()) == 16384 and int(e.counted) == 16384
    _same_exposure(e, host.exposure_measure(a), "flat 256x64")
    a[3, 77] = (9.0, 6.0, 3.0, 2.0)  # one lane elsewhere: that wave leaves the one-add path
    e, _, _ = device.debug_tonemap(a)
    h = np.ctypeslib.as_array(e.hist)
    assert sorted(h[h > 0].tolist()) == [1, 16383]
    _same_exposure(e, host.exposure_measure(a), "flat 256x64 with one other pixel")


# ---- 3, 4, 6. after real renders: accumulator and denoised image as sources; op 0 as the plain resolve; nothing else moves
def _check_context_calls(d, scene, params, frames, what):
    _setup(d, scene, params)
    d.render_frames(params, _seeds(frames))
    d.render_features(params)
    d.denoise()
    acc0, D0, rays0 = d.read_accum(), d.read_denoised(), d.stats().rays
    plain = d.resolve_rgba8(2.2, True)
    assert (acc0[..., 3] == frames).all() and np.isfinite(acc0).all()
    prev = None
    for source, src in ((0, acc0), (1, D0)):
        for op in OPS:
            cfg = dict(op=op, source=source, auto_exposure=1, exposure=1.3, adapt=0.5)
            d.exposure_measure(**cfg)
            want = tm.measure(src, prev, adapt=0.5)
            prev = want["exposure"]
            d.tonemap(**cfg)
            e, T = d.read_exposure(), d.read_tonemapped()
            _same_exposure(e, want, f"{what} source={source} op={op}")
            assert np.array_equal(_bits(T), _bits(tm.tonemap(src, E=want["exposure"], **cfg))), f"{what} source={source} op={op}: T"
            for flip in (1, 0):
                b = d.resolve_tonemapped_rgba8(flip_y=flip, **cfg)
                assert np.array_equal(b, pt_oracle.resolve(T, 2.2, bool(flip))), f"{what} source={source} op={op} flip={flip}: bytes"
    assert d.read_exposure().measurements == 6
    assert np.array_equal(d.resolve_tonemapped_rgba8(op=0, exposure=1.0, auto_exposure=0), plain), f"{what}: op 0 at exposure 1 is not the plain resolve"
    assert np.array_equal(d.resolve_tonemapped_rgba8(op=0, exposure=1.0, auto_exposure=0, flip_y=0), d.resolve_rgba8(2.2, False))
    assert np.array_equal(_bits(d.read_accum()), _bits(acc0)) and np.array_equal(_bits(d.read_denoised()), _bits(D0)), f"{what}: the accumulator or D moved"
    assert d.stats().rays == rays0, f"{what}: the ray count moved"


def test_context_calls_after_c1(dev):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    _check_context_calls(dev, scene, params, 4, "c1 96x64, 4 frames")


def test_context_calls_after_headline(dev):
    scene, params = scenes.config_headline(192, 108)
    _check_context_calls(dev, scene, params, 1, "headline 192x108, 1 frame")


# ---- 5. measure, render, measure, resolve back to back
def test_a_train_without_syncs_is_the_train_with_them(dev):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    cfg = dict(op=2, auto_exposure=1, adapt=0.25)
    out = {}
    for synced in (False, True):
        _setup(dev, scene, params)
        step = (lambda: dev.sync()) if synced else (lambda: None)
        dev.render_frames(params, _seeds(2)); step()
        acc_a = dev.read_accum() if synced else None
        dev.exposure_measure(**cfg); step()
        e_a = dev.read_exposure() if synced else None
        dev.render_frames(params, _seeds(2, 2)); step()
        dev.exposure_measure(**cfg); step()
        out[synced] = (dev.resolve_tonemapped_rgba8(**cfg), dev.read_exposure(), dev.read_accum())
        if synced:
            m1 = tm.measure(acc_a, None, adapt=0.25)
            _same_exposure(e_a, m1, "first measurement")
            m2 = tm.measure(out[True][2], m1["exposure"], adapt=0.25)
            _same_exposure(out[True][1], m2, "second measurement")
            assert m2["exposure"] != m2["target"]
            assert np.array_equal(out[True][0], pt_oracle.resolve(tm.tonemap(out[True][2], E=m2["exposure"], **cfg), 2.2, True))
    assert np.array_equal(out[False][0], out[True][0])
    assert bytes(out[False][1]) == bytes(out[True][1]) and out[True][1].measurements == 2
    assert np.array_equal(_bits(out[False][2]), _bits(out[True][2]))


def test_reset_forgets_the_exposure(dev):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    _setup(dev, scene, params)
    assert dev.read_exposure().measurements == 0
    # before any measurement E counts as 1: auto exposure changes nothing
    dev.render_frames(params, _seeds(1))
    assert np.array_equal(dev.resolve_tonemapped_rgba8(op=1, auto_exposure=1), dev.resolve_tonemapped_rgba8(op=1, auto_exposure=0))
    dev.exposure_measure(adapt=0.25); dev.exposure_measure(adapt=0.25)
    assert dev.read_exposure().measurements == 2
    dev.exposure_reset()
    e = dev.read_exposure()
    assert e.measurements == 0 and e.counted == 0 and not np.ctypeslib.as_array(e.hist).any()
    dev.exposure_measure(adapt=0.25)
    e = dev.read_exposure()
    assert e.measurements == 1 and e.exposure == e.target


# ---- 7. a partitioned context: its own rows
def test_a_partitioned_context_works_on_its_owned_rows(dev):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    _setup(dev, scene, params, rank=1, world=3, stripe=8)
    dev.render_frames(params, _seeds(2))
    acc = dev.read_accum()
    assert acc.shape == (24, 96, 4)  # stripes 1, 4, 7
    cfg = dict(op=1, auto_exposure=1, exposure=0.8)
    dev.exposure_measure(**cfg); dev.tonemap(**cfg)
    want = tm.measure(acc)
    _same_exposure(dev.read_exposure(), want, "rank 1 of 3")
    T = dev.read_tonemapped()
    assert np.array_equal(_bits(T), _bits(tm.tonemap(acc, E=want["exposure"], **cfg)))
    for flip in (1, 0):
        assert np.array_equal(dev.resolve_tonemapped_rgba8(flip_y=flip, **cfg), pt_oracle.resolve(T, 2.2, bool(flip)))
    dev.set_partition(0, 1, 16)


# ---- 8. refusals
def test_refusals_leave_the_context_usable(dev):
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    _setup(dev, scene, params)  # (the resize released every denoised image)
    dev.render_frames(params, _seeds(1))
    before = dev.resolve_tonemapped_rgba8(op=2)
    bad = [dict(source=1), dict(low_permille=950, high_permille=500), dict(low_permille=500, high_permille=500), dict(high_permille=1001), dict(exposure=0.0),
           dict(exposure=-1.0), dict(exposure=float("nan")), dict(adapt=0.0), dict(adapt=1.5), dict(adapt=float("nan")), dict(op=3), dict(source=2), dict(key=0.0),
           dict(white=0.0), dict(gamma=0.0)]
    for b in bad:
        for call in (dev.exposure_measure, dev.tonemap, dev.resolve_tonemapped_rgba8):
            with pytest.raises(device.GlrtxError) as e:
                call(**b)
            assert e.value.code == device.GLRTX_EINVAL and "glrtx_" in str(e.value), b
    with pytest.raises(device.GlrtxError):
        dev.read_tonemapped()  # (no glrtx_tonemap yet at this shape)
    assert dev.read_exposure().measurements == 0
    assert np.array_equal(dev.resolve_tonemapped_rgba8(op=2), before)
    dev.render_features(params); dev.denoise()
    dev.exposure_measure(source=1); dev.tonemap(source=1)
    assert np.array_equal(_bits(dev.read_tonemapped()), _bits(tm.tonemap(dev.read_denoised())))
