"""The two things every render entry point shares since the launch path was restated: the accumulation pass (csrc/accumulate.hip.h: one template, six entry
points) and the helpings loop (render_helpings in csrc/glrtx.hip).  One small image through every form of the pass, bit for bit against ONE reference chain: a fresh
context under GLRTX_NO_PIPELINE=1 doing seven synchronous glrtx_render calls (the render kernel adds every sample to the accumulator itself: no pass at all).

Scene c2 at 200 x 41, 2 samples per pixel, depth 4, 7 seeds: the width is no multiple of 64 (the pass's wave), the rows no multiple of 4 (its workgroup) or 8, the
8 x 8 tiles are partial on both edges (the half buffer's mask), and 7 frames of 2 samples make the count's parity change inside every frame.  Under
GLRTX_FRAMES_BUDGET_MB=1 a frame's planes (2 x 41 rows x the pitch of 200 float4, ~260 KB) fit three times into the budget: the seven frames cannot go into
one launch at this size, so the width did not have to be raised.

glrtx_render_adaptive and glrtx_render_moments refuse to run while presentation is enabled (the ring has no form for them: GLRTX_EINVAL, nothing changes); with the
ring on, that refusal is what their cases pin."""
import numpy as np
import pytest

import adaptive_math as am
import variance_math as vm
from conftest import assert_bit_equal
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

W, H, SPP, DEPTH, FRAMES, RING = 200, 41, 2, 4, 7, 8
GAMMA, FLIP = 2.2, True
FORMS = ["fed", "planes", "stream", "adaptive", "moments"]


def _seeds():
    return [host.frame_seed(i) for i in range(FRAMES)]


def _setup(d, scene, params):
    d.set_variant(2); d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


@pytest.fixture(scope="module")
def ref(gpu_device):
    """The reference chain's accumulator and its resolve after every frame; and the 14 sample planes {rgb, 1} the statements of the half buffer and of M need.
    A frame's two samples are one chain of random numbers, so the second cannot be rendered alone: the first is a 1-sample frame into a cleared accumulator, the
    second a 2-sample frame into an accumulator that holds MINUS the first -- (-s0 + s0) + s1 is s1 exactly.  The planes are checked against the 2-sample frame."""
    import torch
    scene, params = scenes.CONFIGS["c2"](width=W, height=H, max_depth=DEPTH, n_samples=SPP)
    seeds = _seeds()
    mp = pytest.MonkeyPatch()
    mp.setenv("GLRTX_NO_PIPELINE", "1")
    try:
        d = device.Device()
    finally:
        mp.undo()
    try:
        _setup(d, scene, params)
        planes = []
        t = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        for sd in seeds:
            d.clear(); d.render(dict(params, seed=sd, n_samples=1)); s0 = d.read_accum()
            d.clear(); d.render(dict(params, seed=sd)); both = d.read_accum()
            t.copy_(torch.from_numpy(np.concatenate([-s0[..., :3], np.zeros((H, W, 1), np.float32)], -1)))
            torch.cuda.synchronize()
            d.bind_accum(t.data_ptr(), W * 16, H)
            try:
                d.render(dict(params, seed=sd)); d.sync()
                s1 = t.cpu().numpy().copy()
            finally:
                d.bind_accum(0, 0, 0)
            assert (s0[..., 3] == 1).all() and (s1[..., 3] == 2).all() and (both[..., 3] == 2).all()
            s1[..., 3] = 1
            assert_bit_equal(am._op(np.add, s0[..., :3], s1[..., :3]), both[..., :3], "the two sample planes of a frame against the frame")
            planes += [s0, s1]
        planes = np.stack(planes)
        d.clear(); d.reset_stats()
        images = []
        for sd in seeds:
            d.render(dict(params, seed=sd)); d.sync()
            images.append(d.resolve_rgba8(GAMMA, FLIP))
        acc = d.read_accum()
        assert d.stats().feed_appended == 0
    finally:
        d.close()
    zero = np.zeros((H, W, 4), np.float32)
    acc2, half = am.accumulate(zero, zero, planes, np.ones(am.tiles_of(H, W), np.uint8))
    assert_bit_equal(acc2, acc, "adaptive_math's chain against the reference chain")
    return dict(scene=scene, params=params, seeds=seeds, acc=acc, images=images, half=half, moments=vm.fold_moments(zero, planes))


def _run(d, form, ref, monkeypatch):
    """One call of seven frames in the given form; returns the torch stream to keep alive (or None)."""
    params, seeds = ref["params"], ref["seeds"]
    stream = None
    if form == "planes":
        monkeypatch.setenv("GLRTX_NO_FEED", "1")
    if form == "stream":
        import torch
        stream = torch.cuda.Stream()
        d.set_stream(stream.cuda_stream)
    if form == "adaptive":
        d.render_adaptive(params, seeds, -1.0, 2)
    elif form == "moments":
        d.track_moments(True)
        d.render_moments(params, seeds)
    else:
        d.render_frames(params, seeds)
    return stream


def _check_side_buffers(d, form, ref):
    if form == "adaptive":
        active, total = d.adaptive_active_tiles()
        assert active == total == ((W + 7) // 8) * ((H + 7) // 8)
        assert_bit_equal(d.read_adaptive_half(), ref["half"], "half buffer against adaptive_math.accumulate")
    if form == "moments":
        assert_bit_equal(d.read_moments(), ref["moments"], "M against variance_math.fold_moments")


@pytest.mark.parametrize("ring", [0, RING])
@pytest.mark.parametrize("form", FORMS)
def test_every_form_of_the_pass_is_the_reference_chain(gpu_device, ref, monkeypatch, form, ring):
    d = device.Device()
    stream = None
    try:
        _setup(d, ref["scene"], ref["params"])
        if ring:
            d.present_enable(ring, GAMMA, FLIP)
        if ring and form in ("adaptive", "moments"):  # (refused while presenting: nothing changes)
            with pytest.raises(device.GlrtxError) as e:
                _run(d, form, ref, monkeypatch)
            assert "presentation is enabled" in str(e.value)
            assert not d.read_accum().any() and d.present_stats().pending == 0
            return
        stream = _run(d, form, ref, monkeypatch)
        if ring:
            for k in range(FRAMES):
                img = d.present_acquire(wait=True)
                assert img.frame == k + 1
                assert np.array_equal(img.rgba, ref["images"][k]), (form, k)
                d.present_release(img)
            assert d.present_stats().pending == 0
        assert_bit_equal(d.read_accum(), ref["acc"], f"{form}, ring {ring}: accumulator")
        _check_side_buffers(d, form, ref)
        st = d.stats()
        assert st.launches == FRAMES and st.device_error_pending == 0
        if form == "fed":
            assert st.feed_launches >= 1
        else:
            assert st.feed_launches == 0
    finally:
        if ring:
            d.present_enable(0)
        d.set_stream(None)
        d.close()
        del stream


@pytest.mark.parametrize("form", ["fed", "planes", "adaptive", "moments"])
def test_helpings_split_a_call_and_keep_the_chain(gpu_device, ref, monkeypatch, form):
    """GLRTX_FRAMES_BUDGET_MB=1: the seven frames do not fit one launch, the helpings loop issues several, and the result is the same chain."""
    monkeypatch.setenv("GLRTX_FRAMES_BUDGET_MB", "1")
    d = device.Device()
    try:
        _setup(d, ref["scene"], ref["params"])
        _run(d, form, ref, monkeypatch)
        assert_bit_equal(d.read_accum(), ref["acc"], f"{form}, 1 MB budget: accumulator")
        _check_side_buffers(d, form, ref)
        d.sync()
        st = d.stats()
        print(f"{form}: {st.kernel_launches} kernel launches for {st.launches} frames")
        assert st.kernel_launches > 1 and st.launches == FRAMES and st.device_error_pending == 0
    finally:
        d.close()
