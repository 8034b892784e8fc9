"""Firefly re-weighting on the GPU (csrc/reweight.hip.h, the Cascades sink of csrc/accumulate.hip.h), all bit for bit against the CPU statements
(host/reweight.cpp) and the numpy statement (tests/reweight_math.py): the fold and the resolve on hostile arrays; glrtx_render_cascades' accumulator is
glrtx_render_frames' and its C is glrt_fold_cascades of the oracle's frames; glrtx_reweight is glrt_reweight of C; D flows on into the resolve, the tone curve
and the bloom; C's lifecycle; the refusals; with tracking off nothing else changes."""
import numpy as np
import pytest

import reweight_math as rw
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

SIZES = [(37, 61), (16, 16), (17, 33), (5, 130), (1, 1), (70, 49)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what, nan_payloads=True):
    bad = _bits(got) != _bits(ref)
    if not nan_payloads:
        bad &= ~(np.isnan(got) & np.isnan(ref))
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} values differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}"


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, track=True, start=None):
    d.set_variant(2); d.count_rays(False)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()
    d.track_cascades(track, start)


@pytest.fixture(scope="module")
def headline():
    """The headline scene at 64x48, max_depth 4, and the oracle's five per-frame images (computed once, read-only)."""
    from oracle import pt_oracle
    scene, params = scenes.config_headline(64, 48)
    params = dict(params, max_depth=4)
    seeds = _seeds(5)
    frames = np.stack([pt_oracle.render(scene, dict(params, seed=sd))[0] for sd in seeds])
    frames.setflags(write=False)
    return scene, params, seeds, frames


# ---- 1. the kernels on hostile arrays: width 130 gives the fold three waves a row; 17 and 33 cross the resolve's tile edge; 1x1 has no neighbour
@pytest.mark.parametrize("rows,width", SIZES)
def test_debug_fold_cascades_on_hostile_arrays(gpu_device, rows, width):
    for start in (1.0, 0.375, 2.0 ** 20):
        v = rw.hostile_samples(5, rows, width, rows * 1000 + width, start)
        C0 = rw.hostile_cascades(rows, width, rows * 7 + width)
        acc0 = (C0[0] + C0[1]).astype(np.float32)
        for C_in, acc_in in ((np.zeros_like(C0), np.zeros_like(acc0)), (C0, acc0)):
            ga, gc = device.debug_fold_cascades(acc_in, C_in, v, start)
            rc, ra = rw.fold_cascades(C_in, acc_in, v, start)
            _same(gc, rc, f"C {width}x{rows} start {start}", nan_payloads=False)
            _same(ga, ra, f"accumulator {width}x{rows} start {start}", nan_payloads=False)
    ga, gc = device.debug_fold_cascades(acc0, C0, v[:0], 1.0)  # no frames: nothing changes
    assert np.array_equal(_bits(ga), _bits(acc0)) and np.array_equal(_bits(gc), _bits(C0))


@pytest.mark.parametrize("rows,width", SIZES)
def test_debug_reweight_on_hostile_arrays(gpu_device, rows, width):
    v = rw.hostile_samples(4, rows, width, rows * 1000 + width + 1)
    planes = [rw.hostile_cascades(rows, width, rows * 1000 + width), host.fold_cascades(None, v),
              host.fold_cascades(rw.hostile_cascades(rows, width, rows * 31 + width), v)]
    for i, C in enumerate(planes):
        for kappa in (4.0, 1.0, 0.3, 1e-38, 3e38):
            _same(device.debug_reweight(C, kappa=kappa), rw.reweight(C, kappa), f"D {width}x{rows} planes {i} kappa {kappa}")


def test_consequence_2_on_the_device(gpu_device):
    v = np.full((9, 5, 5, 4), 0.5, np.float32)
    v[..., 3] = 1
    v[8, 2, 2, :3] = 5000.0
    acc, C = device.debug_fold_cascades(np.zeros((5, 5, 4), np.float32), np.zeros((6, 5, 5, 4), np.float32), v, 1.0)
    assert C[:, 2, 2, 3].tolist() == [8, 0, 0, 0, 1, 0] and (acc[..., 3] == 9).all()
    D = device.debug_reweight(C, kappa=4.0)
    assert (_bits(D[2, 2, :3]) == _bits(np.float32(4.0) / np.float32(9.0))).all()
    others = np.ones((5, 5), bool)
    others[2, 2] = False
    assert (D[others][:, :3] == np.float32(0.5)).all() and (D[..., 3] == 1).all()


# ---- 2. render_cascades and reweight after real renders
@pytest.mark.parametrize("split", [(5,), (2, 3)])
def test_render_cascades_and_reweight_on_the_headline(dev, gpu_device, headline, split):
    scene, params, seeds, frames = headline
    _setup(dev, scene, params)
    f0 = 0
    for n in split:
        dev.render_cascades(params, seeds[f0:f0 + n]); f0 += n
    acc, C = dev.read_accum(), dev.read_cascades()
    _setup(gpu_device, scene, params, track=False)
    gpu_device.render_frames(params, seeds)
    _same(acc, gpu_device.read_accum(), "render_cascades' accumulator against render_frames'")
    ref_c, ref_acc = host.fold_cascades(None, frames, accum=np.zeros_like(frames[0]))
    _same(acc, ref_acc, "the accumulator against the oracle's frames")
    _same(C, ref_c, "C against glrt_fold_cascades of the oracle's five frames")
    assert (C[..., 3].sum(0) == 5).all() and C[1:, ..., 3].any()
    for kappa in (None, 1.0, 16.0):
        dev.reweight(kappa=kappa)
        _same(dev.read_denoised(), host.reweight(C, 4.0 if kappa is None else kappa), f"reweight, kappa {kappa}")
    assert np.array_equal(_bits(dev.read_accum()), _bits(acc)) and np.array_equal(_bits(dev.read_cascades()), _bits(C)), "reweight moved the accumulator or C"


def test_consequence_1_with_every_sample_below_start(dev, headline):
    scene, params, seeds, frames = headline
    _setup(dev, scene, params, start=2.0 ** 20)  # (a sample is at most 100 per channel)
    dev.render_cascades(params, seeds)
    acc, C = dev.read_accum(), dev.read_cascades()
    assert np.array_equal(_bits(C[0]), _bits(acc)) and not C[1:].any()
    dev.reweight()
    D = dev.read_denoised()
    _same(D[..., :3], (acc[..., :3] / acc[..., 3:4]).astype(np.float32), "D against the plain mean")
    assert (D[..., 3] == 1).all()


# ---- 3. D flows on
def test_d_flows_into_the_resolve_the_tone_curve_and_the_bloom(dev, headline):
    from oracle import pt_oracle
    scene, params, seeds, frames = headline
    fresh = device.Device()
    try:
        _setup(fresh, scene, params)
        fresh.render_cascades(params, seeds[:1])
        for call in (lambda: fresh.tonemap(source=1), lambda: fresh.bloom(source=1), fresh.read_denoised, fresh.resolve_denoised_rgba8,
                     lambda: fresh.exposure_measure(source=1)):
            with pytest.raises(device.GlrtxError) as e:  # nothing wrote D yet
                call()
            assert e.value.code == -1
    finally:
        fresh.close()
    _setup(dev, scene, params)
    dev.render_cascades(params, seeds)
    dev.reweight()
    ref = host.reweight(host.fold_cascades(None, frames))
    _same(dev.read_denoised(), ref, "D")
    for flip in (True, False):
        assert np.array_equal(dev.resolve_denoised_rgba8(2.2, flip), pt_oracle.resolve(ref, 2.2, flip)), f"resolve of D, flip {flip}"
    dev.tonemap(source=1, op=2)
    _same(dev.read_tonemapped(), host.tonemap(ref, op=2)[0], "tonemap(source = 1)")
    assert np.array_equal(dev.resolve_tonemapped_rgba8(source=1, op=1), host.tonemap(ref, op=1)[1])
    dev.bloom(source=1, threshold=0.5)
    _same(dev.read_bloomed(), host.bloom(ref, threshold=0.5)[1], "bloom(source = 1)")
    dev.resize(params["width"], params["height"])  # a resize drops D, as it always did
    with pytest.raises(device.GlrtxError):
        dev.tonemap(source=1)
    with pytest.raises(device.GlrtxError):
        dev.read_denoised()


# ---- 4. C's lifecycle
def test_lifecycle_of_c(dev):
    import reproject_math as rm
    scene, params = scenes.config_c1(40, 24, max_depth=4, subdiv=1)
    _setup(dev, scene, params)
    assert dev.read_cascades().shape == (6, 24, 40, 4) and not dev.read_cascades().any()  # first use: zeros
    dev.render_cascades(params, [])  # no frames: only allocates
    assert not dev.read_cascades().any() and not dev.read_accum().any()
    dev.render_cascades(params, _seeds(2))
    assert (dev.read_cascades()[..., 3].sum(0) == 2).all()
    dev.clear()
    assert not dev.read_cascades().any() and not dev.read_accum().any()
    dev.render_cascades(params, _seeds(1))
    dev.track_cascades(False); dev.track_cascades(True)
    assert not dev.read_cascades().any() and (dev.read_accum()[..., 3] == 1).all()
    dev.render_cascades(params, _seeds(1))
    dev.track_cascades(True, 1.0)  # the same start: C stays
    assert (dev.read_cascades()[..., 3].sum(0) == 1).all()
    dev.track_cascades(True, 0.5)  # another start: zeroed
    assert not dev.read_cascades().any() and (dev.read_accum()[..., 3] == 2).all()
    dev.render_cascades(params, _seeds(1))
    dev.render_features(params)
    dev.reproject(rm.move_camera(params, "orbit", 3.0))  # the bins belong to the old pixel grid
    assert not dev.read_cascades().any() and dev.read_accum()[..., 3].any()
    dev.track_cascades(True, 1.0)
    dev.render_cascades(params, _seeds(1))
    import torch
    buf = torch.zeros((24, 40, 4), dtype=torch.float32, device="cuda")
    dev.bind_accum(buf.data_ptr(), 40 * 16, 24)
    assert not dev.read_cascades().any()
    dev.render_cascades(params, _seeds(1))
    assert (dev.read_cascades()[..., 3].sum(0) == 1).all() and (dev.read_accum()[..., 3] == 1).all()
    dev.bind_accum(0, 0, 0)
    dev.render_cascades(params, _seeds(1))
    dev.resize(24, 40)  # releases C: the next use allocates planes of the new shape
    with pytest.raises(device.GlrtxError) as e:
        dev.reweight()
    assert e.value.code == -1 and "cascade" in str(e.value)
    assert dev.read_cascades().shape == (6, 40, 24, 4) and not dev.read_cascades().any()
    dev.reweight()  # planes of zeros: every pixel is dead
    D = dev.read_denoised()
    assert not D[..., :3].any() and (D[..., 3] == 1).all()


# ---- 5. refusals
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
        assert "track" in refused(d.render_cascades, params, _seeds(1))  # tracking off
        assert "track" in refused(d.reweight)
        assert "track" in refused(d.read_cascades)
        assert not d.read_accum().any()
        for start in (0.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 21, -1.0):
            assert "start" in refused(d.track_cascades, True, start)
        assert "track" in refused(d.reweight)  # (a refused start switched nothing on)
        d.track_cascades(True)
        assert "cascade" in refused(d.reweight)  # no C yet
        d.render_cascades(params, _seeds(1))
        for kappa in (0.0, -1.0, float("nan"), float("inf")):
            assert "kappa" in refused(d.reweight, kappa=kappa)
        refused(d.read_denoised)  # nothing wrote D
        d.set_partition(0, 2, 16)
        d.render_cascades(params, _seeds(1))
        assert "partitioned" in refused(d.reweight)
        d.set_partition(0, 1, 16)
        d.present_enable(2)
        assert "presentation" in refused(d.render_cascades, params, _seeds(1))
        d.present_enable(0)
        d.set_variant(1)
        assert "variant" in refused(d.render_cascades, params, _seeds(1))
        d.set_variant(2)
        p = device.make_params(dict(params, seed=(0.0, 0.0)))
        assert "seeds" in refused(lambda: d._ck(d.L.glrtx_render_cascades(d.h, device.C.byref(p), None, 2)))  # frames without seeds
        assert "params" in refused(lambda: d._ck(d.L.glrtx_render_cascades(d.h, None, None, 0)))
        d.upload_spheres(np.array([[0, 0, 0, 0.5, 0]], np.float32))
        assert "sphere" in refused(d.render_cascades, params, _seeds(1))
    finally:
        d.close()


# ---- 6. with tracking off nothing changes; with both trackings on each render call feeds its own plane
def test_with_tracking_off_the_other_calls_are_what_they_were(dev, gpu_device):
    import reproject_math as rm
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    cur = rm.move_camera(params, "orbit", 3.0)
    seeds = _seeds(4)
    for d in (dev, gpu_device):
        _setup(d, scene, params, track=False)
        d.track_moments(True)
    dev.track_cascades(True)
    dev.render_cascades(params, seeds[:2]); dev.render_moments(params, seeds[2:])
    gpu_device.render_frames(params, seeds[:2]); gpu_device.render_moments(params, seeds[2:])
    assert (dev.read_cascades()[..., 3].sum(0) == 2).all() and (dev.read_moments()[..., 3] == 2).all()
    dev.track_cascades(False)
    for d in (dev, gpu_device):
        d.render_features(params)
    _same(dev.read_accum(), gpu_device.read_accum(), "accumulator")
    _same(dev.read_moments(), gpu_device.read_moments(), "M")
    for d in (dev, gpu_device):
        d.denoise()
    _same(dev.read_denoised(), gpu_device.read_denoised(), "denoise")
    for d in (dev, gpu_device):
        d.denoise_variance()
    _same(dev.read_denoised(), gpu_device.read_denoised(), "denoise_variance")
    for d in (dev, gpu_device):
        d.reproject(cur)
    _same(dev.read_accum(), gpu_device.read_accum(), "reproject: accumulator")
    _same(dev.read_moments(), gpu_device.read_moments(), "reproject: M")
    assert dev.reproject_last() == gpu_device.reproject_last()
    for d in (dev, gpu_device):
        d.render_moments(cur, _seeds(1, 9))
        d.track_moments(False)
    _same(dev.read_accum(), gpu_device.read_accum(), "render_moments after the move")
