"""The CPU statements of variance guidance (libglrt_host.so: glrt_fold_moments, glrt_variance_estimate, glrt_denoise_variance) against their numpy statements
(tests/variance_math.py), bit for bit, and two exact properties: moments of identical samples give a zero variance, which stops the filter at every luminance
difference; and with one sample per pixel the estimate is the spatial one, computed from the accumulator alone."""
import numpy as np
import pytest

import denoise_math as dm
import variance_math as vm
from glrt_amd import host

SIZES = [(37, 61), (16, 16), (17, 33), (5, 130), (1, 1), (70, 49)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_hostile_arrays_hold_what_they_promise():
    acc, M, N, A = vm.hostile_arrays(37, 61, 3)
    w = M[..., 3]
    assert (w == 0).any() and (dm.tiny(w) & (w != 0)).any() and np.isnan(w).any() and np.isinf(w).any()
    for v in (1, 3, 4, 5):
        assert (w == v).any(), v
    with np.errstate(all="ignore"):
        mu1, mu2 = M[..., 0] / w, M[..., 1] / w
        assert ((mu2 < mu1 * mu1) & (w >= 4)).any() and ((mu2 < mu1 * mu1) & (w >= 1) & (w < 4)).any()


@pytest.mark.parametrize("rows,width", SIZES)
def test_statements_agree_on_hostile_arrays(rows, width):
    acc, M, N, A = vm.hostile_arrays(rows, width, rows * 1000 + width)
    for demodulate in (0, 1):
        v0 = host.variance_estimate(acc, M, N, A, 0.1, 0.01, demodulate)
        assert np.array_equal(_bits(v0), _bits(vm.variance_estimate(acc, M, N, A, 0.1, 0.01, demodulate))), f"V0 {width}x{rows} demod={demodulate}"
        for iterations in range(1, 7):
            for sl in (0.5, 4.0, 1e3):
                got, gv = host.denoise_variance(acc, M, N, A, iterations, sl, 0.1, 0.01, demodulate, return_v0=True)
                ref = vm.denoise_variance(acc, M, N, A, iterations, sl, 0.1, 0.01, demodulate)
                bad = _bits(got) != _bits(ref)
                assert not bad.any(), (f"{width}x{rows}, {iterations} iterations, demodulate {demodulate}, sigma_lum {sl}: {int(bad.any(-1).sum())} pixels differ; "
                                       f"first {np.argwhere(bad)[0].tolist()}")
                assert np.array_equal(_bits(gv), _bits(v0)) and (got[..., 3] == 1).all()
                dead = dm.tiny(acc[..., 3]) | (A[..., 3].view(np.int32) == dm.NO_PIXEL)
                assert not got[dead][:, :3].any() and not v0[dead].any()


def test_tiny_sigmas():
    acc, M, N, A = vm.hostile_arrays(9, 11, 77)
    for demodulate in (0, 1):
        got, v0 = host.denoise_variance(acc, M, N, A, 6, 1e-38, 1e-30, 1e-30, demodulate, return_v0=True)
        ref, rv = vm.denoise_variance(acc, M, N, A, 6, 1e-38, 1e-30, 1e-30, demodulate, return_v0=True)
        assert np.array_equal(_bits(got), _bits(ref)) and np.array_equal(_bits(v0), _bits(rv))


def test_fold_moments_equals_numpy():
    rng = np.random.default_rng(5)
    planes = rng.lognormal(0.0, 2.0, (5, 7, 9, 4)).astype(np.float32)
    planes[0, 0, 0, 0] = np.nan
    planes[1, 1, 1, 1] = np.inf
    planes[2, 2, 2, 2] = -np.inf
    planes[3, 3, 3, :3] = np.float32(1e-40)
    planes[4, 4, 4, :3] = np.float32(2e-20)   # l * l is a denormal
    planes[1, 5, 5, :3] = np.float32(3e38)
    m0 = np.zeros((7, 9, 4), np.float32)
    m1 = host.fold_moments(m0, planes[:2])
    assert np.array_equal(_bits(m1), _bits(vm.fold_moments(m0, planes[:2])))
    m2 = host.fold_moments(m1, planes[2:])
    assert np.array_equal(_bits(m2), _bits(vm.fold_moments(m0, planes)))  # two calls are one chain
    assert (m2[..., 3] == 5).all() and not m2[..., 2].any() and not m0.any()
    assert np.array_equal(_bits(host.fold_moments(m2, planes[:0])), _bits(m2))


def _smooth_scene(rows, width, seed=None):
    N = np.zeros((rows, width, 4), np.float32)
    N[..., 2], N[..., 3] = 1, 2.5
    A = np.ones((rows, width, 4), np.float32)
    A[..., :3] = (0.5, 1.0, 0.25) if seed is None else np.random.default_rng(seed).uniform(0.2, 1.0, (rows, width, 3))
    A[..., 3] = np.full((rows, width), 3, np.int32).view(np.float32)
    return N, A


@pytest.mark.parametrize("demodulate", [0, 1])
def test_identical_samples_give_zero_variance_and_an_untouched_image(demodulate):
    """M = the moments of n identical samples (mu2 = mu1^2 exactly: luminances k / 64 with k < 2^10, so that l * l and the products with n = 4, 8 are exact) and
    M.w >= 4 everywhere: V0 is 0, so is g_p, and sl_p = 1e-6.  The image's greys are distinct multiples of 1 / 256 (albedo a power of two per channel, so the
    demodulated colours are exact too): any two pixels' luminances differ by about 1 / 256 or more, the colour term is then above 3000, and lp_exp of minus that
    is 0.  Only the centre tap weighs, and D is the input mean, bit for bit."""
    rows, width = 19, 35
    N, A = _smooth_scene(rows, width)
    y, x = np.mgrid[0:rows, 0:width]
    n = np.where((x + y) % 2 == 0, 4, 8).astype(np.float32)
    k = (y * width + x + 1).astype(np.float32)
    grey = k / np.float32(256)
    acc = np.zeros((rows, width, 4), np.float32)
    acc[..., :3] = (grey * n)[..., None]
    acc[..., 3] = n
    l = k / np.float32(64)
    M = np.zeros_like(acc)
    M[..., 0], M[..., 1], M[..., 3] = l * n, l * l * n, n
    assert np.array_equal((M[..., 1] / n).astype(np.float64), (M[..., 0] / n).astype(np.float64) ** 2)
    assert not host.variance_estimate(acc, M, N, A, 0.1, 0.01, demodulate).any()
    for it in (1, 3, 5):
        D = host.denoise_variance(acc, M, N, A, it, 4.0, 0.1, 0.01, demodulate)
        assert np.array_equal(_bits(D[..., :3]), _bits(np.repeat(grey[..., None], 3, axis=2)))


def test_one_sample_per_pixel_takes_the_spatial_estimate_from_the_accumulator():
    rows, width = 21, 30
    N, A = _smooth_scene(rows, width, 2)
    rng = np.random.default_rng(3)
    acc = np.ones((rows, width, 4), np.float32)
    acc[..., :3] = rng.lognormal(0.0, 1.0, (rows, width, 3))
    M = vm.fold_moments(np.zeros_like(acc), acc[None])
    assert (M[..., 3] == 1).all()
    v0 = host.variance_estimate(acc, M, N, A, 0.1, 0.01, 0)
    none = host.variance_estimate(acc, np.zeros_like(acc), N, A, 0.1, 0.01, 0)  # no moments at all: mu1 = lum(acc.rgb / acc.w), mu2 = mu1^2
    assert np.array_equal(_bits(v0), _bits(none)) and (v0 > 0).all()
    # and that is the weighted spread of the 7x7 neighbourhood's luminances: all weights are lp_exp(-0) = 1 here
    l = vm.lum(acc[..., 0], acc[..., 1], acc[..., 2]).astype(np.float64)
    y, x = 10, 15
    win = l[y - 3:y + 4, x - 3:x + 4]
    assert v0[y, x] == pytest.approx((win ** 2).mean() - win.mean() ** 2, rel=1e-4)


# ---- the two moment reprojections against numpy, on the arrays reproject_math.py and reproject_motion_math.py build, with an M plane added
REPROJECT_CFGS = [dict(max_history=32, depth_tolerance=0.02, normal_tolerance=0.9), dict(max_history=3, depth_tolerance=0.5, normal_tolerance=-1.0),
                  dict(max_history=1000, depth_tolerance=1e3, normal_tolerance=-2.0), dict(max_history=1, depth_tolerance=1e-40, normal_tolerance=1e-40)]


def _same_planes(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} pixels differ; first {np.argwhere(bad)[0].tolist()}"


@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (5, 130), (1, 1)])
def test_reproject_moments_equals_numpy_and_leaves_the_accumulator_alone(rows, width):
    import reproject_math as rm
    from glrt_amd import scenes
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, n1, a1 = rm.hostile_arrays(rows, width, rows * 1000 + width)
    M = vm.hostile_moments(acc, rows + width)
    W, S, o = host.mat4_inverse(params["c2w"]), host.mat4_inverse(params["s2c"]), rm.origin(params["c2w"])
    some = 0
    for cur in (params, rm.move_camera(params, "pan", 1.0), rm.move_camera(params, "orbit", 2.0)):
        for cfg in REPROJECT_CFGS:
            out, mo, carried, hits = host.reproject_moments(acc, M, n0, a0, n1, a1, params, cur, **cfg)
            ref, rmo, c2, h2 = vm.reproject_moments(acc, M, n0, a0, n1, a1, W, S, o, cur, **cfg)
            _same_planes(mo, rmo, f"M {width}x{rows} {cfg}")
            _same_planes(out, ref, f"accumulator {width}x{rows} {cfg}")
            plain, c3, h3 = host.reproject(acc, n0, a0, n1, a1, params, cur, **cfg)
            _same_planes(out, plain, f"accumulator against host.reproject {width}x{rows} {cfg}")
            assert (carried, hits) == (c2, h2) == (c3, h3)
            assert not mo[out[..., 3] == 0].any() and not mo[..., 2].any() and (mo[..., 3] <= cfg["max_history"]).all()
            some += int((mo[..., 3] > 0).sum())
    assert some > 0 or rows * width == 1


@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (1, 1)])
def test_reproject_motion_moments_equals_numpy_and_leaves_the_accumulator_alone(rows, width):
    import reproject_math as rm
    import reproject_motion_math as rmm
    from glrt_amd import scenes
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, g1, a1, vert, tri = rmm.hostile_arrays(rows, width, rows * 1000 + width)
    M = vm.hostile_moments(acc, rows + width)
    some = 0
    for prev in (params, rm.move_camera(params, "pan", 1.0), rm.move_camera(params, "orbit", 2.0)):
        W, S, o = host.mat4_inverse(prev["c2w"]), host.mat4_inverse(prev["s2c"]), rm.origin(prev["c2w"])
        for cfg in REPROJECT_CFGS:
            out, mo, carried, hits = host.reproject_motion_moments(acc, M, n0, a0, g1, a1, vert, tri, prev, **cfg)
            ref, rmo, c2, h2 = vm.reproject_motion_moments(acc, M, n0, a0, g1, a1, vert, tri, W, S, o, **cfg)
            _same_planes(mo, rmo, f"M {width}x{rows} {cfg}")
            _same_planes(out, ref, f"accumulator {width}x{rows} {cfg}")
            plain, c3, h3 = host.reproject_motion(acc, n0, a0, g1, a1, vert, tri, prev, **cfg)
            _same_planes(out, plain, f"accumulator against host.reproject_motion {width}x{rows} {cfg}")
            assert (carried, hits) == (c2, h2) == (c3, h3)
            some += int((mo[..., 3] > 0).sum())
    assert some > 0 or rows * width == 1


def test_an_unmoved_camera_keeps_the_moments_means():
    """Identity reprojection of a smooth image: every pixel takes its own tap with weight ~1, so nm = M.w and the carried means are the old ones to rounding."""
    import reproject_math as rm
    from glrt_amd import scenes
    scene, params = scenes.config_c1(48, 32, max_depth=4, subdiv=1)
    n0, a0 = host.render_features(scene, params, 48, 32)
    rng = np.random.default_rng(4)
    acc = np.ones((32, 48, 4), np.float32) * 6
    acc[..., :3] = rng.uniform(1, 2, (32, 48, 3)) * 6
    M = np.zeros_like(acc)
    M[..., 3] = 6
    M[..., 0] = rng.uniform(1, 2, (32, 48)) * 6
    M[..., 1] = M[..., 0] ** 2 / 6 * 1.25
    out, mo, carried, hits = host.reproject_moments(acc, M, n0, a0, n0, a0, params, params)
    kept = out[..., 3] == 6
    assert carried > 0.9 * hits and kept.sum() > 0.9 * hits
    assert (mo[kept][:, 3] == 6).all() and np.allclose(mo[kept][:, :2], M[kept][:, :2], rtol=1e-3)


def test_denoise_variance_without_v0_equals_with():
    acc, M, N, A = vm.hostile_arrays(9, 11, 5)
    D, _ = host.denoise_variance(acc, M, N, A, return_v0=True)
    assert np.array_equal(_bits(host.denoise_variance(acc, M, N, A)), _bits(D))  # (out_v0 = NULL)
