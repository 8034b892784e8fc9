"""The denoiser's CPU statements (libglrt_host.so: glrt_render_features, glrt_denoise_atrous) against their numpy statements (tests/denoise_math.py),
bit for bit, and the filter's two exact properties: a constant image stays what it is, and materials do not bleed into each other."""
import numpy as np
import pytest

import denoise_math as dm
from fuzz_scenes import CASES, case_scene_and_params
from glrt_amd import host, scenes


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _features_numpy(scene, params, w, h, rows_y=None):
    rays = dm.centre_rays(params, w, h, rows_y)
    hits = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], rays)
    return dm.features_from_hits(scene, hits, rays.shape[0] // w, w)


def _check_features(scene, params, w, h, what):
    n, a = host.render_features(scene, params, w, h)
    n2, a2 = _features_numpy(scene, params, w, h)
    assert np.array_equal(_bits(n), _bits(n2)), f"{what}: normal / depth plane differs on {int((_bits(n) != _bits(n2)).any(-1).sum())} pixels"
    assert np.array_equal(_bits(a), _bits(a2)), f"{what}: albedo / id plane differs on {int((_bits(a) != _bits(a2)).any(-1).sum())} pixels"
    return n, a


def test_features_c1():
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    n, a = _check_features(scene, params, 96, 64, "c1")
    ids = a[..., 3].view(np.int32)
    assert (ids >= 0).any() and (ids == -1).any()  # hits and misses are both in the picture
    hit = ids >= 0
    assert np.allclose(np.linalg.norm(n[hit][:, :3], axis=1), 1.0, atol=1e-5) and (n[hit][:, 3] > 1e-4).all()
    assert not n[~hit].any() and (a[~hit][:, :3] == 1).all()


@pytest.mark.parametrize("case", [0, 1, 4, 7], ids=lambda c: f"fuzz{CASES[c][0]}-{CASES[c][2]}")
def test_features_fuzz_scenes(case):
    scene, params = case_scene_and_params(CASES[case])
    _check_features(scene, params, params["width"], params["height"], f"case {CASES[case][0]}")


def test_features_vine():
    scene, params = scenes.config_c3(48, 32, n=500)
    _check_features(scene, params, 48, 32, "c3 vine")


def test_features_partition_rows():
    scene, params = scenes.config_c1(40, 52, max_depth=4, subdiv=1)
    full_n, full_a = host.render_features(scene, params, 40, 52)
    for rank in range(3):
        rows_y = [y for y in range(52) if (y // 8) % 3 == rank]
        n, a = host.render_features(scene, params, 40, 52, rank=rank, world=3, stripe=8)
        assert np.array_equal(_bits(n), _bits(full_n[rows_y])) and np.array_equal(_bits(a), _bits(full_a[rows_y]))


@pytest.mark.parametrize("demodulate", [0, 1])
@pytest.mark.parametrize("iterations", [1, 2, 3, 4, 5, 6])
def test_atrous_equals_numpy_on_hostile_arrays(iterations, demodulate):
    for (rows, width), seed in (((37, 61), 3), ((16, 16), 4), ((5, 130), 5)):
        acc, N, A = dm.hostile_arrays(rows, width, seed + 10 * iterations)
        for sigma_color in (1.0, 1e3):
            got = host.denoise_atrous(acc, N, A, iterations, sigma_color, 0.1, 0.01, demodulate)
            ref = dm.atrous(acc, N, A, iterations, sigma_color, 0.1, 0.01, demodulate)
            bad = _bits(got) != _bits(ref)
            assert not bad.any(), (f"{width}x{rows}, {iterations} iterations, demodulate {demodulate}, sigma_color {sigma_color}: {int(bad.any(-1).sum())} pixels differ; "
                                   f"first {np.argwhere(bad)[0].tolist()}")
            assert (got[..., 3] == 1).all()
            dead = dm.tiny(acc[..., 3]) | (A[..., 3].view(np.int32) == dm.NO_PIXEL)
            assert not got[dead][:, :3].any()


def test_tiny_sigma_and_one_pixel():
    acc, N, A = dm.hostile_arrays(9, 11, 77)
    for sc in (1e-38, 1e-30):  # sigma_color * 4^-i reaches the denormals: read as zero on both sides
        assert np.array_equal(_bits(host.denoise_atrous(acc, N, A, 6, sc, 1e-30, 1e-30, 1)), _bits(dm.atrous(acc, N, A, 6, sc, 1e-30, 1e-30, 1)))
    one = host.denoise_atrous(acc[:1, :1], N[:1, :1], A[:1, :1], 3, 1.0, 0.1, 0.01, 0)
    assert np.array_equal(_bits(one), _bits(dm.atrous(acc[:1, :1], N[:1, :1], A[:1, :1], 3, 1.0, 0.1, 0.01, 0)))


@pytest.mark.parametrize("demodulate", [0, 1])
def test_constant_image_is_unchanged(demodulate):
    """With constant colour and features every weight is k[dy] k[dx] * lp_exp(-0) = k[dy] k[dx] exactly, the weights' sum is a multiple of 1 / 256, and for
    colours with few significand bits (their products with 1, 4, 6, 16, 24, 36 and the partial sums must stay exact) the quotient gives the colour back
    exactly -- at the borders, where taps are missing, too."""
    rows, width = 23, 45
    colour = np.array([1.5, 0.25, 6.0], np.float32)
    acc = np.zeros((rows, width, 4), np.float32)
    acc[..., :3] = colour * 4
    acc[..., 3] = 4
    N = np.zeros((rows, width, 4), np.float32)
    N[..., 2], N[..., 3] = 1, 2.5
    A = np.ones((rows, width, 4), np.float32)
    A[..., :3] = (0.5, 1.0, 0.25)
    A[..., 3] = np.full((rows, width), 3, np.int32).view(np.float32)
    for it in range(1, 7):
        out = host.denoise_atrous(acc, N, A, it, 1.0, 0.1, 0.01, demodulate)
        assert np.array_equal(out[..., :3], np.broadcast_to(colour, (rows, width, 3))) and (out[..., 3] == 1).all()


def test_checkerboard_materials_do_not_mix():
    """Two materials in a checkerboard of 3x3 blocks, one red and one blue, identical normals and depths, a colour sigma that stops nothing: every pixel keeps
    exactly zero in the other material's channel, and a non-zero value in its own."""
    rows, width = 40, 52
    y, x = np.mgrid[0:rows, 0:width]
    m = ((y // 3 + x // 3) % 2).astype(np.int32)
    rng = np.random.default_rng(9)
    acc = np.zeros((rows, width, 4), np.float32)
    acc[..., 0] = np.where(m == 0, rng.uniform(0.5, 4.0, (rows, width)), 0)
    acc[..., 2] = np.where(m == 1, rng.uniform(0.5, 4.0, (rows, width)), 0)
    acc[..., 3] = 1
    N = np.zeros((rows, width, 4), np.float32)
    N[..., 2], N[..., 3] = 1, 4.0
    A = np.ones((rows, width, 4), np.float32)
    A[..., 3] = m.view(np.float32)
    for demodulate in (0, 1):
        out = host.denoise_atrous(acc, N, A, 5, 1e6, 0.1, 0.01, demodulate)
        assert (out[m == 0][:, 2] == 0).all() and (out[m == 1][:, 0] == 0).all() and (out[..., 1] == 0).all()
        assert (out[m == 0][:, 0] > 0).all() and (out[m == 1][:, 2] > 0).all()
        assert out[m == 0][:, 0].std() < acc[m == 0][:, 0].std()  # and it did filter
