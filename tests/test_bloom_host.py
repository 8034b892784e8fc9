"""Bloom without a GPU (include/glrtx.h "Bloom"): the CPU statement (glrt_bloom, host/bloom.cpp) and the numpy statement (tests/bloom_math.py) agree on every
word of the down chain's planes D_1 .. D_levels and of B, on hostile arrays of every size the contract was prototyped on; and the three properties the header
derives from the arithmetic hold in both."""
import numpy as np
import pytest

import bloom_math as bm
from glrt_amd import host


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def arrays():
    return {s: bm.hostile(s[0], s[1], 19 + i) for i, s in enumerate(bm.SIZES)}


def test_the_hostile_array_holds_what_the_contract_rules_on(arrays):
    a = arrays[(13, 67)]
    w = a[..., 3]
    assert (w == 0).any() and np.isnan(w).any() and np.isinf(w).any() and (w < 0).any() and ((np.abs(w) < 1e-38) & (w != 0)).any()
    assert np.isnan(a[..., :3]).any() and np.isinf(a[..., :3]).any() and (a[..., :3] < 0).any() and (a[..., :3] == np.float32(3e38)).any()
    l = bm.lum(bm.pixel_value(a))
    for centre in (1.0, 1e-4):  # luminances on both sides of the threshold and of the floor of the quotient's divisor, within a few ulps
        near = np.abs(l.astype(np.float64) - centre) <= 8 * np.spacing(np.float32(centre))
        assert (near & (l > np.float32(centre))).any() and (near & (l <= np.float32(centre))).any(), centre


@pytest.mark.parametrize("levels", bm.LEVELS)
@pytest.mark.parametrize("shape", bm.SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_statements_agree_on_hostile_arrays(arrays, shape, levels):
    a = arrays[shape]
    for threshold, strength in ((1.0, 0.25), (0.0, 4.0), (1e-4, 1e4)):
        d, B = host.bloom(a, threshold, strength, levels)
        dn, Bn = bm.bloom(a, threshold, strength, levels)
        assert d.shape == dn.shape == (host.bloom_texels(shape[1], shape[0], levels), 4)
        assert np.array_equal(bits(d), bits(dn)), f"D differs on {int((bits(d) != bits(dn)).any(-1).sum())} texels"
        assert np.array_equal(bits(B), bits(Bn)), f"B differs on {int((bits(B) != bits(Bn)).any(-1).sum())} pixels"
        assert (d[:, 3] == 0).all() and (B[..., 3] == 1).all()


def test_level_sizes():
    assert bm.level_sizes(67, 13, 5) == [(67, 13), (34, 7), (17, 4), (9, 2), (5, 1), (3, 1)]
    assert bm.level_sizes(1, 1, 8)[-1] == (1, 1)
    assert host.bloom_texels(67, 13, 5) == 34 * 7 + 17 * 4 + 9 * 2 + 5 + 3


@pytest.mark.parametrize("levels", [1, 2, 4, 8])
@pytest.mark.parametrize("shape", bm.SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_property_1_a_uniform_image_comes_back_as_one(shape, levels):
    """{0.5, 0.5, 0.5, 1}, threshold 0, strength 1: g = 1, every level holds 0.5, U_1 = levels / 2, glow = 0.5, B = 1.0f at every pixel -- the edge clamps, the
    level sizes and the normalisation."""
    a = np.empty(shape + (4,), np.float32)
    a[...] = (0.5, 0.5, 0.5, 1.0)
    for fn in (host.bloom, bm.bloom):
        d, B = fn(a, 0.0, 1.0, levels)
        assert (bits(d[:, :3]) == bits(np.float32(0.5))).all()
        assert (bits(B) == bits(np.float32(1.0))).all()


@pytest.mark.parametrize("shape", bm.SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_property_2_nothing_over_the_threshold_or_no_strength_gives_x(arrays, shape):
    a = arrays[shape]
    x = bm.pixel_value(a)
    for fn in (host.bloom, bm.bloom):
        _, B = fn(a, 1.0, 0.0, 5)  # strength 0
        assert np.array_equal(bits(B[..., :3]), bits(x))
        d, B = fn(a, 1.0e5, 4.0, 5)  # x <= 65504 per channel: no luminance comes near 1e5
        assert not d.any() and np.array_equal(bits(B[..., :3]), bits(x))


@pytest.mark.parametrize("shape", bm.SIZES, ids=lambda s: f"{s[1]}x{s[0]}")
def test_property_3_b_is_finite(arrays, shape):
    a = arrays[shape].copy()
    a[0, 0] = (3e38, np.nan, np.inf, 1.0)
    for fn in (host.bloom, bm.bloom):
        d, B = fn(a, 0.0, 4.0, 8)
        assert np.isfinite(d).all() and np.isfinite(B).all() and (B[..., :3] >= 0).all() and (d >= 0).all()


def test_the_glow_does_what_it_is_for():
    a = np.zeros((33, 33, 4), np.float32)
    a[...] = (0.2, 0.2, 0.2, 1.0)
    a[16, 16] = (400.0, 200.0, 100.0, 2.0)  # one emitter: mean (200, 100, 50)
    _, B = host.bloom(a, 1.0, 0.25, 5)
    glow = B[..., :3] - bm.pixel_value(a)
    assert (glow >= 0).all() and glow[16, 17, 0] > glow[16, 24, 0] > glow[16, 32, 0] > 0  # falls off with distance, reaches the edge at five levels
    assert glow[16, 17, 0] > glow[16, 17, 1] > glow[16, 17, 2]  # and keeps the emitter's colour
    _, B1 = host.bloom(a, 1.0, 0.25, 1)
    assert (B1[16, 28:, :3] == np.float32(0.2)).all()  # one level reaches a few pixels


BAD = [dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(strength=-0.5), dict(strength=1.0001e4), dict(strength=float("nan")),
       dict(levels=0), dict(levels=9)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_bad_arguments_are_refused(bad):
    with pytest.raises(RuntimeError):
        host.bloom(np.ones((2, 2, 4), np.float32), **bad)
