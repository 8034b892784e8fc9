"""glrt_adaptive_select_moments (host/variance.cpp) against the numpy statement (tests/adaptive_moments_math.py), bit for bit, and the statement's own
properties; the numpy accumulate against glrt_fold_moments.  No GPU."""
import numpy as np
import pytest

from conftest import assert_bit_equal

import adaptive_math as am
import adaptive_moments_cases as cases
import adaptive_moments_math as amm

f32 = np.float32
PLANES = cases.planes()


@pytest.mark.parametrize("M", [p[1] for p in PLANES], ids=[p[0] for p in PLANES])
def test_host_statement_equals_numpy(M):
    from glrt_amd import host
    e_np = amm.tile_error(M)
    for thr in cases.thresholds(e_np):
        for min_samples in (2, cases.MIN_SAMPLES):
            mask, e, lst = amm.select(M, thr, min_samples)
            h_mask, h_e = host.adaptive_select_moments(M, thr, min_samples)
            assert np.array_equal(h_mask, mask), (thr, min_samples)
            assert np.array_equal(h_e.view(np.uint32), e.view(np.uint32)), (thr, min_samples)
            assert np.array_equal(lst, np.flatnonzero(mask.reshape(-1)))


def test_the_cases_hold_what_the_contract_names():
    """The planes really exercise the branches: forced and unforced pixels, a negative variance clipped by the select, NaN and Inf errors, a mid threshold
    that splits the tiles."""
    px = dict(cases.hostile_pixels())
    with np.errstate(all="ignore"):
        d = {k: amm.pixel_error(v[None, None, :])[0, 0] for k, v in px.items()}
    assert d["v_minus_ulp"] == 0 and d["v_zero"] == 0 and d["v_plus_ulp"] > 0
    m = px["v_minus_ulp"]
    assert f32(m[1] / m[3]) - f32(m[0] / m[3]) * f32(m[0] / m[3]) < 0
    assert np.isnan(d["x_nan"]) and np.isnan(d["mu1_below_minus_floor"]) and np.isinf(d["mu1_at_minus_floor"]) and np.isnan(d["mu1_at_minus_floor_v0"])
    assert np.isfinite(d["mu1_above_minus_floor"]) and d["x_denormal"] == 0
    for k in ("w_zero", "w_negzero", "w_denormal", "w_negative", "w_nan", "w_one", "w_min_minus_1"):
        assert amm.select(px[k][None, None, :], np.inf, cases.MIN_SAMPLES)[0].all(), k
    for k in ("w_inf", "w_min", "w_2p24"):
        assert not amm.select(px[k][None, None, :], np.inf, cases.MIN_SAMPLES)[0].any(), k
    M = cases.plausible(241, 135, 3)
    e = amm.tile_error(M)
    mid = cases.thresholds(e)[2]
    mask = amm.select(M, mid, cases.MIN_SAMPLES)[0]
    assert 0 < mask.sum() < mask.size


@pytest.mark.parametrize("M", [p[1] for p in PLANES if "sprinkled" in p[0] or "plausible" in p[0]], ids=[p[0] for p in PLANES if "sprinkled" in p[0] or "plausible" in p[0]])
def test_a_negative_threshold_marks_every_tile(M):
    from glrt_amd import host
    for fn in (lambda: amm.select(M, -1.0, 2)[0], lambda: host.adaptive_select_moments(M, -1.0, 2)[0], lambda: amm.select(M, -1e-30, 2)[0]):
        assert fn().all()


@pytest.mark.parametrize("size", cases.SIZES, ids=[f"{w}x{h}" for w, h in cases.SIZES])
def test_zero_moments_mark_every_tile(size):
    from glrt_amd import host
    M = np.zeros((size[1], size[0], 4), np.float32)
    for thr in (0.0, 1e30, np.inf):
        assert amm.select(M, thr, 2)[0].all() and host.adaptive_select_moments(M, thr, 2)[0].all()


@pytest.mark.parametrize("size", cases.SIZES, ids=[f"{w}x{h}" for w, h in cases.SIZES])
def test_constant_luminance_retires_every_tile_at_threshold_zero(size):
    """A pixel that saw n >= min_samples samples of one luminance l.  With l a multiple of 1/8 below 4 and n <= 64, n l and n l^2 are exact in fp32, so
    mu1 = l and mu2 = l^2 exactly, v = l^2 - l * l = 0 exactly, d = 0 and E = 0 <= 0: every tile retires."""
    from glrt_amd import host
    w, h = size
    rng = np.random.default_rng(w * 1000 + h)
    l = (rng.integers(0, 32, (h, w)) / 8.0).astype(np.float32)
    n = rng.integers(cases.MIN_SAMPLES, 65, (h, w)).astype(np.float32)
    M = np.stack([n * l, n * l * l, np.zeros_like(l), n], -1).astype(np.float32)
    mask, e, lst = amm.select(M, 0.0, cases.MIN_SAMPLES)
    assert not mask.any() and not e.view(np.uint32).any() and lst.size == 0
    h_mask, h_e = host.adaptive_select_moments(M, 0.0, cases.MIN_SAMPLES)
    assert not h_mask.any() and not h_e.view(np.uint32).any()
    M[h // 2, w // 2, 3] = cases.MIN_SAMPLES - 1  # one pixel short of min_samples: its tile, and only its tile, is active
    mask = amm.select(M, 0.0, cases.MIN_SAMPLES)[0]
    assert mask.sum() == 1 and mask[(h // 2) // 8, (w // 2) // 8] == 1
    assert np.array_equal(host.adaptive_select_moments(M, 0.0, cases.MIN_SAMPLES)[0], mask)


@pytest.mark.parametrize("size", [(3, 5), (50, 38)], ids=["3x5", "50x38"])
def test_accumulate_is_fold_moments_on_active_pixels_and_the_identity_elsewhere(size):
    from glrt_amd import host
    w, h = size
    rng = np.random.default_rng(7 + w)
    M0 = cases.plausible(w, h, 5)
    acc0 = np.concatenate([rng.uniform(0, 50, (h, w, 3)), M0[..., 3:4]], -1).astype(np.float32)
    samples = np.concatenate([rng.uniform(0, 100, (5, h, w, 3)), np.ones((5, h, w, 1))], -1).astype(np.float32)
    samples[2, 0, 0, :3] = 1e-39  # (a denormal sample counts as zero)
    ty, tx = am.tiles_of(h, w)
    mask = (rng.uniform(size=(ty, tx)) < 0.5).astype(np.uint8)
    mask.reshape(-1)[0] = 1
    if mask.size > 1:
        mask.reshape(-1)[-1] = 0
    on = am.expand_mask(mask, h, w)
    acc1, M1 = amm.accumulate(acc0, M0, samples, mask)
    folded = host.fold_moments(M0, samples)
    assert_bit_equal(M1[on], folded[on], "M on active pixels")
    assert_bit_equal(M1[~on], M0[~on], "M on inactive pixels")
    assert_bit_equal(acc1, am.accumulate(acc0, np.zeros_like(acc0), samples, mask)[0], "accumulator")
    assert_bit_equal(acc1[~on], acc0[~on], "accumulator on inactive pixels")
    assert (acc1[on][:, 3] == acc0[on][:, 3] + 5).all() and (M1[on][:, 3] == M0[on][:, 3] + 5).all()
    all_on = np.ones_like(mask)
    assert_bit_equal(amm.accumulate(acc0, M0, samples, all_on)[1], folded, "every tile active: fold_moments")
