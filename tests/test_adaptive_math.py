"""Properties of the numpy statement of the adaptive selection (tests/adaptive_math.py) -- the statement the device is pinned against
in tests/test_gpu_adaptive.py."""
import numpy as np

import adaptive_math as am


def _const(rows, width, rgb, count, half_count):
    acc = np.zeros((rows, width, 4), np.float32)
    half = np.zeros_like(acc)
    acc[..., :3] = np.float32(rgb) * np.float32(count)
    acc[..., 3] = count
    half[..., :3] = np.float32(rgb) * np.float32(half_count)
    half[..., 3] = half_count
    return acc, half


def test_constant_image_retires_once_min_samples_is_reached():
    for count in (1, 2, 3, 4, 8):
        acc, half = _const(24, 32, 0.5, count, count // 2)
        mask, e, lst = am.select(acc, half, 1e-6, 4)
        assert np.all(e[np.isfinite(e)] == 0)
        assert mask.all() == (count < 4), count
        assert (not mask.any()) == (count >= 4), count


def test_one_pixel_under_min_samples_or_nan_keeps_its_tile_active():
    acc, half = _const(16, 16, 0.25, 8, 4)
    acc[3, 5, :] = [0.25 * 3, 0.25 * 3, 0.25 * 3, 3]  # tile 0 has a pixel with 3 < 4 samples (and no error)
    acc[12, 9, 0] = np.nan                             # tile 3 has a NaN
    mask, e, lst = am.select(acc, half, 1e-3, 4)
    assert mask.tolist() == [[1, 0], [0, 1]]
    assert e[0, 0] == 0 and np.isnan(e[1, 1])
    assert e.view(np.uint32)[1, 1] == 0x7FC00000
    half[0, 0, 3] = 0  # H.w == 0 activates a tile too
    mask, _, _ = am.select(acc, half, 1e-3, 4)
    assert mask.tolist() == [[1, 0], [0, 1]]
    half[8, 0, 3] = 0
    mask, _, _ = am.select(acc, half, 1e-3, 4)
    assert mask.tolist() == [[1, 0], [1, 1]]


def test_partial_edge_tiles_count_only_in_image_pixels():
    rows, width = 11, 13
    acc, half = _const(rows, width, 1.0, 4, 2)
    acc[..., 0] = acc[..., 0] * np.float32(1.5)  # every pixel: I.r = 1.5, A.r = 1: d = 0.5 / sqrt(3.5 + 1e-3)
    d = np.float32(0.5) / np.sqrt(np.float32(np.float32(3.5) + np.float32(1e-3)))
    mask, e, _ = am.select(acc, half, 10.0, 2)
    assert e.shape == (2, 2) and not mask.any()
    # a sum of n equal d over the tree, divided by n, is d up to rounding; the partial tiles are not diluted by the 0 lanes outside
    assert np.allclose(e, d, rtol=1e-6)
    e_full = am.tile_error(np.tile(acc[:8, :8], (2, 2, 1)), np.tile(half[:8, :8], (2, 2, 1)))
    assert np.allclose(e_full, d, rtol=1e-6)
    # a pixel outside the image never activates a tile: the padding is not looked at
    assert am.to_tiles(np.ones((rows, width), bool), False).sum(-1).tolist() == [[64, 40], [24, 15]]


def test_list_is_ascending_and_matches_the_mask():
    rng = np.random.default_rng(7)
    rows, width = 37, 45
    acc = rng.uniform(0, 4, (rows, width, 4)).astype(np.float32)
    acc[..., 3] = rng.integers(2, 9, (rows, width))
    half = (acc * np.float32(0.5) * rng.uniform(0.8, 1.2, acc.shape)).astype(np.float32)
    half[..., 3] = np.floor(acc[..., 3] / 2)
    mask, e, lst = am.select(acc, half, float(np.median(e_all := am.tile_error(acc, half))), 2)
    assert 0 < mask.sum() < mask.size
    assert np.all(np.diff(lst) > 0)
    assert lst.tolist() == np.flatnonzero(mask.reshape(-1)).tolist()
    assert np.array_equal(mask.astype(bool), ~(e_all <= np.median(e_all)))
    # threshold < 0: nothing retires
    assert am.select(acc, half, -1.0, 2)[0].all()


def test_accumulate_keeps_every_second_sample_in_half():
    rows, width = 9, 10
    acc = np.zeros((rows, width, 4), np.float32)
    half = np.zeros_like(acc)
    samples = np.zeros((5, rows, width, 4), np.float32)
    samples[..., :3] = np.arange(1, 6, dtype=np.float32)[:, None, None, None]
    samples[..., 3] = 1
    mask = np.array([[1, 0], [0, 1]], np.uint8)
    a, h = am.accumulate(acc, half, samples, mask)
    on = am.expand_mask(mask, rows, width)
    assert np.all(a[on][:, 3] == 5) and np.all(a[~on] == 0)
    assert np.all(h[on][:, 3] == 2) and np.all(h[on][:, 0] == 2 + 4) and np.all(h[~on] == 0)
    assert np.all(a[on][:, 0] == 15)
