"""Does variance guidance beat its input at every sample count?  On the CPU, with tests/test_denoise_quality.py's harness: the headline scene at 192x108,
max_depth 8; ground truth 512 frames; noisy inputs of 1, 4, 16 and 64 frames with that test's seeds; its metric.  Moments: glrt_fold_moments over the oracle's
per-frame images.  The condition: with the default configuration the variance-guided image's error is strictly below the raw image's at all four sample counts.
The fixed-sigma filter's error (glrtx_denoise's defaults) is printed beside it, not asserted.

Measured with the defaults (5 iterations, sigma_lum 4, sigma_normal 0.1, sigma_depth 0.01, demodulated): raw / fixed sigma / variance-guided
 1 spp 1.0301 / 0.7705 / 0.2582;  4 spp 0.4640 / 0.3058 / 0.1343;  16 spp 0.4102 / 0.2730 / 0.1187;  64 spp 0.1678 / 0.2317 / 0.0819.
DESIGN.md "Variance guidance" holds the sweep the default sigma_lum was picked from."""
import numpy as np
import pytest

from glrt_amd import host
from test_denoise_quality import _error, setup  # noqa: F401  (the fixture and the metric of the fixed-sigma filter's test)


@pytest.mark.parametrize("spp", [1, 4, 16, 64])
def test_default_configuration_beats_the_raw_image(setup, spp):
    from oracle import pt_oracle
    scene, params, ref, n, a = setup
    acc, frames = None, []
    for f in range(spp):
        p = dict(params, seed=host.frame_seed(1000 + 17 * spp + f))
        frames.append(pt_oracle.render(scene, p)[0])
        acc, _ = pt_oracle.render(scene, p, accum=acc)
    M = host.fold_moments(np.zeros_like(acc), np.stack(frames))
    assert (M[..., 3] == spp).all()
    raw = _error(acc[..., :3] / acc[..., 3:4], ref)
    fixed = _error(host.denoise_atrous(acc, n, a)[..., :3], ref)
    var = _error(host.denoise_variance(acc, M, n, a)[..., :3], ref)
    print(f"{spp} spp: raw {raw:.4f}, fixed sigma {fixed:.4f}, variance-guided {var:.4f}, ratio to raw {var / raw:.3f}")
    assert var < raw, (spp, raw, var)


def test_after_a_reprojection_variance_guidance_beats_the_raw_image():
    """The README's scenario, tests/test_reproject_quality.py's: 16 frames at camera A carried over a 3 degree orbit step to camera B, plus ONE frame at B; truth
    512 frames at B.  M rides along: glrt_fold_moments over the 16 frames at A, glrt_reproject_moments, then the one frame at B folded in -- so pixels with
    M.w = 17 (the temporal estimate) and disoccluded pixels with M.w = 1 (the spatial one) share the image.  Reported: the raw, the fixed-sigma and the
    variance-guided error; asserted: variance-guided below raw."""
    import reproject_math as rm
    from oracle import pt_oracle
    from glrt_amd import scenes
    scene, pa = scenes.config_headline(192, 108)
    pa = dict(pa, max_depth=8)
    pb = rm.move_camera(pa, "orbit", 3.0)
    ref = None
    for f in range(512):
        ref, _ = pt_oracle.render(scene, dict(pb, seed=host.frame_seed(f)), accum=ref)
    ref = ref[..., :3] / ref[..., 3:4]
    acc_a, frames = None, []
    for f in range(16):
        p = dict(pa, seed=host.frame_seed(f))
        frames.append(pt_oracle.render(scene, p)[0])
        acc_a, _ = pt_oracle.render(scene, p, accum=acc_a)
    M_a = host.fold_moments(np.zeros_like(acc_a), np.stack(frames))
    n0, a0 = host.render_features(scene, pa, 192, 108)
    n1, a1 = host.render_features(scene, pb, 192, 108)
    carried_acc, carried_M, carried, hits = host.reproject_moments(acc_a, M_a, n0, a0, n1, a1, pa, pb)
    seed_b = host.frame_seed(2000)
    one, _ = pt_oracle.render(scene, dict(pb, seed=seed_b))
    both, _ = pt_oracle.render(scene, dict(pb, seed=seed_b), accum=carried_acc.copy())
    M = host.fold_moments(carried_M, one[None])
    assert (M[..., 3] == 17).any() and (M[..., 3] == 1).any() and np.array_equal(M[..., 3], both[..., 3])
    raw = _error(both[..., :3] / both[..., 3:4], ref)
    fixed = _error(host.denoise_atrous(both, n1, a1)[..., :3], ref)
    var = _error(host.denoise_variance(both, M, n1, a1)[..., :3], ref)
    print(f"carried {carried} of {hits} hit pixels; raw {raw:.4f}, fixed sigma {fixed:.4f}, variance-guided {var:.4f}, ratio to raw {var / raw:.3f}")
    assert var < raw, (raw, var)
