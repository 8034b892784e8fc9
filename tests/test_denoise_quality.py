"""Does the denoiser beat its input where it is meant to be used?  On the CPU (the oracle's renders, the filter's CPU statement -- which the device equals bit
for bit, tests/test_gpu_denoise.py): the headline scene at 192x108, max_depth 8; ground truth 512 frames; noisy inputs of 1 and 4 frames with other seeds;
metric sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) over rgb.  The condition: with the default configuration the denoised image's error is strictly below the raw
image's at both sample counts.

Measured with the defaults (5 iterations, sigma_color 100, sigma_normal 0.1, sigma_depth 0.01, demodulated): 1 spp 1.030 raw -> 0.771 (ratio 0.75),
4 spp 0.464 raw -> 0.306 (ratio 0.66).  DESIGN.md "Denoising" holds the sweep these defaults were picked from."""
import numpy as np
import pytest

from glrt_amd import host, scenes

W, H = 192, 108


@pytest.fixture(scope="module")
def setup():
    from oracle import pt_oracle
    scene, params = scenes.config_headline(W, H)
    params = dict(params, max_depth=8)
    ref = None
    for f in range(512):
        ref, _ = pt_oracle.render(scene, dict(params, seed=host.frame_seed(f)), accum=ref)
    assert (ref[..., 3] == 512).all()
    n, a = host.render_features(scene, params, W, H)
    return scene, params, ref[..., :3] / ref[..., 3:4], n, a


def _error(x, ref):
    return float(np.sqrt(np.mean((x.astype(np.float64) - ref) ** 2 / (ref.astype(np.float64) ** 2 + 1e-2))))


@pytest.mark.parametrize("spp", [1, 4])
def test_default_configuration_beats_the_raw_image(setup, spp):
    from oracle import pt_oracle
    scene, params, ref, n, a = setup
    acc = None
    for f in range(spp):
        acc, _ = pt_oracle.render(scene, dict(params, seed=host.frame_seed(1000 + 17 * spp + f)), accum=acc)
    raw = _error(acc[..., :3] / acc[..., 3:4], ref)
    den = _error(host.denoise_atrous(acc, n, a)[..., :3], ref)
    print(f"{spp} spp: raw {raw:.4f}, denoised {den:.4f}, ratio {den / raw:.3f}")
    assert den < raw, (spp, raw, den)
