"""Does firefly re-weighting beat its input where it is meant to be used, without simply dropping what is bright?  On the CPU, with
tests/test_denoise_quality.py's harness: the headline scene at 192x108, max_depth 8; ground truth 512 frames; noisy inputs of 4, 16 and 64 frames with that
test's seeds; its metric.  Cascades: glrt_fold_cascades over the oracle's per-frame images; resolve: glrt_reweight; the default configuration (start 1, kappa 4).
Three conditions per sample count: the re-weighted error is strictly below the raw error; R <= mean * (1 + 1e-5) + 1e-7 at every pixel (the resolve only ever
takes away); sum lum(R) >= 0.98 * sum lum(mean) (it takes away next to nothing: a resolve that drops everything bright fails here).

Measured with the defaults: raw / re-weighted / sum lum(R) / sum lum(mean)
  4 spp 0.4640 / 0.4039 / 0.991;  16 spp 0.4102 / 0.2075 / 0.991;  64 spp 0.1678 / 0.1141 / 0.993.
DESIGN.md "Firefly re-weighting" holds the table with 1 and 256 spp and the sweep over kappa and start."""
import numpy as np
import pytest

from glrt_amd import host
from test_denoise_quality import _error, setup  # noqa: F401  (the fixture and the metric of the fixed-sigma filter's test)


def _lum(x):
    return 0.2126 * x[..., 0].astype(np.float64) + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]


@pytest.mark.parametrize("spp", [4, 16, 64])
def test_default_configuration_beats_the_raw_image_and_keeps_the_energy(setup, spp):
    from oracle import pt_oracle
    scene, params, ref, n, a = setup
    frames = [pt_oracle.render(scene, dict(params, seed=host.frame_seed(1000 + 17 * spp + f)))[0] for f in range(spp)]
    C, acc = host.fold_cascades(None, np.stack(frames), accum=np.zeros_like(frames[0]), **{"start": host.REWEIGHT_DEFAULTS["start"]})
    assert (acc[..., 3] == spp).all() and (C[..., 3].sum(0) == spp).all()
    mean = acc[..., :3] / acc[..., 3:4]
    R = host.reweight(C, host.REWEIGHT_DEFAULTS["kappa"])[..., :3]
    raw, rew = _error(mean, ref), _error(R, ref)
    energy = _lum(R).sum() / _lum(mean).sum()
    print(f"{spp} spp: raw {raw:.4f}, re-weighted {rew:.4f}, ratio {rew / raw:.3f}, sum lum(R) / sum lum(mean) {energy:.4f}, "
          f"max (R - mean) {float((R.astype(np.float64) - mean).max()):.3g}")
    assert rew < raw, (spp, raw, rew)
    assert (R <= mean.astype(np.float64) * (1 + 1e-5) + 1e-7).all()
    assert energy >= 0.98, (spp, energy)
