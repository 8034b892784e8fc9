"""Is arriving at a new viewpoint with the old samples worth it?  On the CPU (the oracle's renders, the reprojection's CPU statement -- which the device equals
bit for bit, tests/test_gpu_reproject.py): the headline scene at 192x108, max_depth 8; 16 frames at camera A, reprojected to camera B, 3 degrees further along an
orbit about the world's y axis, plus ONE frame at B -- against that one frame at B alone.  Ground truth: 512 frames at B; metric as in
tests/test_denoise_quality.py, sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) over rgb.  The condition: the error is strictly lower with the carried history, raw
and after the default denoiser; and the pass is not vacuous: at least 80 % of the new view's hit pixels carry history.

Measured with the defaults (max_history 32, depth_tolerance 0.02, normal_tolerance 0.9): carried 0.992 of the hit pixels; raw 0.913 -> 0.270 (ratio 0.30),
denoised 0.589 -> 0.243 (ratio 0.41).  DESIGN.md "Reprojection" holds the sweep these defaults were picked from."""
import numpy as np
import pytest

import reproject_math as rm
from glrt_amd import host, scenes

W, H = 192, 108
ORBIT_DEGREES = 3.0


def _error(x, ref):
    return float(np.sqrt(np.mean((x.astype(np.float64) - ref) ** 2 / (ref.astype(np.float64) ** 2 + 1e-2))))


def test_carried_history_beats_one_frame_alone():
    from oracle import pt_oracle
    scene, pa = scenes.config_headline(W, H)
    pa = dict(pa, max_depth=8)
    pb = rm.move_camera(pa, "orbit", ORBIT_DEGREES)
    ref = None
    for f in range(512):
        ref, _ = pt_oracle.render(scene, dict(pb, seed=host.frame_seed(f)), accum=ref)
    assert (ref[..., 3] == 512).all()
    ref = ref[..., :3] / ref[..., 3:4]
    acc_a = None
    for f in range(16):
        acc_a, _ = pt_oracle.render(scene, dict(pa, seed=host.frame_seed(f)), accum=acc_a)
    n0, a0 = host.render_features(scene, pa, W, H)
    n1, a1 = host.render_features(scene, pb, W, H)
    seed_b = host.frame_seed(2000)
    one, _ = pt_oracle.render(scene, dict(pb, seed=seed_b))
    carried_acc, carried, hits = host.reproject(acc_a, n0, a0, n1, a1, pa, pb)
    both, _ = pt_oracle.render(scene, dict(pb, seed=seed_b), accum=carried_acc.copy())
    assert (both[..., 3] >= 1).all() and both[..., 3].max() == 17
    raw1, raw2 = _error(one[..., :3] / one[..., 3:4], ref), _error(both[..., :3] / both[..., 3:4], ref)
    den1, den2 = _error(host.denoise_atrous(one, n1, a1)[..., :3], ref), _error(host.denoise_atrous(both, n1, a1)[..., :3], ref)
    print(f"carried {carried} of {hits} hit pixels ({carried / hits:.3f}); raw {raw1:.4f} -> {raw2:.4f}, ratio {raw2 / raw1:.3f}; "
          f"denoised {den1:.4f} -> {den2:.4f}, ratio {den2 / den1:.3f}")
    assert carried >= 0.8 * hits, (carried, hits)
    assert raw2 < raw1, (raw1, raw2)
    assert den2 < den1, (den1, den2)
