"""Is carrying the history across a GEOMETRY move worth it, and does the motion vector do what the static reprojection cannot?  On the CPU (the oracle's renders,
the CPU statements -- which the device equals bit for bit, tests/test_gpu_reproject_motion.py): the headline scene at 192x108, max_depth 8, metric as in
tests/test_reproject_quality.py, sqrt(mean((x - ref)^2 / (ref^2 + 1e-2))) over rgb, truth 512 frames, 16 frames before the move, ONE after it.

Rigid equivalence.  Every vertex (positions and normals, the lamp included) turned by -3 degrees about the world's y axis, the tree refitted, the camera kept:
up to rounding the picture of tests/test_reproject_quality.py's +3 degree camera orbit.  Conditions: at least 80 % of the new view's hit pixels carry history
(the existing test's cap; the camera orbit measures 0.992), and the error with the carried history is strictly below the one frame alone, raw and denoised.
Measured: carried 14404 of 14519 hit pixels (0.992); raw 1.264 -> 0.271 (ratio 0.21), denoised 1.047 -> 0.245 (ratio 0.23).  The camera orbit
(tests/test_reproject_quality.py): carried 0.992; raw 0.913 -> 0.270, denoised 0.589 -> 0.243.  The share and the two errors WITH history agree to the third
place.  The one frame alone does not, and need not: the two scenes agree up to rounding only, a path's later bounces amplify that, and the two 1-spp frames
differ visibly in 27 % of their pixels (336 of 20,736 by more than 1.0) -- two draws of the same noise, in a metric that a handful of fireflies dominates.

One object moves.  The diffuse sphere at x = -1.1 (material 5) lifted by 0.3 in y, everything else and the camera fixed.  Over the pixels that show the sphere
after the move (A1.id == 5) the motion-aware result's error must be strictly below that of the static glrt_reproject given the same planes and one camera twice;
over the whole image it must beat the one frame alone, raw and denoised; and at least half of the sphere's pixels carry history -- a 0.3-unit lateral move at
about 14.5 units' distance turns the visible cap by about 1.2 degrees, so only the silhouette ring can lose its source.
Measured: 329 pixels show the sphere; with the motion vector all of them carry history (1.000), the static call finds history for 0.760 of them -- from
where the sphere used to be; error over them 0.398 (motion) against 0.905 (static) and 1.587 for the one frame alone.  Whole image: carried 14511 of 14556
hit pixels (0.997); raw 1.994 -> 0.330, denoised 1.857 -> 0.230."""
import numpy as np

import reproject_motion_math as rmm
from glrt_amd import host, scenes
from test_reproject_motion_host import lifted, moved_scene

W, H = 192, 108
TURN_DEGREES = -3.0
SPHERE, LIFT = 5, 0.3


def _error(x, ref, mask=None):
    e = (x.astype(np.float64) - ref) ** 2 / (ref.astype(np.float64) ** 2 + 1e-2)
    return float(np.sqrt(np.mean(e if mask is None else e[mask])))


def _frames(scene, params, n, f0=0, accum=None):
    from oracle import pt_oracle
    for f in range(n):
        accum, _ = pt_oracle.render(scene, dict(params, seed=host.frame_seed(f0 + f)), accum=accum)
    return accum


def _mean(acc):
    return acc[..., :3] / acc[..., 3:4]


def _before_and_after(v1):
    """16 frames and the planes before the move; the moved scene, its truth, its planes, one frame alone and that frame's seed offset."""
    scene, pa = scenes.config_headline(W, H)
    pa = dict(pa, max_depth=8)
    after = moved_scene(scene, v1(scene))
    ref = _frames(after, pa, 512)
    assert (ref[..., 3] == 512).all()
    acc_a = _frames(scene, pa, 16)
    n0, a0 = host.render_features(scene, pa, W, H)
    n1, a1, g1 = host.render_features_geom(after, pa, W, H)
    one = _frames(after, pa, 1, 2000)
    return scene, after, pa, _mean(ref), acc_a, (n0, a0), (n1, a1, g1), one


def test_rigid_turn_of_everything_equals_the_camera_orbit():
    scene, after, pa, ref, acc_a, (n0, a0), (n1, a1, g1), one = _before_and_after(lambda s: rmm.rotate_vertices(s["vert"], TURN_DEGREES))
    carried_acc, carried, hits = host.reproject_motion(acc_a, n0, a0, g1, a1, scene["vert"], scene["tri"], pa)
    both = _frames(after, pa, 1, 2000, carried_acc.copy())
    assert (both[..., 3] >= 1).all() and both[..., 3].max() == 17
    raw1, raw2 = _error(_mean(one), ref), _error(_mean(both), ref)
    den1, den2 = _error(host.denoise_atrous(one, n1, a1)[..., :3], ref), _error(host.denoise_atrous(both, n1, a1)[..., :3], ref)
    print(f"rigid turn: carried {carried} of {hits} hit pixels ({carried / hits:.3f}); raw {raw1:.4f} -> {raw2:.4f}, ratio {raw2 / raw1:.3f}; "
          f"denoised {den1:.4f} -> {den2:.4f}, ratio {den2 / den1:.3f}")
    assert carried >= 0.8 * hits, (carried, hits)
    assert raw2 < raw1, (raw1, raw2)
    assert den2 < den1, (den1, den2)


def test_one_lifted_sphere_keeps_its_history_where_the_static_call_does_not():
    scene, after, pa, ref, acc_a, (n0, a0), (n1, a1, g1), one = _before_and_after(lambda s: lifted(s, SPHERE, LIFT))
    on = a1[..., 3].view(np.int32) == SPHERE
    assert on.sum() > 100
    motion, carried, hits = host.reproject_motion(acc_a, n0, a0, g1, a1, scene["vert"], scene["tri"], pa)
    static, carried_s, _ = host.reproject(acc_a, n0, a0, n1, a1, pa, pa)
    both_m = _frames(after, pa, 1, 2000, motion.copy())
    both_s = _frames(after, pa, 1, 2000, static.copy())
    share = float((motion[..., 3][on] != 0).mean())
    share_s = float((static[..., 3][on] != 0).mean())
    err_m, err_s, err_1 = _error(_mean(both_m), ref, on), _error(_mean(both_s), ref, on), _error(_mean(one), ref, on)
    raw1, raw2 = _error(_mean(one), ref), _error(_mean(both_m), ref)
    den1, den2 = _error(host.denoise_atrous(one, n1, a1)[..., :3], ref), _error(host.denoise_atrous(both_m, n1, a1)[..., :3], ref)
    print(f"lifted sphere: {int(on.sum())} pixels; carrying history: motion {share:.3f}, static {share_s:.3f}; error over them: motion {err_m:.4f}, "
          f"static {err_s:.4f}, one frame {err_1:.4f}; whole image: carried {carried} of {hits} ({carried / hits:.3f}; static {carried_s}), "
          f"raw {raw1:.4f} -> {raw2:.4f}, denoised {den1:.4f} -> {den2:.4f}")
    assert err_m < err_s, (err_m, err_s)
    assert raw2 < raw1, (raw1, raw2)
    assert den2 < den1, (den1, den2)
    assert share >= 0.5, share
