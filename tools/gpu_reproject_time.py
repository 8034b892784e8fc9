"""Device time of a camera move on the GPU box: glrtx_reproject (csrc/reproject.hip.h) at 1920x1080 on the headline scene, an orbit step of --degrees there and
back again, after a few 1-spp frames.

Timing: HIP events on the context's stream (glrtx_timer_begin / _end) around --reps back-to-back calls after --warmup calls, per call; the median of --trials
such timings.  Two things are timed that way: glrtx_render_features alone (alternating between the two cameras), and the whole glrtx_reproject call -- the same
feature pass, a memset of the counters and the reprojection kernel; the kernel's time is the difference of the two.  Compulsory bytes of the kernel per pixel:
32 read once (N1, A1), 48 read at least once (old accumulator, N0, A0: every old pixel is somebody's tap), 16 written; the other three taps per buffer are
what L1 and L2 are there to absorb.  The fraction given is bytes / (time x 6.29 TB/s), the float4-copy rate measured on this part.
For comparison, in the same context: one 1-spp frame (glrtx_stats.kernel_ms_last) and glrtx_clear (what a host without reprojection does on a move).
Writes the table to profiles/r15_reproject_time.txt (or --out) and prints it.

    python tools/gpu_reproject_time.py [--degrees 3] [--reps 20] [--warmup 3] [--trials 3] [--commit HASH] [--out profiles/r15_reproject_time.txt]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, scenes  # noqa: E402

HBM = 6.29e12  # bytes / s: the measured float4-copy rate


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def orbit(params, degrees):
    """params with the camera turned about the world's y axis through the origin (tests/reproject_math.py: move_camera 'orbit')."""
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    M = R @ np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    return dict(params, c2w=np.ascontiguousarray(M.T.reshape(16), np.float32))


degrees = float(arg("--degrees", 3.0))
reps, warmup, trials = int(arg("--reps", 20)), int(arg("--warmup", 3)), int(arg("--trials", 3))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r15_reproject_time.txt"))
W, H = 1920, 1080
PX = W * H

torch.cuda.init()
try:
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
except OSError:
    head = "?"
head = arg("--commit", head)  # (where the tree that runs is a copy without its history)
lines = [f"python tools/gpu_reproject_time.py --degrees {degrees:g} --reps {reps} --warmup {warmup} --trials {trials}",
         f"A camera move at {W}x{H} on one {torch.cuda.get_device_name(0)}; parent commit {head} plus this change; headline scene, an orbit step of {degrees:g} degrees there and "
         f"back; per call, {reps} calls per timing after {warmup}, median of {trials}; HBM figure {HBM / 1e12:.2f} TB/s", ""]


def timed(d, fn):
    k = 0
    for _ in range(warmup):
        fn(k); k += 1
    ts = []
    for _ in range(trials):
        d.sync()
        d.timer_begin()
        for _ in range(reps):
            fn(k); k += 1
        ts.append(d.timer_end() / reps)
    return float(np.median(ts)), ts


sc, pa = scenes.config_headline(W, H)
cams = [orbit(pa, degrees), pa]
d = device.Device(0)
d.set_variant(2); d.count_rays(False)
d.upload_scene(sc); d.resize(W, H); d.clear()
for f in range(3):
    d.clear(); d.render(dict(pa, seed=host.frame_seed(f))); d.sync()
frame_ms = d.stats().kernel_ms_last
clear_ms, _ = timed(d, lambda k: d.clear())
for f in range(4):
    d.render(dict(pa, seed=host.frame_seed(f)))
d.render_features(pa)
ft, ft_all = timed(d, lambda k: d.render_features(cams[k & 1]))
d.render_features(pa)
rp, rp_all = timed(d, lambda k: d.reproject(cams[k & 1]))
carried, hits = d.reproject_last()
kern = rp - ft
nbytes = 96 * PX
lines += [f"headline ({sc['tri'].shape[0]} triangles): one 1-spp frame {frame_ms:.3f} ms (render kernel); glrtx_clear {clear_ms * 1e3:.1f} us",
          f"  render_features alone      {ft * 1e3:8.1f} us   (trials: {', '.join(f'{t * 1e3:.1f}' for t in ft_all)})",
          f"  glrtx_reproject, the call  {rp * 1e3:8.1f} us   (trials: {', '.join(f'{t * 1e3:.1f}' for t in rp_all)})   = {rp / frame_ms * 100:.0f} % of one 1-spp frame",
          f"  reproject_kernel (+memset) {kern * 1e3:8.1f} us   (the difference)   compulsory {nbytes / 1e6:6.1f} MB   {nbytes / (max(kern, 1e-9) * 1e-3) / HBM * 100:5.1f} % of the HBM figure",
          f"  last call: {carried} of {hits} hit pixels carried history ({carried / max(hits, 1):.3f})", ""]
print("\n".join(lines), flush=True)
d.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
