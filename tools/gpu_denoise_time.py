"""Device time of the denoiser on the GPU box: glrtx_render_features (csrc/features.hip.h) and glrtx_denoise (csrc/denoise.hip.h) per iteration count, at
1920x1080 on the headline scene and config 5, after one 1-spp frame.

Timing: HIP events on the context's stream (glrtx_timer_begin / _end) around --reps back-to-back calls after --warmup calls, per call; the median of --trials
such timings.  Per kernel the fraction of the HBM figure its COMPULSORY bytes would take: bytes / (time x 6.29 TB/s), the float4-copy rate measured on this
part (8.0 TB/s is the specification).  Compulsory bytes per pixel: features 32 written (two float4); prep 32 read (accumulator, albedo) + 16 written; one
filter iteration 32 read (colour, normal/depth) + 16 written, the last one reads the albedo too (16) when demodulating.  The 25 x 32 bytes of tap traffic per
pixel and iteration are not compulsory: they are what the LDS tiles (spacings 1, 2) and the caches (spacing >= 4) are there to absorb.
For comparison, in the same context: the stand-alone resolve kernel (glrtx_debug_resolve_burst) and one 1-spp frame (glrtx_stats.kernel_ms_last).
Writes the table to profiles/r14_denoise_time.txt (or --out) and prints it.

    python tools/gpu_denoise_time.py [--scenes headline,c5] [--reps 20] [--warmup 3] [--trials 3] [--commit HASH] [--out profiles/r14_denoise_time.txt]"""
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


names = arg("--scenes", "headline,c5").split(",")
reps, warmup, trials = int(arg("--reps", 20)), int(arg("--warmup", 3)), int(arg("--trials", 3))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r14_denoise_time.txt"))
W, H = 1920, 1080
PX = W * H

torch.cuda.init()
try:
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
except OSError:
    head = "?"
head = arg("--commit", head)  # (where the tree that runs is a copy without its history)
lines = [f"The denoiser at {W}x{H} on one {torch.cuda.get_device_name(0)}; parent commit {head} plus this change; per call, {reps} calls per timing after {warmup}, "
         f"median of {trials}; HBM figure {HBM / 1e12:.2f} TB/s", ""]
print(lines[0], flush=True)


def timed(d, fn):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(trials):
        d.sync()
        d.timer_begin()
        for _ in range(reps):
            fn()
        ts.append(d.timer_end() / reps)
    return float(np.median(ts))


for name in names:
    sc, params = scenes.CONFIGS[name](width=W, height=H)
    d = device.Device(0)
    d.set_variant(2); d.count_rays(False)
    d.upload_scene(sc); d.resize(W, H); d.clear()
    for f in range(3):
        d.clear(); d.render(dict(params, seed=host.frame_seed(f))); d.sync()
    frame_ms = d.stats().kernel_ms_last
    resolve_ms = d.resolve_burst_ms(2.2, 32)
    lines.append(f"{name} ({sc['tri'].shape[0]} triangles): one 1-spp frame {frame_ms:.3f} ms (render kernel), stand-alone resolve_kernel {resolve_ms * 1e3:.1f} us")
    ft = timed(d, lambda: d.render_features(params))
    lines.append(f"  render_features            {ft * 1e3:8.1f} us   compulsory {32 * PX / 1e6:6.1f} MB   {32 * PX / (ft * 1e-3) / HBM * 100:5.1f} % of the HBM figure "
                 f"(a traversal: paced by the tree walk, not by its 66 MB of stores)")
    prev = 0.0
    for demod in (1, 0):
        for it in range(1, 7):
            t = timed(d, lambda: d.denoise(iterations=it, demodulate=demod))
            nbytes = PX * (48 + 48 * it + (16 if demod else 0))
            lines.append(f"  denoise it={it} demodulate={demod}  {t * 1e3:8.1f} us   (+{(t - prev) * 1e3:7.1f} us for this iteration)   compulsory {nbytes / 1e6:6.1f} MB   "
                         f"{nbytes / (t * 1e-3) / HBM * 100:5.1f} % of the HBM figure")
            prev = t
        prev = 0.0
    lines.append("")
    print("\n".join(lines[-16:]), flush=True)
    d.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
