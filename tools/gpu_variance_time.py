"""Device times of variance guidance on the GPU box, one process, one context, 1920x1080 headline scene (include/glrtx.h "Variance guidance").

Timing: HIP events on the context's stream (glrtx_timer_begin / _end) around --reps back-to-back calls after --warmup calls, per call; the median of --trials
such timings (tools/gpu_reproject_time.py's method).  Timed: glrtx_denoise and glrtx_denoise_variance at 1 .. 5 iterations (the differences are the
iterations; denoise_variance at 1 iteration minus denoise at 1 iteration is the variance pass plus what the first guided iteration costs over the plain one),
on the temporal branch (16 samples in M) and on the spatial branch (1 sample); glrtx_render_moments of 16 frames beside glrtx_render_adaptive with a
threshold < 0 for the same 16 frames (the same launch shape: the difference is the fold); glrtx_reproject with tracking on beside tracking off.
Writes profiles/r17_variance_time.txt (or --out) and prints it.

    python tools/gpu_variance_time.py [--reps 10] [--warmup 2] [--trials 3] [--out profiles/r17_variance_time.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def orbit(params, degrees):
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    M = R @ np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    return dict(params, c2w=np.ascontiguousarray(M.T.reshape(16), np.float32))


reps, warmup, trials = int(arg("--reps", 10)), int(arg("--warmup", 2)), int(arg("--trials", 3))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r17_variance_time.txt"))
W, H = 1920, 1080
torch.cuda.init()
lines = [f"python tools/gpu_variance_time.py --reps {reps} --warmup {warmup} --trials {trials}",
         f"{W}x{H} headline scene on one {torch.cuda.get_device_name(0)}, one process, one context; HIP events around {reps} back-to-back calls after {warmup}, per call, "
         f"median of {trials}", ""]


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
    return float(np.median(ts))


sc, pa = scenes.config_headline(W, H)
cams = [orbit(pa, 3.0), pa]
seeds = [host.frame_seed(f) for f in range(16)]
d = device.Device(0)
d.set_variant(2); d.count_rays(False)
d.upload_scene(sc); d.resize(W, H); d.clear()
d.track_moments(True)

# 1. the fold: render_moments against render_adaptive(threshold < 0), 16 frames a call
ad = timed(d, lambda k: d.render_adaptive(pa, seeds, -1.0, 2))
mo = timed(d, lambda k: d.render_moments(pa, seeds))
lines += ["16 frames in one call (ms per call):",
          f"  render_adaptive, threshold < 0   {ad:8.3f}",
          f"  render_moments                   {mo:8.3f}   ({(mo / ad - 1) * 100:+.1f} %)", ""]

# 2. the filters
for spp, what in ((16, "temporal branch (M.w = 16)"), (1, "spatial branch (M.w = 1)")):
    d.clear()
    d.render_moments(pa, seeds[:spp])
    d.render_features(pa)
    fx = [timed(d, lambda k, it=it: d.denoise(iterations=it)) for it in range(1, 6)]
    vr = [timed(d, lambda k, it=it: d.denoise_variance(iterations=it)) for it in range(1, 6)]
    lines += [f"filters, {what} (us per call):", "  iterations        " + "".join(f"{it:9d}" for it in range(1, 6)),
              "  denoise           " + "".join(f"{t * 1e3:9.1f}" for t in fx),
              "  denoise_variance  " + "".join(f"{t * 1e3:9.1f}" for t in vr),
              "  per added iteration, denoise / denoise_variance: " + ", ".join(f"{(fx[i] - fx[i - 1]) * 1e3:.1f} / {(vr[i] - vr[i - 1]) * 1e3:.1f}" for i in range(1, 5)),
              f"  variance pass + the first guided iteration's extra cost: {(vr[0] - fx[0]) * 1e3:.1f} us", ""]

# 3. reproject with tracking on against off (the same context: M exists / tracking switched off)
d.clear(); d.render_moments(pa, seeds[:4]); d.render_features(pa)
on = timed(d, lambda k: d.reproject(cams[k & 1]))
d.track_moments(False)
d.render_features(pa)
off = timed(d, lambda k: d.reproject(cams[k & 1]))
lines += ["glrtx_reproject, an orbit step of 3 degrees there and back (us per call, feature pass included):",
          f"  tracking off  {off * 1e3:8.1f}", f"  tracking on   {on * 1e3:8.1f}   ({(on / off - 1) * 100:+.1f} %)", ""]
print("\n".join(lines), flush=True)
d.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
