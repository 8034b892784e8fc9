"""Device time of a geometry move on the GPU box: glrtx_reproject_motion (csrc/reproject_motion.hip.h) against glrtx_reproject on the same 1920x1080 headline
view pair (an orbit step of --degrees there and back), the feature pass with and without the geometry plane, and glrtx_update_vertices with and without
motion tracking (headline and config 5).

One process, one context, HIP events on the context's stream (glrtx_timer_begin / _end) throughout.
Calls: --reps back-to-back calls after --warmup calls, per call; the two sides ALTERNATE trial by trial (static, motion, static, ...; tracking is switched for
each side, with a feature pass after the switch), and the median of --trials such timings per side is reported.  In these runs nothing moved since the last
feature pass, so every motion call also runs the snapshot kernel (previous = current).  The motion call of a host that DID move is timed one call at a time:
a glrtx_update_vertices (blocking, outside the events), then the events around the one call; the median of --reps x --trials calls.  The reprojection
kernel's time is that call minus the feature pass with G; the snapshot kernel's is the difference of the two motion figures, and again the difference of the
refit with tracking on and off below.
Refit: the events around one glrtx_update_vertices (host vertices: the copy to the device, the snapshot with tracking on, the three refit kernels, the
read-back), a feature pass before each one outside the events so that every call with tracking on takes the snapshot; tracking alternates call by call; the
median per side.
Compulsory bytes of the motion kernel per pixel: 32 read once (G1, A1), 48 read at least once (old accumulator, N0, A0), 16 written, plus 96 per triangle of
the previous geometry; the fraction given is bytes / (time x 6.29 TB/s), the float4-copy rate measured on this part.
Writes the table to profiles/r16_reproject_motion_time.txt (or --out) and prints it.

    python tools/gpu_reproject_motion_time.py [--degrees 3] [--reps 20] [--warmup 3] [--trials 5] [--commit HASH] [--out FILE]"""
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
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    M = R @ np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    return dict(params, c2w=np.ascontiguousarray(M.T.reshape(16), np.float32))


degrees = float(arg("--degrees", 3.0))
reps, warmup, trials = int(arg("--reps", 20)), int(arg("--warmup", 3)), int(arg("--trials", 5))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r16_reproject_motion_time.txt"))
W, H = 1920, 1080
PX = W * H

torch.cuda.init()
try:
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
except OSError:
    head = "?"
head = arg("--commit", head)
lines = [f"python tools/gpu_reproject_motion_time.py --degrees {degrees:g} --reps {reps} --warmup {warmup} --trials {trials}",
         f"A geometry move at {W}x{H} on one {torch.cuda.get_device_name(0)}; parent commit {head} plus this change; headline scene, an orbit step of {degrees:g} degrees "
         f"there and back; per call, {reps} calls per timing after {warmup}, the two sides alternating, median of {trials}; HBM figure {HBM / 1e12:.2f} TB/s", ""]


def once(d, fn, k0):
    k = k0
    for _ in range(warmup):
        fn(k); k += 1
    d.sync()
    d.timer_begin()
    for _ in range(reps):
        fn(k); k += 1
    return d.timer_end() / reps


def fmt(ts):
    return ", ".join(f"{t * 1e3:.1f}" for t in ts)


sc, pa = scenes.config_headline(W, H)
cams = [orbit(pa, degrees), pa]
n_tri = sc["tri"].shape[0]
v = [np.ascontiguousarray(np.asarray(sc["vert"], np.float32).reshape(-1, 15)).copy() for _ in range(2)]
v[1][:, 1] += np.float32(0.01)
d = device.Device(0)
d.set_variant(2); d.count_rays(False)
d.upload_scene(sc); d.resize(W, H); d.clear()
for f in range(4):
    d.render(dict(pa, seed=host.frame_seed(f)))
res = {k: [] for k in ("ft_off", "ft_on", "static", "motion")}
for _ in range(trials):
    d.track_motion(False); d.render_features(pa)
    res["ft_off"].append(once(d, lambda k: d.render_features(cams[k & 1]), 0))
    d.render_features(pa)
    res["static"].append(once(d, lambda k: d.reproject(cams[k & 1]), 0))
    d.track_motion(True); d.render_features(pa)
    res["ft_on"].append(once(d, lambda k: d.render_features(cams[k & 1]), 0))
    d.render_features(pa)
    res["motion"].append(once(d, lambda k: d.reproject_motion(cams[k & 1]), 0))
carried, hits = d.reproject_last()
moved = []
for k in range(warmup + reps * trials):  # the geometry moved: the snapshot was taken by the update, not by the call
    d.update_vertices(v[(k + 1) & 1])
    d.timer_begin()
    d.reproject_motion(cams[k & 1])
    t = d.timer_end()
    if k >= warmup:
        moved.append(t)
d.update_vertices(v[0])
med = {k: float(np.median(x)) for k, x in res.items()}
med["moved"] = float(np.median(moved))
k_static, k_motion = med["static"] - med["ft_off"], med["moved"] - med["ft_on"]
b_static, b_motion = 96 * PX, 96 * PX + 96 * n_tri


def share(nbytes, ms):
    return f"compulsory {nbytes / 1e6:6.1f} MB   {nbytes / (max(ms, 1e-9) * 1e-3) / HBM * 100:5.1f} % of the HBM figure"


lines += [f"headline ({n_tri} triangles)",
          "glrtx_reproject (tracking off):",
          f"  render_features alone             {med['ft_off'] * 1e3:8.1f} us   (trials: {fmt(res['ft_off'])})",
          f"  the call                          {med['static'] * 1e3:8.1f} us   (trials: {fmt(res['static'])})",
          f"  reproject_kernel (+memset)        {k_static * 1e3:8.1f} us   (the difference)   {share(b_static, k_static)}",
          "glrtx_reproject_motion (tracking on):",
          f"  render_features alone, with G     {med['ft_on'] * 1e3:8.1f} us   (trials: {fmt(res['ft_on'])})   = {med['ft_on'] / med['ft_off']:.3f} of the pass without G",
          f"  the call, nothing moved           {med['motion'] * 1e3:8.1f} us   (trials: {fmt(res['motion'])})   (with the snapshot kernel inside)",
          f"  the call, after an update         {med['moved'] * 1e3:8.1f} us   (single calls: min {min(moved) * 1e3:.1f}, max {max(moved) * 1e3:.1f}, n {len(moved)})",
          f"  reproject_motion_kernel (+memset) {k_motion * 1e3:8.1f} us   (after an update, minus the pass with G)   {share(b_motion, k_motion)}",
          f"  snapshot_kernel                   {(med['motion'] - med['moved']) * 1e3:8.1f} us   (nothing moved minus after an update)",
          f"  motion call / static call = {med['moved'] / med['static']:.3f} after an update, {med['motion'] / med['static']:.3f} with nothing moved",
          f"  last back-to-back motion call: {carried} of {hits} hit pixels carried history ({carried / max(hits, 1):.3f})", ""]
print("\n".join(lines), flush=True)


def refit_times(what, params, verts):
    ts = {False: [], True: []}
    for r in range(2 * (reps + warmup)):
        on = bool(r & 1)
        d.track_motion(on)
        d.render_features(params); d.sync()
        d.timer_begin()
        d.update_vertices(verts[(r >> 1) & 1])
        t = d.timer_end()
        if r >= 2 * warmup:
            ts[on].append(t)
    off, on = float(np.median(ts[False])), float(np.median(ts[True]))
    return f"  {what:28s} glrtx_update_vertices (host vertices): tracking off {off:.3f} ms, on {on:.3f} ms (the snapshot: {(on - off) * 1e3:+.1f} us)"


lines.append("The refit with the snapshot of the previous geometry (events around one call; median of %d per side):" % reps)
lines.append(refit_times(f"headline ({n_tri} triangles)", pa, v))
s5, p5 = scenes.config_c5(W, H)
d.upload_scene(s5)
v5 = [np.ascontiguousarray(np.asarray(s5["vert"], np.float32).reshape(-1, 15)).copy() for _ in range(2)]
v5[1][:, 1] += np.float32(0.01)
lines.append(refit_times(f"config 5 ({s5['tri'].shape[0]} triangles)", p5, v5))
lines.append("")
print("\n".join(lines[-4:]), flush=True)
d.close()
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print("wrote", out_path)
