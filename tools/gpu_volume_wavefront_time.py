"""The volume on the wavefront kernel (glrtx_set_volume_wavefront: pt_render_wgwf's V form) against the persistent megakernel's volume instantiation,
on the GPU box: the 1080p fire scene (scenes.config_fire: 64^3 grid, 8 bounces, 1 sample per pixel per frame), one context, GLRTX_VOLUME_WAVEFRONT
alternating per setting (read at every launch).  Settings, each --reps times in rotating order after --warmup frames of its own:

  persistent    --frames glrtx_render calls on the megakernel (GLRTX_VOLUME_WAVEFRONT=0)
  v_frames      one --frames-frame glrtx_render_frames call on the V form
  v_fed         --frames glrtx_render calls on the V form (fed: they run as one launch)

Time per frame: host wall clock around issue + sync, and device time (glrtx_stats: render kernel + accumulation pass, over the frames).  Rays per frame
from one counting frame per form (every Woodcock trial ray included; equal on both forms).  Then adaptive sampling with the volume on (the V form) against
uniform bursts, as tools/gpu_adaptive_time.py does: the time to reach the rMSE that uniform frames have after --target-frames frames, against a
--truth-frame ground truth.  One JSON line per setting, then a summary line.

    python tools/gpu_volume_wavefront_time.py [--frames 20] [--warmup 3] [--reps 5] [--thresholds 0.05,0.01] [--burst 8] [--budget 128]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


frames, warmup, reps = int(arg("--frames", 20)), int(arg("--warmup", 3)), int(arg("--reps", 5))
thresholds = [float(v) for v in arg("--thresholds", "0.05,0.01").split(",")]
burst, budget, truth_frames, target_frames = int(arg("--burst", 8)), int(arg("--budget", 128)), int(arg("--truth", 512)), int(arg("--target-frames", 64))
w, h = 1920, 1080


def seeds(f0, n):
    return [host.frame_seed(f0 + i) for i in range(n)]


def form(v):
    os.environ["GLRTX_VOLUME_WAVEFRONT"] = "1" if v else "0"


scene, params, vol = scenes.config_fire(w, h, max_depth=8, n_samples=1, grid=64)
d = device.Device()
d.upload_scene(scene)
d.upload_volume(vol["density"], vol["temperature"], vol["bbox_min"], vol["bbox_max"])
d.set_extensions(device.EXT_VOLUME)
d.set_partition(0, 1, 16)
d.resize(w, h)


def issue(setting, f0, n):
    if setting == "v_frames":
        d.render_frames(params, seeds(f0, n))
    else:
        for sd in seeds(f0, n):
            d.render(dict(params, seed=sd))


def timed(setting, f0):
    form(setting != "persistent")
    d.clear(); d.sync()
    issue(setting, f0, warmup); d.sync()
    d.reset_stats()
    t0 = time.perf_counter()
    issue(setting, f0 + warmup, frames)
    d.sync()
    wall = (time.perf_counter() - t0) * 1e3 / frames
    st = d.stats()
    return dict(wall_ms_per_frame=wall, device_ms_per_frame=(st.kernel_ms_total + st.accumulate_ms_total) / frames,
                kernel_ms_per_frame=st.kernel_ms_total / frames, variant=int(st.variant_last), kernel_launches=int(st.kernel_launches),
                feed_appended=int(st.feed_appended))


rays = {}
for v in (False, True):
    form(v)
    d.clear(); d.reset_stats(); d.count_rays(True)
    d.render(dict(params, seed=host.frame_seed(0))); d.sync()
    rays[v] = int(d.stats().rays)
    d.count_rays(False)

settings = ["persistent", "v_frames", "v_fed"]
runs = {s: [] for s in settings}
for r in range(reps):
    for k in range(len(settings)):
        s = settings[(k + r) % len(settings)]
        runs[s].append(timed(s, 1000 * (r + 1)))
med = {}
for s in settings:
    keys = ("wall_ms_per_frame", "device_ms_per_frame", "kernel_ms_per_frame")
    m = {k: round(float(np.median([x[k] for x in runs[s]])), 4) for k in keys}
    m.update({k + "_range": [round(min(x[k] for x in runs[s]), 4), round(max(x[k] for x in runs[s]), 4)] for k in keys})
    med[s] = m
    rr = rays[s != "persistent"]
    print(json.dumps(dict(scene="fire", setting=s, width=w, height=h, depth=8, grid=64, frames=frames, reps=reps, rays_per_frame=rr,
                          mrays_per_s_wall=round(rr / m["wall_ms_per_frame"] / 1e3, 1), variant=runs[s][0]["variant"],
                          kernel_launches=runs[s][0]["kernel_launches"], feed_appended=runs[s][0]["feed_appended"], **m)), flush=True)


# ---- adaptive sampling with the volume on (V form) against uniform bursts
def image(acc):
    return acc[..., :3] / np.maximum(acc[..., 3:], 1.0)


def rmse(acc, gt):
    return float((((image(acc) - gt) ** 2) / (gt ** 2 + 1e-2)).mean())


form(True)
d.clear(); d.sync()
for f0 in range(0, truth_frames, 64):
    d.render_frames(params, seeds(100_000 + f0, min(64, truth_frames - f0)))
d.sync()
gt = image(d.read_accum())


def run(thr):
    d.clear(); d.sync(); d.reset_stats()
    trace, t, f = [], 0.0, 0
    while f < budget:
        t0 = time.perf_counter()
        if thr is None:
            d.render_frames(params, seeds(10_000 + f, burst))
        else:
            d.render_adaptive(params, seeds(10_000 + f, burst), thr, 8)
        d.sync()
        t += time.perf_counter() - t0
        f += burst
        active, total = d.adaptive_active_tiles() if thr is not None else (1, 1)
        trace.append(dict(frames=f, wall_ms=round(t * 1e3, 3), active=round(active / total, 4), rmse=rmse(d.read_accum(), gt)))
    return trace


def time_to(trace, target):
    prev = dict(rmse=float("inf"), wall_ms=0.0)
    for r in trace:
        if r["rmse"] <= target:
            if not np.isfinite(prev["rmse"]):
                return r["wall_ms"]
            a = (prev["rmse"] - target) / (prev["rmse"] - r["rmse"])
            return round(prev["wall_ms"] + a * (r["wall_ms"] - prev["wall_ms"]), 3)
        prev = r
    return None


for _ in range(2):  # warm-up of both shapes
    run(None); run(thresholds[0])
uniform = [run(None) for _ in range(3)]
target = float(np.median([next(r["rmse"] for r in t if r["frames"] >= target_frames) for t in uniform]))
print(json.dumps(dict(scene="fire", setting="uniform", target_rmse=target, target_frames=target_frames, burst=burst, budget=budget,
                      time_to_target_wall_ms=[time_to(t, target) for t in uniform], trace_rep0=uniform[0])), flush=True)
for thr in thresholds:
    tr = [run(thr) for _ in range(3)]
    print(json.dumps(dict(scene="fire", setting=f"adaptive {thr}", target_rmse=target, burst=burst, budget=budget, min_spp=8,
                          time_to_target_wall_ms=[time_to(t, target) for t in tr], active_first_last=[tr[0][0]["active"], tr[0][-1]["active"]],
                          trace_rep0=tr[0])), flush=True)
os.environ.pop("GLRTX_VOLUME_WAVEFRONT", None)
d.set_extensions(0)
d.close()
