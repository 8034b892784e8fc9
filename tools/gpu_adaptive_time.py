"""Adaptive sampling (glrtx_render_adaptive) against uniform frames on the GPU box, at 1080p, 1 sample per pixel per frame.

Per scene: a 1024-frame uniform image is the ground truth G.  Then, from a cleared accumulator, uniform bursts (glrtx_render_frames) and adaptive
bursts (glrtx_render_adaptive, per threshold) of --burst frames, each timed on the host around issue + sync (the read-back for the error is outside the
clock), and on the device (glrtx_stats: render kernel + accumulation pass).  rMSE = mean over pixels and channels of (I - G)^2 / (G^2 + 1e-2).
Every shape that is timed is warmed up first: two uniform bursts (a fed launch takes its own pipe slot: the second burst's is allocated then) and two
adaptive ones.  Each setting runs --reps times; the summary gives the median and the range over the repetitions of: the time to reach the uniform
run's rMSE after 64 frames (wall and device time, interpolated linearly between bursts), the rMSE at equal wall time (log-linear between bursts), the
device time per burst, the active fraction and the Mrays/s of the launches (ray counting on in every run: the counting instantiations on both sides).
Besides the fixed thresholds, a LOW setting takes the 90th percentile of the tile errors after 64 nothing-retires frames as its threshold, so that about
a tenth of the tiles stays active; it is run with bursts of --burst and of 4 x --burst frames (more frames per call at a low active fraction).
The selection alone: n_frames = 0 calls back to back (host clock, launch overhead included); kernel times come from a separate
`rocprofv3 --kernel-trace --stats` run of this tool.  One JSON line per scene and setting.

    python tools/gpu_adaptive_time.py [--scenes headline,c5] [--thresholds 0.05,0.01] [--burst 16] [--budget 256] [--min-spp 8] [--reps 3]"""
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


names = arg("--scenes", "headline,c5").split(",")
thresholds = [float(v) for v in arg("--thresholds", "0.05,0.01").split(",")]
burst, budget, min_spp = int(arg("--burst", 16)), int(arg("--budget", 256)), int(arg("--min-spp", 8))
reps, truth_frames = int(arg("--reps", 3)), int(arg("--truth", 1024))


def image(acc):
    return acc[..., :3] / np.maximum(acc[..., 3:], 1.0)


def rmse(acc, gt):
    return float((((image(acc) - gt) ** 2) / (gt ** 2 + 1e-2)).mean())


def seeds(f0, n):
    return [host.frame_seed(f0 + i) for i in range(n)]


def run(d, params, gt, thr, b=burst):
    """thr None: uniform bursts; else adaptive bursts.  Returns the per-burst trace (cumulative wall / device ms)."""
    d.clear(); d.sync(); d.reset_stats(); d.count_rays(True)
    trace, t, dev, f = [], 0.0, 0.0, 0
    while f < budget:
        st0 = d.stats()
        t0 = time.perf_counter()
        if thr is None:
            d.render_frames(params, seeds(10_000 + f, b))
        else:
            d.render_adaptive(params, seeds(10_000 + f, b), thr, min_spp)
        d.sync()
        t += time.perf_counter() - t0
        f += b
        st = d.stats()
        active, total = d.adaptive_active_tiles() if thr is not None else (1, 1)
        kms = st.kernel_ms_total - st0.kernel_ms_total
        dev += kms + st.accumulate_ms_total - st0.accumulate_ms_total
        trace.append(dict(frames=f, wall_ms=round(t * 1e3, 3), device_ms=round(dev, 3), active=round(active / total, 4), rmse=rmse(d.read_accum(), gt),
                          kernel_ms=round(kms, 3), acc_ms=round(st.accumulate_ms_total - st0.accumulate_ms_total, 4),
                          launches=int(st.kernel_launches - st0.kernel_launches), mrays_s=round((st.rays - st0.rays) / max(kms, 1e-6) / 1e3, 1)))
    d.count_rays(False)
    return trace


def time_to(trace, target, key):
    """The time at which the rMSE reaches target, linear between the bursts around the crossing (None: not reached)."""
    prev = dict(rmse=float("inf"), **{key: 0.0})
    for r in trace:
        if r["rmse"] <= target:
            if not np.isfinite(prev["rmse"]):
                return r[key]
            a = (prev["rmse"] - target) / (prev["rmse"] - r["rmse"])
            return prev[key] + a * (r[key] - prev[key])
        prev = r
    return None


def rmse_at(trace, t_ms):
    """rMSE at wall time t, log-linear between bursts (None outside the run)."""
    ts = [r["wall_ms"] for r in trace]
    if t_ms < ts[0] or t_ms > ts[-1]:
        return None
    return float(np.exp(np.interp(t_ms, ts, [np.log(r["rmse"]) for r in trace])))


def spread(vals):
    v = [x for x in vals if x is not None]
    if not v:
        return None
    return dict(median=round(float(np.median(v)), 4), min=round(float(min(v)), 4), max=round(float(max(v)), 4), n=len(v))


def summary(name, setting, traces, target, marks, **extra):
    return dict(scene=name, setting=setting, reps=len(traces), **extra,
                time_to_target_wall_ms=spread([time_to(t, target, "wall_ms") for t in traces]),
                time_to_target_device_ms=spread([time_to(t, target, "device_ms") for t in traces]),
                rmse_at_wall_ms={str(m): spread([rmse_at(t, m) for t in traces]) for m in marks},
                device_ms_per_burst=spread([t[-1]["device_ms"] / len(t) for t in traces]),
                active_first_last=[traces[0][0]["active"], traces[0][-1]["active"]],
                mrays_s_first_last=[spread([t[0]["mrays_s"] for t in traces]), spread([t[-1]["mrays_s"] for t in traces])],
                frames_run=traces[0][-1]["frames"], trace_rep0=traces[0])


d = device.Device()
for name in names:
    scene, params = scenes.CONFIGS[name](width=1920, height=1080, n_samples=1)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(1920, 1080)
    # warm-up of every shape that is timed: two uniform bursts (the second fed launch takes a second pipe slot), two adaptive ones
    for _ in range(2):
        d.render_frames(params, seeds(0, burst)); d.sync()
    for _ in range(2):
        d.render_adaptive(params, seeds(0, burst), -1.0, 2); d.sync()
    d.render_adaptive(params, seeds(0, 4 * burst), -1.0, 2); d.sync()
    d.clear()
    t0 = time.perf_counter()
    for f0 in range(0, truth_frames, 64):
        d.render_frames(params, seeds(100_000 + f0, 64))
    d.sync()
    gt = image(d.read_accum())
    print(json.dumps(dict(scene=name, setting="truth", frames=truth_frames, wall_ms_per_frame=round((time.perf_counter() - t0) * 1e3 / truth_frames, 3))), flush=True)
    uni = [run(d, params, gt, None) for _ in range(reps)]
    target = float(np.median([next(r["rmse"] for r in t if r["frames"] >= 64) for t in uni]))
    marks = [round(float(np.median([t[k]["wall_ms"] for t in uni])), 1) for k in range(len(uni[0])) if uni[0][k]["frames"] in (32, 64, 128, 256)]
    print(json.dumps(summary(name, "uniform", uni, target, marks, target_rmse=target, burst=burst)), flush=True)
    # LOW: the 90th percentile of the tile errors after 64 frames in which nothing retires
    d.clear()
    d.render_adaptive(params, seeds(10_000, 64), -1.0, 2)
    _, err, _ = device.adaptive_select(d.read_accum(), d.read_adaptive_half(), -1.0, 2)
    low = float(np.quantile(err[np.isfinite(err)], 0.9))
    settings = [(f"adaptive {thr}", thr, burst) for thr in thresholds] + [("adaptive low", low, burst), ("adaptive low, 4x burst", low, 4 * burst)]
    for label, thr, b in settings:
        ad = [run(d, params, gt, thr, b) for _ in range(reps)]
        d.sync(); t0 = time.perf_counter()
        for _ in range(50):  # the selection alone, on the state the last run ended with
            d.render_adaptive(params, [], thr, min_spp)
        d.sync()
        sel_us = (time.perf_counter() - t0) * 1e6 / 50
        acc_us = 1e3 * sum(r["acc_ms"] for t in ad for r in t) / max(1, sum(r["launches"] for t in ad for r in t))
        print(json.dumps(summary(name, label, ad, target, marks, threshold=round(thr, 5), min_spp=min_spp, burst=b, select_us_per_call_host=round(sel_us, 2),
                                 masked_accumulate_us_per_launch=round(acc_us, 2))), flush=True)
d.close()
