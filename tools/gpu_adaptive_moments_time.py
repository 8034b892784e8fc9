"""Adaptive sampling by variance (glrtx_render_adaptive_moments) on the GPU box, in one context, headline scene, 1 sample per pixel per frame.

Three measurements, each with its variants alternating inside the run, --rounds times after a warm-up pass; the median and the range are printed.
  selection    glrtx_render_adaptive_moments against glrtx_render_adaptive with n_frames = 0 at 1920x1080: --reps calls back to back between the context's timer
               calls, per call.  A call is the selection kernel plus adaptive_compact_kernel (one workgroup, the same in both forms), so the two forms differ by
               their selection kernels alone; the kernels' own times come from a run of this tool under `rocprofv3 --kernel-trace --stats -- python3
               tools/gpu_adaptive_moments_time.py --only selection`.
  masked fold  16 frames at 1920x1080 through render_adaptive_moments (threshold -1), glrtx_render_moments and glrtx_render_adaptive (threshold -1): the
               call between the timer calls, and the accumulation pass's share (glrtx_stats.accumulate_ms_total).
  scenario     at 1920x1080 and 192x108: 16 frames with render_moments, a 3-degree orbit step through glrtx_reproject, then 8 frames by the H form, by the M form
               (its threshold the median tile error before the move: about half the tiles would retire there; min_samples 4) or uniformly (render_moments).
               Per path: the active share right after the move, the device time of the 8 frames (timer around the call: selection, render kernel, pass), and
               the relative rMSE -- mean of (I - G)^2 / (G^2 + 1e-2) -- against a --truth frame image G of the new view, raw and after glrtx_denoise_variance.

    python tools/gpu_adaptive_moments_time.py [--out profiles/r21_adaptive_moments.txt] [--rounds 5] [--reps 50] [--truth 512] [--only selection|fold|scenario]"""
import os
import sys

import numpy as np
import torch  # (before libglrtx is loaded: torch brings its own copy of the HIP runtime and wants to initialise first)

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


out_path, rounds, reps, truth, only = arg("--out", ""), int(arg("--rounds", 5)), int(arg("--reps", 50)), int(arg("--truth", 512)), arg("--only", "")
W, H = 1920, 1080
HBM = 6.29e12  # bytes / s: the measured float4-copy rate
lines = [f"adaptive sampling by variance on one {torch.cuda.get_device_name(0)}, headline scene, one context; median [min .. max] of {rounds} rounds, the variants "
         "alternating inside every round", ""]


def say(s=""):
    lines.append(s)
    print(s, flush=True)


def spread(v, unit, scale=1.0, w=9, p=1):
    v = np.array(v, np.float64) * scale
    return f"{np.median(v):{w}.{p}f} {unit}  [{v.min():{w}.{p}f} .. {v.max():{w}.{p}f}]"


def seeds(f0, n):
    return [host.frame_seed(f0 + i) for i in range(n)]


def orbit(params, degrees):
    """params with the camera turned about the world's y axis through the origin (tests/reproject_math.py: move_camera 'orbit')."""
    C = np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    a = np.deg2rad(degrees)
    R = np.array([[np.cos(a), 0, np.sin(a), 0], [0, 1, 0, 0], [-np.sin(a), 0, np.cos(a), 0], [0, 0, 0, 1]])
    return dict(params, c2w=np.ascontiguousarray((R @ C).T.reshape(16), np.float32))


def image(acc):
    return acc[..., :3] / np.maximum(acc[..., 3:], 1.0)


def rmse(img, gt):
    return float((((img - gt) ** 2) / (gt ** 2 + 1e-2)).mean())


def timed(d, fn):
    d.sync(); d.timer_begin()
    fn()
    return d.timer_end()


def setup(d, scene, params):
    d.set_variant(2); d.count_rays(False); d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear()
    d.track_moments(True)


def selection(d, scene, params):
    setup(d, scene, params)
    d.render_adaptive(params, seeds(0, 16), -1.0, 2)  # (both buffers filled: 16 samples in the accumulator and M, 8 in H)
    d.render_moments(params, seeds(16, 16))
    _, e_m, _ = device.adaptive_select_moments(d.read_moments(), -1.0, 4)
    _, e_h, _ = device.adaptive_select(d.read_accum(), d.read_adaptive_half(), -1.0, 4)
    thr = {"M": float(np.median(e_m)), "H": float(np.median(e_h))}
    call = {"M": lambda: d.render_adaptive_moments(params, [], thr["M"], 4), "H": lambda: d.render_adaptive(params, [], thr["H"], 4)}
    t = {"M": [], "H": []}
    for r in range(rounds + 1):
        for k in ("H", "M"):
            ms = timed(d, lambda: [call[k]() for _ in range(reps)]) / reps
            if r > 0:
                t[k].append(ms)
    share = {}
    for k in ("H", "M"):
        call[k]()
        a, n = d.adaptive_active_tiles()
        share[k] = a / n
    px = W * H
    say(f"selection at {W}x{H} ({(W + 7) // 8 * ((H + 7) // 8)} tiles), n_frames = 0: us per call (selection kernel + adaptive_compact_kernel), {reps} calls between the timer calls")
    say(f"  glrtx_render_adaptive          (adaptive_select_kernel: accumulator + H, {32 * px / 1e6:.1f} MB)   {spread(t['H'], 'us', 1e3)}   active {share['H']:.3f} at threshold {thr['H']:.4g}")
    say(f"  glrtx_render_adaptive_moments  (adaptive_moments::select_kernel: M, {16 * px / 1e6:.1f} MB)        {spread(t['M'], 'us', 1e3)}   active {share['M']:.3f} at threshold {thr['M']:.4g}")
    dm = np.median(t["H"]) - np.median(t["M"])
    say(f"  difference of the medians (the two selection kernels): {dm * 1e3:.1f} us; 16.6 MB less at the HBM figure {HBM / 1e12:.2f} TB/s would be {16 * px / HBM * 1e6:.1f} us")
    say()


def fold(d, scene, params):
    setup(d, scene, params)
    n = 16
    calls = [("render_adaptive_moments, threshold -1", lambda s: d.render_adaptive_moments(params, s, -1.0, 2)),
             ("glrtx_render_moments", lambda s: d.render_moments(params, s)),
             ("glrtx_render_adaptive, threshold -1", lambda s: d.render_adaptive(params, s, -1.0, 2))]
    t = {k: ([], [], []) for k, _ in calls}
    for r in range(rounds + 1):
        for k, fn in calls:
            s = seeds(1000 + 16 * r, n)
            st0 = d.stats()
            ms = timed(d, lambda: fn(s))
            st = d.stats()
            if r > 0:
                t[k][0].append(ms); t[k][1].append(st.accumulate_ms_total - st0.accumulate_ms_total); t[k][2].append(st.kernel_ms_total - st0.kernel_ms_total)
    say(f"{n} frames at {W}x{H} in one call: ms per call (timer around the call) | the render kernel | the accumulation pass")
    for k, _ in calls:
        say(f"  {k:<40s} {spread(t[k][0], 'ms', 1.0, 8, 3)} | {spread(t[k][2], 'ms', 1.0, 8, 3)} | {spread(t[k][1], 'ms', 1.0, 7, 3)}")
    say()


def scenario(d, w, h):
    scene, params = scenes.config_headline(w, h)
    cur = orbit(params, 3.0)
    setup(d, scene, params)
    for f0 in range(0, truth, 64):
        d.render_frames(cur, seeds(100_000 + f0, min(64, truth - f0)))
    gt = image(d.read_accum())
    paths = ("H form", "M form", "uniform")
    res = {k: dict(active=[], ms=[], raw=[], dn=[], spp=[]) for k in paths}
    before, thr_m = [], None
    for r in range(rounds + 1):
        for k in paths:
            d.clear()
            if k == "H form":
                d.render_adaptive(params, [], -1.0, 2)  # (H exists before the move, as in a loop that uses the H form)
            d.render_moments(params, seeds(0, 16))
            d.render_features(params)
            if thr_m is None:
                _, e, _ = device.adaptive_select_moments(d.read_moments(), -1.0, 4)
                thr_m = float(np.median(e))
            if k == "M form" and r == 1:
                d.render_adaptive_moments(params, [], thr_m, 4)
                a, n = d.adaptive_active_tiles()
                before.append(a / n)
            d.reproject(cur)
            s = seeds(16, 8)
            if k == "H form":
                ms = timed(d, lambda: d.render_adaptive(cur, s, thr_m, 4))
            elif k == "M form":
                ms = timed(d, lambda: d.render_adaptive_moments(cur, s, thr_m, 4))
            else:
                ms = timed(d, lambda: d.render_moments(cur, s))
            a, n = d.adaptive_active_tiles() if k != "uniform" else (1, 1)
            acc = d.read_accum()
            d.denoise_variance()
            if r > 0:
                q = res[k]
                q["active"].append(a / n); q["ms"].append(ms); q["raw"].append(rmse(image(acc), gt)); q["dn"].append(rmse(d.read_denoised()[..., :3], gt))
                q["spp"].append(float(acc[..., 3].mean()))
    say(f"scenario at {w}x{h}: 16 frames of render_moments, a 3-degree orbit through glrtx_reproject, 8 further frames; truth: {truth} frames of the new view")
    say(f"  M-form threshold {thr_m:.4g} (the median tile error before the move: active share there {before[0]:.3f}), min_samples 4; the H form is given the same number")
    say(f"  {'path':<10s} {'active after the move':>22s}   {'8 frames, ms (timer around the call)':<40s} {'rel. rMSE raw':>14s} {'after denoise_variance':>24s} {'mean count':>11s}")
    for k in paths:
        q = res[k]
        say(f"  {k:<10s} {np.median(q['active']):22.3f}   {spread(q['ms'], 'ms', 1.0, 8, 3):<40s} {np.median(q['raw']):14.5f} {np.median(q['dn']):24.5f} {np.median(q['spp']):11.2f}")
    say()


d = device.Device()
scene, params = scenes.config_headline(W, H)
if only in ("", "selection"):
    selection(d, scene, params)
if only in ("", "fold"):
    fold(d, scene, params)
if only in ("", "scenario"):
    scenario(d, W, H)
    scenario(d, 192, 108)
d.close()

if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
