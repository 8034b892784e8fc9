"""Firefly re-weighting on the GPU box: device time of the cascade fold and of the resolve at 1080p on the headline scene, in one process and one context.

The fold: glrtx_render_cascades of --frames frames beside glrtx_render_moments of the same frames, alternating, each call between the context's timer calls
(HIP events); the two accumulation kernels by themselves from glrtx_stats.accumulate_ms_total (the events around the pass).  Per pixel the cascade pass moves
16 B a frame + 32 B for the accumulator + 6 x 32 B for the cascades, the moments pass 16 B a frame + 64 B; the yardstick is 1.5 x the moments pass's time in
the same run, and a tenth over that is allowed for the per-sample quotient.
The resolve: glrtx_debug_reweight_burst (--reps launches between one pair of events after a warm-up pass) against the HBM figure the project uses (6.29 TB/s,
the measured float4-copy rate) for its compulsory 112 B a pixel; in the same run the fused tone-mapping resolve and the five-iteration glrtx_denoise_variance.
Every figure is the median of --rounds rounds after a warm-up round; the range is printed beside it.

    python tools/gpu_reweight_time.py [--out profiles/r22_reweight_time.txt] [--frames 16] [--reps 20] [--rounds 3]"""
import os
import sys

import numpy as np
import torch  # (before libglrtx is loaded: torch brings its own copy of the HIP runtime and wants to initialise first)

torch.cuda.init()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
from glrt_amd import device, host, scenes  # noqa: E402

HBM = 6.29e12  # bytes / s: the measured float4-copy rate


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


out_path, frames, reps, rounds = arg("--out", ""), int(arg("--frames", 16)), int(arg("--reps", 20)), int(arg("--rounds", 3))
W, H = 1920, 1080
PX = W * H
lines = [f"firefly re-weighting at {W}x{H}, headline scene, one context; median [min .. max] of {rounds} rounds after a warm-up round;",
         f"bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]


def row(name, ms, nbytes=None, note=""):
    us = np.array(ms) * 1e3
    med = float(np.median(us))
    tail = "" if nbytes is None else f"   {nbytes / 1e6:6.1f} MB   {nbytes / (med * 1e-6) / HBM * 100:5.1f} % of the HBM figure"
    lines.append(f"  {name:<58s} {med:9.1f} us  [{us.min():9.1f} .. {us.max():9.1f}]{tail}{note}")
    print(lines[-1], flush=True)
    return med


d = device.Device()
d.set_variant(2)
scene, params = scenes.config_headline(W, H)
d.upload_scene(scene); d.resize(W, H)
d.track_moments(True); d.track_cascades(True)
seeds = [host.frame_seed(i) for i in range(frames)]


def timed(call):
    """(ms of the whole call between the timer's events, ms of its accumulation passes)"""
    st0 = d.stats()
    d.timer_begin()
    call(params, seeds)
    ms = d.timer_end()
    st = d.stats()
    return ms, st.accumulate_ms_total - st0.accumulate_ms_total


t = {k: [] for k in ("casc", "casc_pass", "mom", "mom_pass")}
for r in range(rounds + 1):
    for key, call in (("mom", d.render_moments), ("casc", d.render_cascades)):
        ms, pass_ms = timed(call)
        if r > 0:
            t[key].append(ms); t[key + "_pass"].append(pass_ms)
lines.append(f"the fold: {frames} frames a call, 1 sample a frame")
mom_bytes, casc_bytes = PX * (16 * frames + 64), PX * (16 * frames + 32 + 6 * 32)
row(f"glrtx_render_moments, {frames} frames (whole call)", t["mom"])
row(f"glrtx_render_cascades, {frames} frames (whole call)", t["casc"])
m = row("accumulate_moments_kernel (the passes of one call)", t["mom_pass"], mom_bytes)
c = row("accumulate_cascades_kernel (the passes of one call)", t["casc_pass"], casc_bytes)
lines.append(f"  cascade pass / moments pass = {c / m:.3f}   (bytes: {casc_bytes / mom_bytes:.3f}; the yardstick 1.5, a tenth over it allowed: 1.65)")
print(lines[-1], flush=True)
lines.append("")

lines.append(f"the resolve and its neighbours ({reps} launches or calls between one pair of events)")
d.render_features(params)
d.reweight(); d.denoise_variance(); d.sync()  # (allocations and first launches outside the timed rounds)


def denoise_var_ms():
    d.timer_begin()
    for _ in range(reps):
        d.denoise_variance()
    return d.timer_end() / reps


t = {k: [] for k in ("rw", "fused", "plain", "var")}
for r in range(rounds + 1):
    got = dict(plain=d.tonemap_burst_ms(0, reps), fused=d.tonemap_burst_ms(1, reps, op=2), rw=d.reweight_burst_ms(reps), var=denoise_var_ms())
    if r > 0:
        for k, v in got.items():
            t[k].append(v)
row("resolve_kernel<2> (the plain resolve)", t["plain"], 20 * PX)
row("tonemap_resolve<2> op 2 (the fused tone-mapping resolve)", t["fused"], 20 * PX)
row("reweight_kernel (compulsory 6 x 16 B in, 16 B out)", t["rw"], 112 * PX)
row("glrtx_denoise_variance, 5 iterations (timer around calls)", t["var"])
d.reweight()
D, C = d.read_denoised(), d.read_cascades()
lum = lambda x: 0.2126 * x[..., 0].astype(np.float64) + 0.7152 * x[..., 1] + 0.0722 * x[..., 2]  # noqa: E731
folded = frames * (rounds + 1)  # (render_cascades' frames; render_moments' frames went into the accumulator as well: D is not compared with its mean)
mean_c = C[..., :3].sum(0) / C[..., 3:4].sum(0)
lines.append(f"  (D of a last call at the defaults, {folded} samples a pixel in C: finite {bool(np.isfinite(D).all())}, sum_k C_k.w == {folded} {bool((C[..., 3].sum(0) == folded).all())}, "
             f"{int((D[..., :3] < mean_c * (1 - 1e-5)).any(-1).sum())} of {PX} pixels below the cascades' own mean, sum lum(D) / sum lum(that mean) {lum(D).sum() / lum(mean_c).sum():.4f})")
print(lines[-1], flush=True)
d.close()

if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
