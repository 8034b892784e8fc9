"""Bloom on the GPU box: device time of one glrtx_bloom at 1080p, in one context, on the headline scene and the 64^3 fire scene.

Every figure is a burst's: 20 calls back to back between one pair of HIP events after a warm-up pass, per call (glrtx_debug_bloom_burst: one call is 2 * levels
launches; glrtx_debug_tonemap_burst for the plain resolve and the fused tone-mapping resolve beside it; glrtx_denoise between the context's timer calls).  The
passes alternate within the run, --rounds times; the median and the range are printed.  The bloom's compulsory bytes are set against the HBM figure the project
uses (6.29 TB/s, the measured float4-copy rate): the source read twice and B written, 16 B a pixel each, plus the pyramid written once and read and rewritten
along the up chain, 3 x 16 B a texel.

    python tools/gpu_bloom_time.py [--out profiles/r20_bloom_time.txt] [--reps 20] [--rounds 5] [--frames 4] [--levels 5]"""
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


out_path, reps, rounds, frames = arg("--out", ""), int(arg("--reps", 20)), int(arg("--rounds", 5)), int(arg("--frames", 4))
levels = int(arg("--levels", 5))
W, H = 1920, 1080
PX = W * H
lines = [f"bloom at {W}x{H}: us per call, {reps} calls between one pair of events after a warm-up pass; median [min .. max] of {rounds} rounds;",
         f"compulsory bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]


def bloom_bytes(n):
    return 16 * (3 * PX + 3 * host.bloom_texels(W, H, n))


def row(name, ms, nbytes=None):
    us = np.array(ms) * 1e3
    med = float(np.median(us))
    tail = "" if nbytes is None else f"   {nbytes / 1e6:6.1f} MB   {nbytes / (med * 1e-6) / HBM * 100:5.1f} % of the HBM figure"
    lines.append(f"  {name:<52s} {med:8.1f} us  [{us.min():7.1f} .. {us.max():7.1f}]{tail}")
    print(lines[-1], flush=True)


def denoise_ms(d):
    d.timer_begin()
    for _ in range(reps):
        d.denoise()
    return d.timer_end() / reps


def time_scene(d, name, params, with_denoiser):
    lines.append(name)
    print(name, flush=True)
    if with_denoiser:
        d.render_features(params)
        d.denoise()
    d.bloom(levels=levels); d.sync()  # (allocations and first launches outside the timed rounds)
    t = {k: [] for k in ("plain", "fused", "bloom", "bloom1", "bloom8", "bloomD", "denoise")}
    for _ in range(rounds):
        t["plain"].append(d.tonemap_burst_ms(0, reps))
        t["fused"].append(d.tonemap_burst_ms(1, reps, op=2))
        t["bloom"].append(d.bloom_burst_ms(reps, levels=levels))
        t["bloom1"].append(d.bloom_burst_ms(reps, levels=1))
        t["bloom8"].append(d.bloom_burst_ms(reps, levels=8))
        if with_denoiser:
            t["bloomD"].append(d.bloom_burst_ms(reps, levels=levels, source=1))
            t["denoise"].append(denoise_ms(d))
    row("resolve_kernel<2> (the plain resolve)", t["plain"], 20 * PX)
    row("tonemap_resolve<2> op 2 (the fused resolve)", t["fused"], 20 * PX)
    row(f"glrtx_bloom, {levels} levels ({2 * levels} launches)", t["bloom"], bloom_bytes(levels))
    if with_denoiser:
        row(f"glrtx_bloom, {levels} levels, from D", t["bloomD"], bloom_bytes(levels))
    row("glrtx_bloom, 1 level (2 launches)", t["bloom1"], bloom_bytes(1))
    row("glrtx_bloom, 8 levels (16 launches)", t["bloom8"], bloom_bytes(8))
    if with_denoiser:
        row("glrtx_denoise, 5 iterations (timer around the calls)", t["denoise"])
    d.bloom(levels=levels)
    B, acc = d.read_bloomed(), d.read_accum()
    with np.errstate(all="ignore"):
        x = np.clip(np.nan_to_num(acc[..., :3] / acc[..., 3:4], nan=0.0, posinf=65504.0, neginf=0.0), 0, 65504)
    lines.append(f"  (B of a last call at the defaults: finite {bool(np.isfinite(B).all())}, {int((B[..., :3] > x).any(-1).sum())} of {PX} pixels carry glow, mean glow {float((B[..., :3] - x).mean()):.4g})")
    lines.append("")


d = device.Device()
d.set_variant(2)
scene, params = scenes.config_headline(W, H)
d.upload_scene(scene); d.resize(W, H)
d.render_frames(params, [host.frame_seed(i) for i in range(frames)]); d.sync()
time_scene(d, f"headline, {frames} frames", params, True)

scene, params, vol = scenes.config_fire(W, H, grid=64)
d.upload_scene(scene); d.upload_volume(vol["density"], vol["temperature"], vol["bbox_min"], vol["bbox_max"]); d.set_extensions(device.EXT_VOLUME)
d.resize(W, H)
d.render_frames(params, [host.frame_seed(i) for i in range(frames)]); d.sync()
time_scene(d, f"fire 64^3, {frames} frames", params, False)
d.close()

if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
