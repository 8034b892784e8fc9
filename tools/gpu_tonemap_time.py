"""Tone mapping on the GPU box: device time of the passes at 1080p, in one context, on the headline scene, the 64^3 fire scene and a flat image.

Every figure is glrtx_debug_tonemap_burst's: 20 launches back to back between one pair of HIP events after a warm-up pass, per launch.  The fused resolve
(tonemap_resolve, per op) and the plain resolve kernel (resolve_kernel on the same source) alternate within the run, --rounds times; the median and the range
are printed.  The measurement (exposure_histogram + exposure_reduce) is timed on the headline, the fire scene and an image of one flat colour -- the case that
puts every lane of a wave on one LDS counter.  Each pass's compulsory bytes are set against the HBM figure the project uses (6.29 TB/s, the measured float4-copy
rate): resolve 16 B in + 4 B out a pixel, the plane 16 + 16, the measurement 16 in.

    python tools/gpu_tonemap_time.py [--out profiles/r19_tonemap_time.txt] [--reps 20] [--rounds 5] [--frames 4]"""
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
W, H = 1920, 1080
PX = W * H
BYTES = {0: 20 * PX, 1: 20 * PX, 2: 32 * PX, 3: 16 * PX}
lines = [f"tone mapping at {W}x{H}: us per launch, {reps} launches between one pair of events after a warm-up pass; median [min .. max] of {rounds} rounds;",
         f"compulsory bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]


def row(name, which, ms):
    us = np.array(ms) * 1e3
    med = float(np.median(us))
    lines.append(f"  {name:<44s} {med:7.1f} us  [{us.min():6.1f} .. {us.max():6.1f}]   {BYTES[which] / 1e6:5.1f} MB   {BYTES[which] / (med * 1e-6) / HBM * 100:5.1f} % of the HBM figure")
    print(lines[-1], flush=True)


def time_scene(d, name, measure_only=False):
    lines.append(f"{name}")
    print(name, flush=True)
    if not measure_only:
        t = {k: [] for k in ("plain", 0, 1, 2)}
        for _ in range(rounds):  # alternate the plain resolve and the fused kernels within the run
            t["plain"].append(d.tonemap_burst_ms(0, reps))
            for op in (0, 1, 2):
                t[op].append(d.tonemap_burst_ms(1, reps, op=op, auto_exposure=1, exposure=1.3))
        row("resolve_kernel<2> (the parent's, beside it)", 0, t["plain"])
        for op, nm in ((0, "clamp"), (1, "reinhard"), (2, "aces")):
            row(f"tonemap_resolve<2> op {op} ({nm})", 1, t[op])
        row("tonemap_plane op 2", 2, [d.tonemap_burst_ms(2, reps, op=2, auto_exposure=1) for _ in range(rounds)])
    row("exposure_histogram + exposure_reduce", 3, [d.tonemap_burst_ms(3, reps) for _ in range(rounds)])
    e = d.read_exposure()
    lines.append(f"  (histogram: {int(e.counted)} counted, {int(np.count_nonzero(np.ctypeslib.as_array(e.hist)))} bins occupied, mean log2 {e.mean_log2:.3f})")
    lines.append("")


d = device.Device()
d.set_variant(2)
scene, params = scenes.config_headline(W, H)
d.upload_scene(scene); d.resize(W, H)
d.render_frames(params, [host.frame_seed(i) for i in range(frames)]); d.sync()
time_scene(d, f"headline, {frames} frames")

# one flat colour through the accumulator the context is bound to: a torch tensor of the accumulator's pitch
flat = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
flat[...] = torch.tensor([0.9, 0.6, 0.3, 2.0], device="cuda")
torch.cuda.synchronize()
d.bind_accum(flat.data_ptr(), W * 16, H)
time_scene(d, "one flat colour (every lane of a wave on one LDS counter)", measure_only=True)
d.bind_accum(None, 0, 0)

scene, params, vol = scenes.config_fire(W, H, grid=64)
d.upload_scene(scene); d.upload_volume(vol["density"], vol["temperature"], vol["bbox_min"], vol["bbox_max"]); d.set_extensions(device.EXT_VOLUME)
d.resize(W, H)
d.render_frames(params, [host.frame_seed(i) for i in range(frames)]); d.sync()
time_scene(d, f"fire 64^3, {frames} frames")
d.close()

if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
