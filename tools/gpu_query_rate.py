"""Ray-query throughput on the GPU box: glrtx_trace_rays_device (csrc/query.hip.h) in rays per second.

Per scene (headline = the C2 scene, c2, c5 = 100k random triangles; full size) and ray set:
  camera     coherent pinhole rays through the 1920x1080 pixel centres, from the scene's camera matrices (tmin 1e-4, tmax 1e8)
  incoherent cosine-distributed directions from random points on the surfaces (either side; 2 M rays)
  shadow     from those points to random points on the light triangles (tmax just short of the light; 2 M rays)
each in closest-hit and any-hit mode and in both node layouts (GLRTX_COMPACT_NODES=0 / 1).  Timing: device
events on the context's stream around --reps back-to-back device calls after --warmup calls; the median of --trials such timings.  Also: the share of
rays that hit.  Writes the table to profiles/r13_query_rate.txt (or --out) and prints it.

    python tools/gpu_query_rate.py [--scenes headline,c2,c5] [--reps 10] [--warmup 3] [--trials 3] [--out profiles/r13_query_rate.txt]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
import query_rays as qr  # noqa: E402
from glrt_amd import device, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


names = arg("--scenes", "headline,c2,c5").split(",")
reps, warmup, trials = int(arg("--reps", 10)), int(arg("--warmup", 3)), int(arg("--trials", 3))
n_inc = int(arg("--rays", 2_000_000))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r13_query_rate.txt"))

torch.cuda.init()
try:
    head = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short=12", "HEAD"], capture_output=True, text=True).stdout.strip() or "?"
except OSError:
    head = "?"
lines = [f"glrtx_trace_rays_device on one {torch.cuda.get_device_name(0)}; parent commit {head} plus this change; {reps} calls per timing after {warmup}, "
         f"median of {trials}", "",
         f"{'scene':9s} {'tris':>7s} {'rays':9s} {'mode':7s} {'layout':11s} {'n':>9s} {'ms/call':>9s} {'Grays/s':>8s} {'hit %':>6s}"]
print(lines[0], flush=True)
for name in names:
    sc, params = scenes.CONFIGS[name](width=1920, height=1080)
    n_tri = sc["tri"].shape[0]
    d = device.Device(0)
    d.upload_scene(sc)
    s = torch.cuda.Stream()
    d.set_stream(s.cuda_stream)
    sets = {"camera": qr.camera_rays(params), "incoherent": qr.incoherent_rays(sc, n_inc, seed=1), "shadow": qr.shadow_rays(sc, n_inc, seed=2)}
    os.environ.pop("GLRTX_COMPACT_NODES", None)
    for set_name, rays in sets.items():
        r = torch.from_numpy(rays).cuda()
        out = torch.empty((len(rays), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for any_hit in (False, True):
            results = {}
            for layout in ("64-byte", "compact"):
                os.environ["GLRTX_COMPACT_NODES"] = "1" if layout == "compact" else "0"
                with torch.cuda.stream(s):
                    for _ in range(warmup):
                        d.trace_rays(r, any_hit=any_hit, out=out)
                    ms = []
                    for _ in range(trials):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(s)
                        for _ in range(reps):
                            d.trace_rays(r, any_hit=any_hit, out=out)
                        e1.record(s)
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1) / reps)
                s.synchronize()
                hit = float((out[:, 1].view(torch.int32) >= 0).float().mean().item()) * 100.0
                results[layout] = (float(np.median(ms)), hit)
            os.environ.pop("GLRTX_COMPACT_NODES", None)
            for layout, (ms, hit) in results.items():
                line = (f"{name:9s} {n_tri:7d} {set_name:9s} {'any' if any_hit else 'closest':7s} {layout:11s} {len(rays):9d} {ms:9.3f} "
                        f"{len(rays) / ms / 1e6:8.2f} {hit:6.1f}")
                lines.append(line)
                print(line, flush=True)
    d.set_stream(0)
    d.close()
os.environ.pop("GLRTX_COMPACT_NODES", None)
text = "\n".join(lines) + "\n"
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write(text)
print(f"wrote {out_path}")
