"""What moving geometry costs on the GPU box: glrtx_update_vertices (the device refit, csrc/refit.hip.h) against what the same change costs with a rebuild.

Per scene (headline, c5 = 100k random triangles, c3 = the 10 000-level chain):
  refit device ms      glrtx_timer_begin / _end around glrtx_update_vertices_device (a torch tensor already on the GPU): the refit's three kernels and the
                       7-word read-back, median and range of --reps calls
  update wall ms       the host-memory call (glrtx_update_vertices: copy in + refit + read-back) and the device-memory call, host clock, median
  rebuild wall ms      the CPU SAH build (host.build_bvh + lights_first, as scenes.SceneBuilder does) + glrtx_upload_scene; glrtx_build_bvh_sah + glrtx_upload_scene
  cadence ms/frame     at 1080p, 1 spp: --frames iterations of update (host memory) + glrtx_render with no sync in the loop, against the same loop without the update
Writes the table to profiles/r12_refit_time.txt (or --out) and prints it.

    python tools/gpu_refit_time.py [--scenes headline,c5,c3] [--reps 50] [--frames 30] [--out profiles/r12_refit_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


names = arg("--scenes", "headline,c5,c3").split(",")
reps, frames = int(arg("--reps", 50)), int(arg("--frames", 30))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r12_refit_time.txt"))


def moved(v, k):
    w = v.copy()
    w[:, :3] += np.float32(0.001 * (k + 1))
    return w


def med(xs):
    return f"{np.median(xs):8.3f} [{np.min(xs):.3f} .. {np.max(xs):.3f}]"


torch.cuda.init()
lines = [f"glrtx_update_vertices on one MI355X; reps {reps}, cadence over {frames} frames at 1920x1080, 1 spp", ""]
for name in names:
    sc, params = scenes.CONFIGS[name](width=1920, height=1080)
    v0 = sc["vert"].reshape(-1, 15).copy()
    n_tri = sc["tri"].shape[0]
    d = device.Device(0)
    d.upload_scene(sc)
    d.set_partition(0, 1, 16)
    d.resize(params["width"], params["height"])
    tv = [torch.from_numpy(moved(v0, k)).cuda() for k in range(2)]
    torch.cuda.synchronize()
    for k in range(5):
        d.update_vertices(tv[k & 1])
    dev_ms, wall_dev, wall_host = [], [], []
    for k in range(reps):
        d.timer_begin()
        d.update_vertices(tv[k & 1])
        dev_ms.append(d.timer_end())
    for k in range(reps):
        t0 = time.perf_counter(); d.update_vertices(tv[k & 1]); wall_dev.append(1e3 * (time.perf_counter() - t0))
    hv = [moved(v0, k) for k in range(2)]
    for k in range(reps):
        t0 = time.perf_counter(); d.update_vertices(hv[k & 1]); wall_host.append(1e3 * (time.perf_counter() - t0))
    # the same change by rebuilding: CPU SAH + upload, device SAH + upload (a few repetitions: these are slow)
    cpu_ms, gpu_ms = [], []
    kind = sc.get("bvh_kind", "sah")
    for k in range(3):
        v = hv[k & 1]
        t0 = time.perf_counter()
        built, _ = host.build_bvh(v, sc["tri"], kind)
        nodes = host.lights_first(built, sc["tri"], sc["mat"])[0] if kind not in ("chain", "reference") else built
        d.upload_scene(dict(sc, vert=v.reshape(-1, 3), bvh=nodes))
        cpu_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        nodes, _, _ = d.build_bvh_sah(v, sc["tri"])
        d.upload_scene(dict(sc, vert=v.reshape(-1, 3), bvh=nodes))
        gpu_ms.append(1e3 * (time.perf_counter() - t0))
    d.upload_scene(sc)
    # cadence: update + render per frame, no sync inside the loop; the same loop without the update
    seeds = [host.frame_seed(i) for i in range(frames)]
    cad = {}
    for mode in ("render only", "update + render", "render only", "update + render"):
        d.clear(); d.sync()
        t0 = time.perf_counter()
        for i, sd in enumerate(seeds):
            if mode != "render only":
                d.update_vertices(hv[i & 1])
            d.render(dict(params, seed=sd))
        d.sync()
        cad.setdefault(mode, []).append(1e3 * (time.perf_counter() - t0) / frames)
    lines += [f"{name}: {n_tri} triangles, tree '{kind}'",
              f"  refit, device time (ms)           {med(dev_ms)}",
              f"  update, device vertices, wall     {med(wall_dev)}",
              f"  update, host vertices, wall       {med(wall_host)}",
              f"  CPU {kind} build + upload, wall    {med(cpu_ms)}",
              f"  device SAH build + upload, wall   {med(gpu_ms)}",
              f"  cadence render only (ms/frame)    {med(cad['render only'])}",
              f"  cadence update + render           {med(cad['update + render'])}", ""]
    print("\n".join(lines[-9:]), flush=True)
    d.close()
    del tv
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
