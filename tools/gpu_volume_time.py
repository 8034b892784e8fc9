"""Volume branch (GLRTX_EXT_VOLUME) timing on the GPU box: the 1080p fire scene (scenes.config_fire: a 64^3 fire blob in a media box over a
floor, a lamp above, 8 bounces, 1 sample per pixel per frame) rendered by the persistent megakernel's volume instantiation.  Reports ms per
frame (render kernel, HIP events; and wall time) and Mrays/s (rays = executions of intersect(), every Woodcock trial ray included, from a counting pass;
the timed frames run the non-counting instantiation), and the same scene with the switch off for comparison.  One JSON line per setting.

    python tools/gpu_volume_time.py [--frames K] [--warmup W] [--size 1920x1080]"""
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


frames, warmup = int(arg("--frames", 20)), int(arg("--warmup", 3))
w, h = (int(v) for v in arg("--size", "1920x1080").split("x"))
scene, params, vol = scenes.config_fire(w, h, max_depth=8, n_samples=1, grid=64)
d = device.Device()
d.upload_scene(scene)
d.upload_volume(vol["density"], vol["temperature"], vol["bbox_min"], vol["bbox_max"])
d.resize(w, h)
for flags, label in ((device.EXT_VOLUME, "volume"), (0, "switch off")):
    d.set_extensions(flags)
    # rays of one frame (counting instantiation), then the timed frames (the instantiation without counters)
    d.clear(); d.reset_stats(); d.count_rays(True)
    d.render(dict(params, seed=host.frame_seed(0))); d.sync()
    rays = int(d.stats().rays)
    d.count_rays(False)
    for f in range(warmup):
        d.render(dict(params, seed=host.frame_seed(1 + f)))
    d.sync(); d.reset_stats()
    t0 = time.perf_counter()
    for f in range(frames):
        d.render(dict(params, seed=host.frame_seed(1 + warmup + f)))
    d.sync()
    wall = (time.perf_counter() - t0) * 1e3 / frames
    st = d.stats()
    ms = st.kernel_ms_total / max(1, int(st.launches))  # (render kernel time per FRAME: a fed launch of the switch-off path covers several)
    acc = d.read_accum()
    out = dict(scene="fire", setting=label, width=w, height=h, depth=8, grid=64, frames=frames, kernel_ms_per_frame=round(ms, 3), wall_ms_per_frame=round(wall, 3),
               rays_per_frame=rays, mrays_per_s=round(rays / ms / 1e3, 1), variant=int(st.variant_last),
               mean_rgb=[round(float(v), 4) for v in (acc[..., :3] / np.maximum(acc[..., 3:], 1)).mean(axis=(0, 1))])
    print(json.dumps(out), flush=True)
d.set_extensions(0)
d.close()
