"""What environment lighting costs on the GPU box (csrc/environment.hip.h; include/glrtx.h "Environment").  One process, one context a variant, config c2
(1920 x 1080, depth 4, 1 spp).  Event timing (glrtx_timer_begin / _end: HIP events on the context's stream) around --frames render calls, a warm-up burst,
then --reps repetitions; ms a frame, median [min .. max].

    timeout -k 10 400 python tools/gpu_env_time.py [--frames 8] [--reps 3] [--out profiles/r28_environment_time.txt]
    timeout -k 10 200 python tools/gpu_env_time.py --weights-only      # one table build of the 2048^2 map and nothing else, for a kernel trace of env_weights_kernel

  mega           the extension megakernel without a map (GLRTX_EXT_DIELECTRIC set; c2 has no dielectric material): the parent commit's kernel, the yardstick
  escape-2       escape mode, a 2 x 2 map (the smallest an octahedral map can be): the environment kernel's code with no spread of addresses
  escape-2048    escape mode, a 2048 x 2048 RGBA32F map (64 MiB, well past one XCD's 4 MiB L2)
  sampled-64     sampled mode, the 2048^2 map, G = 64, light_pick 0.5
  sampled-256    sampled mode, the 2048^2 map, G = 256, light_pick 0.5
  tables         wall-clock time of one glrtx_set_environment_cfg that rebuilds the tables of the 2048^2 map (weights kernel, read-back, Vose's method on the
                 host, five uploads), G = 256; the weights kernel alone is in the kernel trace of --weights-only
Registers and scratch of the new kernels: tools/isa_report.py."""
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


frames, reps = int(arg("--frames", 8)), int(arg("--reps", 3))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r28_environment_time.txt"))
W, H = 1920, 1080
torch.cuda.init()
scene, params = scenes.config_c2(W, H, max_depth=4, n_samples=1)


def sky(n):
    """A sky with a sun: a smooth gradient and a small bright disc in the upper half, RGBA32F."""
    c = (np.arange(n, dtype=np.float32) + 0.5) / n
    s, t = np.meshgrid(c, c)
    a = np.empty((n, n, 4), np.float32)
    a[..., 0], a[..., 1], a[..., 2], a[..., 3] = 0.4 + 0.3 * s, 0.5 + 0.3 * t, 0.9, 1.0
    a[(s - 0.6) ** 2 + (t - 0.55) ** 2 < 0.01 ** 2, :3] = 2000.0
    return (a, "rgba32f", "bilinear")


big = sky(2048)
if "--weights-only" in sys.argv:
    d = device.Device(0)
    d.upload_scene(scene)
    d.upload_environment(big, host.env_cfg("sampled", grid=256))
    d.sync(); d.close()
    print("one table build of a 2048 x 2048 RGBA32F map, G = 256")
    raise SystemExit(0)

VARIANTS = [("mega", None, None), ("escape-2", sky(2), host.env_cfg("escape")), ("escape-2048", big, host.env_cfg("escape")),
            ("sampled-64", big, host.env_cfg("sampled", grid=64, light_pick=0.5)), ("sampled-256", big, host.env_cfg("sampled", grid=256, light_pick=0.5))]
lines = []
for name, env_map, cfg in VARIANTS:
    d = device.Device(0)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H); d.set_variant(2); d.count_rays(False)
    if env_map is None:
        d.set_extensions(device.EXT_DIELECTRIC)
    else:
        d.upload_environment(env_map, cfg)

    def burst(f0):
        d.timer_begin()
        for f in range(frames):
            d.render(dict(params, seed=host.frame_seed(f0 + f)))
        return d.timer_end() / frames

    d.clear()
    burst(0)  # warm-up: code objects, buffers
    ms = [burst(frames * (r + 1)) for r in range(reps)]
    st = d.stats()
    assert st.variant_last == 1
    extra = ""
    if name == "sampled-256":
        t0 = time.perf_counter()
        d.set_environment_cfg(host.env_cfg("sampled", grid=256, light_pick=0.5, scale=0.5))
        extra = f"; tables rebuilt (weights kernel + read-back + host alias + uploads) in {(time.perf_counter() - t0) * 1e3:.1f} ms wall clock"
    lines.append(f"{name:12s} {np.median(ms):8.3f} [{np.min(ms):.3f} .. {np.max(ms):.3f}] ms a frame{extra}")
    print(lines[-1], flush=True)
    d.close()
head = [f"Environment lighting on one MI355X: config c2, {W} x {H}, depth 4, 1 spp, on the extension megakernel; {frames} frames between one pair of events after a "
        f"warm-up burst, {reps} repetitions: median [min .. max].  One process, one context a variant.", ""]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(head + lines) + "\n")
print(f"wrote {out_path}")
