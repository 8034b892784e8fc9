"""What textured albedo costs on the GPU box (csrc/texture.hip.h; include/glrtx.h "Textures"), and what it costs the extension kernel's other users.
Event timing (glrtx_timer_begin / _end: HIP events on the context's stream) around --frames render calls, a warm-up burst, then --reps repetitions; ms a frame,
median [min .. max].  One configuration a process, each under its own time limit:

    timeout -k 10 240 python tools/gpu_texture_time.py --config c2-mega
    timeout -k 10 240 python tools/gpu_texture_time.py --config c2-tex-1 --append
    ...                                                [--frames 8] [--reps 3] [--lib other/libglrtx.so] [--label parent] [--out profiles/r27_texture_time.txt]

  c2-mega       config c2 (1920 x 1080, depth 4, 1 spp) untextured on the persistent megakernel (glrtx_set_variant(1)): the kernel family textures run in
  c2-wavefront  the same on the default wavefront kernel, for scale
  c2-tex-1      every diffuse material bound to its own 1 x 1 bilinear RGBA8 sRGB texture: the textured kernel's code with no spread of addresses
  c2-tex-1024   ... to its own 1024 x 1024 texture (7 x 4 MiB)
  c2-tex-4096   ... to ONE 4096 x 4096 texture (64 MiB, well past one XCD's 4 MiB L2) shared by the seven materials
                The coordinates are a planar map of the positions (s = 0.37 x + 0.11 z, t = 0.37 y + 0.23 z, repeat): c2's own vertices carry none.
  spheres-glass config_spheres(glass=True) at 1920 x 1080, depth 8: three analytic spheres and GLRTX_EXT_DIELECTRIC on the extension megakernel
  fire          config_fire at 1920 x 1080, depth 8, a 64^3 grid: GLRTX_EXT_VOLUME on the megakernel's volume instantiation
--lib loads another build of libglrtx.so (the parent commit's, for the two extension configurations) and --label names it in the table."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


config = arg("--config", "c2-mega")
frames, reps = int(arg("--frames", 8)), int(arg("--reps", 3))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r27_texture_time.txt"))
label = arg("--label", "this commit")
if "--lib" in sys.argv:
    import pathlib
    other = pathlib.Path(arg("--lib", "")).resolve()
    device.lib_path = lambda: other

W, H = 1920, 1080
torch.cuda.init()
d = device.Device(0)
note = ""
if config.startswith("c2"):
    scene, params = scenes.config_c2(W, H, max_depth=4, n_samples=1)
    v = np.array(scene["vert"], np.float32).reshape(-1, 5, 3)
    v[:, 2, 0] = np.float32(0.37) * v[:, 0, 0] + np.float32(0.11) * v[:, 0, 2]
    v[:, 2, 1] = np.float32(0.37) * v[:, 0, 1] + np.float32(0.23) * v[:, 0, 2]
    scene = dict(scene, vert=v.reshape(-1, 3))
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H)
    d.set_variant(2 if config == "c2-wavefront" else 1)
    if config.startswith("c2-tex"):
        size = int(config.split("-")[2])
        types = scene["mat"].reshape(-1, 18)[:, 0].astype(int)
        diffuse = np.flatnonzero(types == 2)
        rng = np.random.default_rng(size)
        n_tex = 1 if size >= 4096 else len(diffuse)
        tex = [(rng.integers(0, 256, (size, size, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear") for _ in range(n_tex)]
        bind = np.full(types.size, -1, np.int32)
        bind[diffuse] = np.arange(len(diffuse)) % n_tex
        d.upload_textures(tex, bind)
        note = f"{len(diffuse)} diffuse materials over {n_tex} texture(s) of {size} x {size}, {n_tex * size * size * 4 / 2 ** 20:.3g} MiB of texels"
elif config == "spheres-glass":
    scene, params, spheres = scenes.config_spheres(W, H, max_depth=8, n_samples=1, glass=True)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H)
    d.upload_spheres(spheres); d.set_extensions(device.EXT_DIELECTRIC)
elif config == "fire":
    scene, params, vol = scenes.config_fire(W, H, max_depth=8, n_samples=1, grid=64)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H)
    d.upload_volume(vol["density"], vol["temperature"], vol["bbox_min"], vol["bbox_max"]); d.set_extensions(device.EXT_VOLUME)
else:
    raise SystemExit(f"unknown --config {config}")
d.count_rays(False)


def burst(f0):
    d.timer_begin()
    for f in range(frames):
        d.render(dict(params, seed=host.frame_seed(f0 + f)))
    return d.timer_end() / frames


d.clear()
burst(0)  # warm-up: code objects, buffers
ms = [burst(frames * (r + 1)) for r in range(reps)]
st = d.stats()
kernel = {1: "persistent megakernel", 2: "wavefront kernel"}.get(st.variant_last, str(st.variant_last))
line = f"{config:14s} {label:12s} {np.median(ms):8.3f} [{np.min(ms):.3f} .. {np.max(ms):.3f}] ms a frame   ({kernel}{'; ' + note if note else ''})"
print(line, flush=True)
d.close()
head = [f"Textured albedo on one MI355X: {W} x {H}, 1 spp, {frames} frames between one pair of events after a warm-up burst, {reps} repetitions: median [min .. max]", ""]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
new = "--append" not in sys.argv or not os.path.exists(out_path)
with open(out_path, "w" if new else "a") as f:
    f.write("\n".join((head if new else []) + [line]) + "\n")
print(f"wrote {out_path}")
