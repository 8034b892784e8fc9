"""What material maps cost on the GPU box (csrc/maps.hip.h; include/glrtx.h "Material maps").  Config c2 at 1920 x 1080, depth 4, 1 spp on the textured
extension megakernel, four variants ALTERNATING inside one context (README "Measuring a change"): every repetition runs each variant once, in order, so drift
of the box lands on all of them alike.  Event timing (glrtx_timer_begin / _end) around --frames render calls after a warm-up round; ms a frame, median [min .. max].

    timeout -k 10 400 python tools/gpu_maps_time.py [--frames 8] [--reps 5] [--out profiles/r29_maps_time.txt] [--parent-isa parent_table.txt]

  albedo        every diffuse material bound to its own 1024 x 1024 sRGB albedo texture, no maps: the parent commit's kernel (pt_render_persistent_tex), the baseline
  flat          + a 2 x 2 flat RGBA32F normal map on every diffuse and conductor material: the MAPS kernel, the lookup, the flat-texel exit
  normal-1024   + a 1024 x 1024 non-flat RGBA32F normal map instead: the frame and the perturbation at every mapped hit
  normal+rough  + a 1024 x 1024 RGBA8 roughness map on the conductors as well
The coordinates are a planar map of the positions (s = 0.37 x + 0.11 z, t = 0.37 y + 0.23 z, repeat), as tools/gpu_texture_time.py's: c2's vertices carry none.
The file ends with tools/isa_report.py's table of this build and, with --parent-isa, the parent commit's table and the comparison of the kernels in both."""
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


frames, reps = int(arg("--frames", 8)), int(arg("--reps", 5))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r29_maps_time.txt"))
parent_isa = arg("--parent-isa", None)

W, H = 1920, 1080
torch.cuda.init()
d = device.Device(0)
scene, params = scenes.config_c2(W, H, max_depth=4, n_samples=1)
v = np.array(scene["vert"], np.float32).reshape(-1, 5, 3)
v[:, 2, 0] = np.float32(0.37) * v[:, 0, 0] + np.float32(0.11) * v[:, 0, 2]
v[:, 2, 1] = np.float32(0.37) * v[:, 0, 1] + np.float32(0.23) * v[:, 0, 2]
scene = dict(scene, vert=v.reshape(-1, 3))
d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H); d.set_variant(1); d.count_rays(False)
types = scene["mat"].reshape(-1, 18)[:, 0].astype(int)
diffuse, conductor = np.flatnonzero(types == 2), np.flatnonzero(types == 3)
rng = np.random.default_rng(29)
S = 1024
tex = [(rng.integers(0, 256, (S, S, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear") for _ in diffuse]
k_flat, k_bump, k_rough = len(tex), len(tex) + 1, len(tex) + 2
tex.append((np.tile(np.float32([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear"))
m = np.concatenate([rng.uniform(-0.5, 0.5, (S, S, 2)), np.ones((S, S, 1))], -1)
tex.append((((m / np.linalg.norm(m, axis=-1, keepdims=True) + 1.0) / 2.0).astype(np.float32), "rgba32f", "repeat", "bilinear"))
tex.append((rng.integers(10, 128, (S, S, 4), dtype=np.uint8), "rgba8_unorm", "repeat", "bilinear"))
bind = np.full(types.size, -1, np.int32)
bind[diffuse] = np.arange(len(diffuse))
d.upload_textures(tex, bind)
surfaces = np.isin(types, (2, 3))
VARIANTS = {
    "albedo": None,
    "flat": dict(normal=np.where(surfaces, k_flat, -1)),
    "normal-1024": dict(normal=np.where(surfaces, k_bump, -1)),
    "normal+rough": dict(normal=np.where(surfaces, k_bump, -1), roughness=np.where(types == 3, k_rough, -1)),
}


def burst(f0):
    d.timer_begin()
    for f in range(frames):
        d.render(dict(params, seed=host.frame_seed(f0 + f)))
    return d.timer_end() / frames


ms = {name: [] for name in VARIANTS}
for r in range(reps + 1):  # round 0 is the warm-up: code objects, buffers
    for name, maps in VARIANTS.items():
        d.bind_material_maps(**(maps or {}))
        d.clear()
        t = burst(frames * r)
        if r:
            ms[name].append(t)
d.close()

base = float(np.median(ms["albedo"]))
lines = [f"Material maps on one MI355X: config c2, {W} x {H}, depth 4, 1 spp, textured extension megakernel; {len(diffuse)} diffuse materials with a {S} x {S} sRGB albedo "
         f"texture each, {len(conductor)} conductor(s).",
         f"Four variants alternating inside one context: {frames} frames between one pair of events, {reps} repetitions after a warm-up round: median [min .. max] ms a frame.", ""]
for name, t in ms.items():
    med = float(np.median(t))
    lines.append(f"{name:14s} {med:8.3f} [{np.min(t):.3f} .. {np.max(t):.3f}] ms a frame   {med - base:+.3f} ms ({100.0 * (med - base) / base:+.1f} %) against albedo only")
print("\n".join(lines), flush=True)


def table(text):
    rows = {}
    for ln in text.splitlines():
        mt = re.match(r"(\S.*?)\s{2,}(\d+(?:\s+\d+)+)\s*$", ln)
        if mt:
            rows[mt.group(1)] = mt.group(2).split()
    return rows


this = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_report.py")], capture_output=True, text=True, timeout=300).stdout
lines += ["", "---- tools/isa_report.py, this commit", this.rstrip()]
if parent_isa:
    parent = open(parent_isa).read()
    lines += ["", "---- tools/isa_report.py, the parent commit", parent.rstrip(), ""]
    a, b = table(parent), table(this)
    # the two persistent kernels that gained the MAPS template flag are named <.., false> now: the same instantiations
    same_name = lambda k: re.sub(r"^(glrtx::pt_render_persistent_(?:tex|env)<\w+, \w+), false>$", r"\1>", k)
    bn = {same_name(k): row for k, row in b.items()}
    differ = [k for k in a if k in bn and bn[k] != a[k]]
    gone = [k for k in a if k not in bn]
    new = [k for k in b if same_name(k) not in a]
    lines.append(f"---- comparison: {len(a)} kernels in the parent, {len(b)} in this commit; {len(a) - len(gone)} in both (pt_render_persistent_tex / _env<a, b> are <a, b, false> now)")
    lines.append(f"kernels in both whose vgpr / agpr / sgpr / spill / scratch / lds figures differ: {len(differ)}{'' if not differ else ': ' + ', '.join(differ)}")
    lines.append(f"kernels gone: {len(gone)}{'' if not gone else ': ' + ', '.join(gone)}")
    lines.append("new kernels (vgpr agpr sgpr vspill sspill scratch lds):")
    lines += [f"  {k:60s} {' '.join(b[k])}" for k in new]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
