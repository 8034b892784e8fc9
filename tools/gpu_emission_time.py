"""What emission maps cost on the GPU box (csrc/texture.hip.h: emit_light_st, emit_radiance; csrc/pt_kernel.hip.h: shade_core<.., EMIT>; include/glrtx.h "Emission
maps").  Config c2 at 1920 x 1080, depth 4, 1 spp on the textured extension megakernel, four cases ALTERNATING inside one process and one context (README
"Measuring a change"): every repetition runs each case once, in order, so drift of the box lands on all of them alike.  Event timing (glrtx_timer_begin /
_end) around --frames render calls after a warm-up round; ms a frame, median of --reps bursts [min .. max].

    timeout -k 10 400 python tools/gpu_emission_time.py [--frames 8] [--reps 3] [--out profiles/r32_emission_time.txt] [--parent-lib path/to/parent/libglrtx.so]

  (a) textured       every diffuse material bound to its own 1024 x 1024 sRGB albedo texture, no emission maps: the parent commit's kernel, the baseline
  (b) unused         + an emission map bound to an emitter material no triangle uses: the EMIT kernel, its per-hit and per-light-sample mat_emit gathers, and
                     nothing behind them
  (c) lamp-1x1       + every emitter material bound to a 1 x 1 RGBA32F map of ones: a lookup wherever the lamp is seen and at every contributing light
                     sample, all on one texel -- the image of (a)
  (d) lamp-1024      + a 1024 x 1024 RGBA8 sRGB bilinear map instead: four texel gathers a lookup, spread over the map -- another image
The coordinates are a planar map of the positions (s = 0.37 x + 0.11 z, t = 0.37 y + 0.23 z, repeat), as tools/gpu_maps_time.py's: c2's vertices carry none.

With --parent-lib, case (a) is also measured against a build of the parent commit, as tools/gpu_ab_inproc.py measures builds: three contexts in this process --
the parent's library twice and this commit's once --, the same textured scene in each, bursts going round the three in rotating order.  The two parent contexts
show the spread one binary has between contexts in this very run; this commit's kernels for case (a) are the parent's instruction for instruction
(tools/isa_diff.py), so its difference is to lie inside that spread.
The file ends with tools/isa_report.py's rows of the pt_render_persistent forms of this build."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, scenes  # noqa: E402


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


frames, reps = int(arg("--frames", 8)), int(arg("--reps", 3))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r32_emission_time.txt"))
parent_lib = arg("--parent-lib", None)
ab_rounds = int(arg("--ab-rounds", 12))

W, H = 1920, 1080
torch.cuda.init()
scene, params = scenes.config_c2(W, H, max_depth=4, n_samples=1)
v = np.array(scene["vert"], np.float32).reshape(-1, 5, 3)
v[:, 2, 0] = np.float32(0.37) * v[:, 0, 0] + np.float32(0.11) * v[:, 0, 2]
v[:, 2, 1] = np.float32(0.37) * v[:, 0, 1] + np.float32(0.23) * v[:, 0, 2]
# one more emitter material that no triangle uses: case (b) binds its map there
spare = np.array(scenes._mat_rows(scenes.emitter((1.0, 1.0, 1.0))), np.float32)
scene = dict(scene, vert=v.reshape(-1, 3), mat=np.concatenate([scene["mat"].reshape(-1, 3), spare], 0))
types = scene["mat"].reshape(-1, 18)[:, 0].astype(int)
k_spare = types.size - 1
diffuse = np.flatnonzero(types == 2)
lamps = np.flatnonzero(types == 1)[:-1]
assert lamps.size > 0 and scene["light"].reshape(-1, 4).shape[0] > 0
rng = np.random.default_rng(32)
S = 1024
tex = [(rng.integers(0, 256, (S, S, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear") for _ in diffuse]
k_one, k_big = len(tex), len(tex) + 1
tex.append((np.ones((1, 1, 4), np.float32), "rgba32f", "repeat", "nearest"))
tex.append((rng.integers(0, 256, (S, S, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear"))
bind = np.full(types.size, -1, np.int32)
bind[diffuse] = np.arange(len(diffuse))


def at(materials, k):
    a = np.full(types.size, -1, np.int32)
    a[materials] = k
    return a


CASES = {
    "(a) textured": None,
    "(b) unused": at([k_spare], k_one),
    "(c) lamp-1x1": at(lamps, k_one),
    "(d) lamp-1024": at(lamps, k_big),
}


def prepare(d):
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H); d.set_variant(1); d.count_rays(False)
    d.upload_textures(tex, bind)


def burst(d, f0):
    d.timer_begin()
    for f in range(frames):
        d.render(dict(params, seed=host.frame_seed(f0 + f)))
    return d.timer_end() / frames


d = device.Device(0)
prepare(d)
ms, kernels = {name: [] for name in CASES}, {}
for r in range(reps + 1):  # round 0 is the warm-up: code objects, buffers
    for name, emit in CASES.items():
        d.bind_emission_maps(emit)
        d.clear()
        t = burst(d, frames * r)
        kernels[name] = d.last_kernel()
        if r:
            ms[name].append(t)
d.close()

base = float(np.median(ms["(a) textured"]))
lines = [f"Emission maps on one MI355X: config c2, {W} x {H}, depth 4, 1 spp, textured extension megakernel; {len(diffuse)} diffuse materials with a {S} x {S} sRGB albedo "
         f"texture each; {lamps.size} emitter material(s), {scene['light'].reshape(-1, 4).shape[0]} light triangles; the big map {S} x {S} RGBA8 sRGB, bilinear.",
         f"Four cases alternating inside one context: {frames} frames between one pair of events, {reps} bursts after a warm-up round: median [min .. max] ms a frame.", ""]
for name, t in ms.items():
    med = float(np.median(t))
    lines.append(f"{name:18s} {med:8.3f} [{np.min(t):.3f} .. {np.max(t):.3f}] ms a frame   {med - base:+.3f} ms ({100.0 * (med - base) / base:+.1f} %) against (a)   {kernels[name]}")
print("\n".join(lines), flush=True)

if parent_lib:
    import gpu_ab_inproc
    V = []
    for tag, lib in (("parent", parent_lib), ("parent-again", parent_lib), ("this", str(device.lib_path()))):
        m = gpu_ab_inproc.load_device_module(f"emit_{tag.replace('-', '_')}", os.path.abspath(lib))
        dv = m.Device(0)
        prepare(dv)
        dv.count_rays(True); dv.clear(); dv.reset_stats()
        for f in range(2):
            dv.render(dict(params, seed=host.frame_seed(f)))
        dv.sync()
        V.append(dict(name=tag, d=dv, rays=int(dv.stats().rays), image=np.ascontiguousarray(dv.read_accum()).view(np.uint32), ms=[]))
        dv.count_rays(False)
    same = all(x["rays"] == V[0]["rays"] and np.array_equal(x["image"], V[0]["image"]) for x in V)
    for r in range(ab_rounds + 1):
        order = list(range(len(V)))
        order = order[r % len(V):] + order[:r % len(V)]  # rotate who goes first
        for k in order:
            V[k]["d"].clear()
            t = burst(V[k]["d"], frames * r)
            if r:
                V[k]["ms"].append(t)
    ref = np.asarray(V[0]["ms"])
    ab = ["", f"---- case (a) against the parent commit, built side by side: three contexts in this process, {frames} frames a burst, {ab_rounds} rounds in rotating order after a "
          f"warm-up round; images and ray counts of two frames {'identical' if same else 'DIFFER'}."]
    for x in V:
        t = np.asarray(x["ms"])
        q = np.percentile((t - ref) / ref * 100.0, [25, 50, 75])
        ab.append(f"{x['name']:14s} median {np.median(t):.4f} ms a frame [{t.min():.4f} .. {t.max():.4f}]   per-round difference to parent: median {q[1]:+.2f} % (quartiles {q[0]:+.2f} .. {q[2]:+.2f})")
    for x in V:
        x["d"].close()
    print("\n".join(ab), flush=True)
    lines += ab

this = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_report.py")], capture_output=True, text=True, timeout=300).stdout.splitlines()
lines += ["", "---- tools/isa_report.py, this commit: the forms of pt_render_persistent<COUNT_RAYS, EXT, VOL, TEX, ENV, MAPS, CUT[, Emit]>", this[0], this[1]]
lines += [ln for ln in this if "pt_render_persistent" in ln]
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
