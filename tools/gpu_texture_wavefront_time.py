"""Textures and material maps on the wavefront kernel (glrtx_set_texture_wavefront: pt_render_wgwf's T and TM forms) against the textured extension
megakernel, on the GPU box.  Config c2 at 1920 x 1080, depth 4, 1 spp; tools/gpu_texture_time.py's set (every diffuse material bound to its own 1024 x 1024
bilinear RGBA8 sRGB texture) and tools/gpu_maps_time.py's maps (a 1024 x 1024 RGBA32F normal map on every diffuse and conductor material, a 1024 x 1024
RGBA8 roughness map on the conductors); the coordinates are those tools' planar map of the positions.  Five cases ALTERNATING inside one process (README
"Measuring a change"): every repetition runs each case once, in rotating order, so drift of the box lands on all of them alike.

  t-form        the albedo set on the T form (switch on)
  mega-tex      the same set on the megakernel's textured kernel (switch off)
  wavefront     the scene untextured on the plain wavefront kernel, for scale
  tm-form       albedo set + maps on the TM form
  mega-maps     the same on the megakernel's MAPS kernel

Three contexts (albedo set | albedo set + maps | untextured); the switch is toggled between bursts.  A burst is --frames glrtx_render calls after a warm-up
round: ms a frame by HIP events on the context's stream (glrtx_timer_begin / _end) and by the host clock around issue + sync; median [min .. max] of --reps.
Before anything is timed, one 1080p frame of each textured case is compared bit for bit between the two kernels, rays included: a difference ends the run.

    timeout -k 10 500 python tools/gpu_texture_wavefront_time.py [--frames 8] [--reps 3] [--out profiles/r30_texture_wavefront.txt] [--append]"""
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
out_path = arg("--out", os.path.join(ROOT, "profiles", "r30_texture_wavefront.txt"))
os.environ.pop("GLRTX_TEXTURE_WAVEFRONT", None)

W, H = 1920, 1080
torch.cuda.init()
scene, params = scenes.config_c2(W, H, max_depth=4, n_samples=1)
v = np.array(scene["vert"], np.float32).reshape(-1, 5, 3)
v[:, 2, 0] = np.float32(0.37) * v[:, 0, 0] + np.float32(0.11) * v[:, 0, 2]
v[:, 2, 1] = np.float32(0.37) * v[:, 0, 1] + np.float32(0.23) * v[:, 0, 2]
scene = dict(scene, vert=v.reshape(-1, 3))
types = scene["mat"].reshape(-1, 18)[:, 0].astype(int)
diffuse, conductor = np.flatnonzero(types == 2), np.flatnonzero(types == 3)
rng = np.random.default_rng(29)
S = 1024
tex = [(rng.integers(0, 256, (S, S, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear") for _ in diffuse]
k_bump, k_rough = len(tex), len(tex) + 1
m = np.concatenate([rng.uniform(-0.5, 0.5, (S, S, 2)), np.ones((S, S, 1))], -1)
tex.append((((m / np.linalg.norm(m, axis=-1, keepdims=True) + 1.0) / 2.0).astype(np.float32), "rgba32f", "repeat", "bilinear"))
tex.append((rng.integers(10, 128, (S, S, 4), dtype=np.uint8), "rgba8_unorm", "repeat", "bilinear"))
bind = np.full(types.size, -1, np.int32)
bind[diffuse] = np.arange(len(diffuse))
surfaces = np.isin(types, (2, 3))


def context(textured, maps):
    d = device.Device(0)
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H); d.set_variant(2); d.count_rays(False)
    if textured:
        d.upload_textures(tex, bind)
    if maps:
        d.bind_material_maps(normal=np.where(surfaces, k_bump, -1), roughness=np.where(types == 3, k_rough, -1))
    return d


d_tex, d_maps, d_plain = context(True, False), context(True, True), context(False, False)
CASES = {  # name -> (context, switch, the variant it must run on)
    "t-form": (d_tex, True, 2), "mega-tex": (d_tex, False, 1), "wavefront": (d_plain, False, 2), "tm-form": (d_maps, True, 2), "mega-maps": (d_maps, False, 1),
}

# ---- the same bits first: one frame of each textured set on both kernels, rays counted
for d, what in ((d_tex, "albedo set"), (d_maps, "albedo set + maps")):
    got = []
    for on in (True, False):
        d.set_texture_wavefront(on); d.count_rays(True); d.clear(); d.reset_stats()
        d.render(dict(params, seed=host.frame_seed(7))); d.sync()
        st = d.stats()
        assert st.variant_last == (2 if on else 1) and st.device_error_pending == 0, (what, on, st.variant_last)
        got.append((d.read_accum(), int(st.rays), int(st.rays_untraced)))
        d.count_rays(False)
    same = np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32)) and got[0][1:] == got[1][1:]
    print(f"{what}: one {W} x {H} frame, wavefront form vs megakernel: {'bit-identical' if same else 'DIFFERENT'}, {got[0][1]} rays ({got[0][2]} untraced) vs {got[1][1]} ({got[1][2]})", flush=True)
    if not same:
        raise SystemExit("the two kernels differ: nothing is timed")


def burst(name, f0):
    d, on, variant = CASES[name]
    d.set_texture_wavefront(on)
    d.clear(); d.sync()
    t0 = time.perf_counter()
    d.timer_begin()
    for f in range(frames):
        d.render(dict(params, seed=host.frame_seed(f0 + f)))
    ev = d.timer_end() / frames
    d.sync()
    wall = (time.perf_counter() - t0) * 1e3 / frames
    assert d.stats().variant_last == variant, (name, d.stats().variant_last)
    return ev, wall


names = list(CASES)
ms = {n: [] for n in names}
for r in range(reps + 1):  # round 0 is the warm-up: code objects, buffers, pipe slots
    for k in range(len(names)):
        n = names[(k + r) % len(names)]
        t = burst(n, 1000 * (r + 1))
        if r:
            ms[n].append(t)
for d in (d_tex, d_maps, d_plain):
    d.close()

med = {n: float(np.median([t[0] for t in ms[n]])) for n in names}
lines = [f"Textures on the wavefront kernel, one MI355X: config c2, {W} x {H}, depth 4, 1 spp; {len(diffuse)} diffuse materials with a {S} x {S} bilinear sRGB albedo texture each; "
         f"maps: a {S} x {S} RGBA32F normal map on every diffuse and conductor material, a {S} x {S} RGBA8 roughness map on the {len(conductor)} conductor(s).",
         f"Five cases alternating in one process: {frames} glrtx_render calls a burst, {reps} repetitions after a warm-up round.  ms a frame, median [min .. max]: HIP events | host clock.",
         "One 1080p frame of each textured set was bit-identical on both kernels, rays included, before the timing.", ""]
for n in names:
    ev, wall = [t[0] for t in ms[n]], [t[1] for t in ms[n]]
    lines.append(f"{n:10s} {np.median(ev):8.3f} [{np.min(ev):.3f} .. {np.max(ev):.3f}] | {np.median(wall):8.3f} [{np.min(wall):.3f} .. {np.max(wall):.3f}] ms a frame")
lines += ["",
          f"t-form / mega-tex    {med['t-form'] / med['mega-tex']:.3f}   (mega-tex / t-form {med['mega-tex'] / med['t-form']:.2f} x)",
          f"tm-form / mega-maps  {med['tm-form'] / med['mega-maps']:.3f}   (mega-maps / tm-form {med['mega-maps'] / med['tm-form']:.2f} x)",
          f"t-form - wavefront   {med['t-form'] - med['wavefront']:+.3f} ms ({100.0 * (med['t-form'] - med['wavefront']) / med['wavefront']:+.1f} %): what the albedo lookups cost on the wavefront kernel",
          f"tm-form - t-form     {med['tm-form'] - med['t-form']:+.3f} ms ({100.0 * (med['tm-form'] - med['t-form']) / med['t-form']:+.1f} %): what the maps cost on top"]
print("\n".join(lines), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
new = "--append" not in sys.argv or not os.path.exists(out_path)
with open(out_path, "w" if new else "a") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
