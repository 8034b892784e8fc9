"""The hand-written loop of the traverse phase (csrc/trav_asm.hip.h: GLRTX_TRAV_LOOP_ASM, driven by wg_traverse_phase): idle count, refill from the wave's
chunk, parking test, stepping block, finished-lane bookkeeping.  Every case is compared bit for bit, ray counts included, with the CPU oracle and with the
megakernel (variant 1, whose traversal is the C++ statement), at the smallest shapes at which the loop can go wrong: one tile (a first pass of exactly 64
rays, one full chunk, then an empty fetch), exactly two chunks, tiles with invalid ids mixed into a chunk, every refill threshold from "any idle lane" to
"all of them", parking never / by default / always, small and large path queues, every node fetch, and the V and T forms.

Every case runs in a child process under a time limit: a loop that fails to end shows as a failed test, not as a stuck test run."""
import json
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

pytestmark = pytest.mark.gpu

_CHILD = r"""
import json, os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {pkg!r}); sys.path.insert(0, {tests!r})
import numpy as np
import torch
if torch.cuda.is_available():
    torch.cuda.init()
from glrt_amd import device, host, scenes
from oracle import pt_oracle

KNOBS = ("GLRTX_REFILL_MIN", "GLRTX_SUSPEND_MAX", "GLRTX_BLOCK_PATHS", "GLRTX_PAIR_FETCH", "GLRTX_COMPACT_NODES")
spec = json.loads(sys.argv[1])
d = device.Device()


def same(a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def run(variant, params, seeds):
    d.set_variant(variant); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats(); d.count_rays(True)
    if len(seeds) > 1:
        d.render_frames(params, seeds)
    else:
        d.render(dict(params, seed=seeds[0]))
    d.sync()
    st = d.stats()
    return d.read_accum(), int(st.rays), int(st.variant_last), int(st.device_error_pending)


def check(tag, params, seeds, ref, ref_rays):
    acc1, rays1, v1, _ = run(1, params, seeds)
    acc2, rays2, v2, err = run(2, params, seeds)
    bad = []
    if (v1, v2) != (1, 2): bad.append("kernels run: %d %d" % (v1, v2))
    if err: bad.append("device error pending")
    if ref is not None and not same(acc2, ref): bad.append("image differs from the reference")
    if ref_rays is not None and rays2 != ref_rays: bad.append("rays %d, reference %d" % (rays2, ref_rays))
    if not same(acc2, acc1): bad.append("image differs from the megakernel's")
    if rays2 != rays1: bad.append("rays %d, megakernel %d" % (rays2, rays1))
    print("CASE", tag, "FAIL " + "; ".join(bad) if bad else "OK", flush=True)


if spec["kind"] == "plain":
    refs = {{}}
    for c in spec["cases"]:
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(c["env"])
        key = json.dumps([c["cfg"], c["kw"], c["depth"], c["frames"]], sort_keys=True)
        scene, params = scenes.CONFIGS[c["cfg"]](**c["kw"])
        params = dict(params, max_depth=c["depth"])
        seeds = [host.frame_seed(i) for i in range(c["frames"])]
        if key not in refs:  # the oracle's image once per shape
            ref, n = None, 0
            for sd in seeds:
                ref, k = pt_oracle.render(scene, dict(params, seed=sd), accum=ref)
                n += k
            refs[key] = (ref, n)
        d.upload_scene(scene)
        check(c["tag"], params, seeds, *refs[key])
elif spec["kind"] == "volume":
    import test_gpu_volume_wavefront as tv
    scene, params, frames, vol, rgb, cnt = tv.load_volume(tv.FIXTURES[0])
    d.upload_scene(scene); d.upload_volume(**vol); d.set_extensions(device.EXT_VOLUME); d.set_volume_wavefront(True)
    seeds = frames or [params["seed"]]
    acc2, rays2, v2, err = run(2, params, seeds)
    d.set_volume_wavefront(False)
    acc1, rays1, v1, _ = run(2, params, seeds)   # the V form off: the megakernel's volume instantiation takes the launch
    ok = v2 == 2 and v1 == 1 and not err and same(acc2[..., :3], rgb) and same(acc2[..., 3], cnt) and same(acc2, acc1) and rays2 == rays1
    print("CASE volume", "OK" if ok else "FAIL %r" % ((v2, v1, err, rays2, rays1),), flush=True)
else:
    import test_gpu_texture_wavefront as tt
    scene, params, wall, cell_scene, tex = tt._constant_per_cell("nearest")
    seeds = [host.frame_seed(i) for i in range(3)]
    ref, n = None, 0
    for sd in seeds:
        ref, k = pt_oracle.render(cell_scene, dict(params, seed=sd), accum=ref)   # a texture constant over each cell: the per-cell scene's image
        n += k
    d.upload_scene(scene); d.upload_textures([tex], tt._at(scene, wall["material"])); d.set_texture_wavefront(True)
    acc2, rays2, v2, err = run(2, params, seeds)
    d.set_texture_wavefront(False)
    acc1, rays1, v1, _ = run(2, params, seeds)   # the T form off: the textured megakernel takes the launch
    ok = v2 == 2 and v1 == 1 and not err and same(acc2, ref) and rays2 == n and same(acc2, acc1) and rays2 == rays1
    print("CASE texture", "OK" if ok else "FAIL %r" % ((v2, v1, err, rays2, n, rays1),), flush=True)
d.close()
print("DONE", flush=True)
"""


def _run(spec, n_cases, timeout=150):
    code = _CHILD.format(root=str(ROOT), pkg=str(PKG / "python"), tests=str(ROOT / "tests"))
    r = subprocess.run([sys.executable, "-c", code, json.dumps(spec)], capture_output=True, text=True, timeout=timeout)
    out = r.stdout
    assert r.returncode == 0 and "DONE" in out, (r.returncode, out[-2000:], r.stderr[-2000:])
    lines = [ln for ln in out.splitlines() if ln.startswith("CASE ")]
    assert len(lines) == n_cases, out[-2000:]
    failed = [ln for ln in lines if not ln.endswith(" OK")]
    assert not failed, "\n".join(failed)


def _plain(cases):
    _run({"kind": "plain", "cases": cases}, len(cases))


def _case(tag, w, h, depth=3, frames=1, spp=1, env=None, cfg="headline"):
    return dict(tag=tag, cfg=cfg, kw=dict(width=w, height=h, n_samples=spp), depth=depth, frames=frames, env=env or {})


@pytest.mark.parametrize("size", [(8, 8), (16, 8), (9, 9), (65, 1), (24, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_image_shapes_and_render_settings(size):
    """8 x 8: one tile -- a first pass of exactly 64 rays, one full chunk, then an empty fetch; 16 x 8: exactly two chunks; 9 x 9 and 65 x 1: tiles with
    invalid ids mixed into a chunk; 24 x 16.  Each at max_depth 1 / 3 / 8, 1 and 3 frames a launch, 1 and 3 samples a pixel."""
    w, h = size
    _plain([_case(f"{w}x{h} depth {dp} frames {fr} spp {spp}", w, h, dp, fr, spp) for dp in (1, 3, 8) for fr in (1, 3) for spp in (1, 3)])


@pytest.mark.parametrize("refill_min", [1, 8, 16, 33, 64])
def test_refill_thresholds(refill_min):
    """From "any idle lane takes a ray at once" to "only when the whole wave idles", on one tile, on tiles with invalid ids and on several chunks a wave."""
    env = {"GLRTX_REFILL_MIN": str(refill_min)}
    _plain([_case(f"refill_min {refill_min} {w}x{h}", w, h, 8, 3, 3, env) for w, h in ((8, 8), (9, 9), (48, 32))])


@pytest.mark.parametrize("suspend_max", [0, 24, 64])
def test_parking_and_path_queue_sizes(suspend_max):
    """Never park, the default, park whenever a wave's share of the queue is used up -- with small and large path queues (paths change position every trip)."""
    _plain([_case(f"suspend_max {suspend_max} block_paths {bp} {w}x{h}", w, h, 8, 3, 3, {"GLRTX_SUSPEND_MAX": str(suspend_max), "GLRTX_BLOCK_PATHS": str(bp)})
            for bp in (256, 1024) for w, h in ((9, 9), (48, 32))])


@pytest.mark.parametrize("compact", [0, 1])
def test_every_node_fetch(compact):
    """One record per lane, pair-cooperative, alternating, each on the 64-byte records and with the compact array asked for, on a tree scene."""
    _plain([_case(f"compact {compact} pair_fetch {pf} refill_min {rm}", 48, 32, 8, 3, 2,
                  {"GLRTX_COMPACT_NODES": str(compact), "GLRTX_PAIR_FETCH": str(pf), "GLRTX_REFILL_MIN": str(rm)}) for pf in (0, 1, 2) for rm in (16, 1)])


def test_volume_form():
    """The V form on its golden fixture: the fixture's image, and the megakernel's volume instantiation, ray count included."""
    _run({"kind": "volume"}, 1)


def test_textured_form():
    """The T form on the textured wall: the oracle's image of the per-cell scene, and the textured megakernel, ray counts included."""
    _run({"kind": "texture"}, 1)
