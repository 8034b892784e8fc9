"""What a deform costs on the GPU box: glrtx_pose_morph with 0, 1, 4 and 16 active morph targets and glrtx_pose_dualquat against glrtx_pose in the same run, and
the deform kernel alone against its compulsory traffic.  tools/gpu_pose_time.py's method.

One process, one context per scene (headline, c5 = 100k random triangles) at 1920x1080; the rig is rigid by material, the pose a small turn and shift per bone,
the dual quaternions glrt_dualquat_from_matrix of the same matrices; 16 targets of small random deltas are uploaded once, and a call's weights make the first
0, 1, 4 or 16 of them active.
  call, device ms      glrtx_timer_begin / _end (HIP events on the context's stream) around ONE call: a warm-up round, then --rounds rounds, the calls
                       alternating within a round; median [min .. max] of the rounds
  call, wall ms        the same calls under the host clock (they block until the refit has run), the same alternation
  kernel alone         glrtx_debug_deform_burst after the call: --reps launches back to back between one pair of events after a warm-up pass, and one launch
                       (reps = 1, still behind the hook's warm-up launch); against 152 + 24 x active bytes a vertex for matrices (60 rest + 32 rig in, 60 out, 24
                       a target; the bone records are cache-resident) and 136 + 24 x active for dual quaternions (the issue's accounting: a 32-byte bone record
                       against a 48-byte one), at the HBM figure the project uses (6.29 TB/s, the measured float4-copy rate)
Writes the table to profiles/r24_deform_time.txt (or --out; --append adds to it) and prints it.  Run one scene a process, each under its own time limit:

    timeout -k 10 300 python tools/gpu_deform_time.py --scenes headline
    timeout -k 10 300 python tools/gpu_deform_time.py --scenes c5 --append      [--rounds 3] [--reps 20] [--out profiles/r24_deform_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, rig, scenes  # noqa: E402

HBM = 6.29e12  # bytes / s: the measured float4-copy rate
N_TARGETS = 16
ACTIVE = (0, 1, 4, 16)


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


names = arg("--scenes", "headline,c5").split(",")
rounds, reps = int(arg("--rounds", 3)), int(arg("--reps", 20))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r24_deform_time.txt"))
append = "--append" in sys.argv


def by_material(sc):
    tri = np.asarray(sc["tri"], np.float32).reshape(-1, 4)
    obj = np.zeros(np.asarray(sc["vert"]).size // 15, np.int32)
    for k in range(3):
        obj[tri[:, k].astype(np.int64)] = tri[:, 3].astype(np.int32)
    return obj, int(np.asarray(sc["mat"]).size // 18)


def pose_of(n_bones, k):
    """Bone b turned about y by a few degrees and shifted a little; k picks one of two poses so that consecutive calls move something."""
    out = np.zeros((n_bones, 3, 4), np.float32)
    for b in range(n_bones):
        th = np.deg2rad(1.0 + (b % 7) + 3.0 * k)
        c, s = np.cos(th), np.sin(th)
        out[b, :, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).astype(np.float32)
        out[b, :, 3] = np.float32(0.01 * (k + 1)) * np.array([1, 0.5, -1], np.float32)
    return out.reshape(n_bones, 12)


def weights_of(active, k):
    w = np.zeros(N_TARGETS, np.float32)
    w[:active] = np.float32(0.02 * (k + 1))
    return w


def med(xs):
    return f"{np.median(xs):8.3f} [{np.min(xs):.3f} .. {np.max(xs):.3f}]"


torch.cuda.init()
lines = [] if append else [
    f"glrtx_pose_morph / glrtx_pose_dualquat on one MI355X at 1920x1080: one process and one context a scene, a warm-up round then {rounds} rounds, the calls",
    f"alternating; kernel bursts of {reps}; bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]
for name in names:
    sc, params = scenes.CONFIGS[name](width=1920, height=1080)
    rest = np.ascontiguousarray(np.asarray(sc["vert"], np.float32).reshape(-1, 15))
    n_vert = rest.shape[0]
    obj, n_bones = by_material(sc)
    bones, weights = rig.rigid(obj)
    poses = [pose_of(n_bones, k) for k in range(2)]
    dqs = [rig.dualquat(p) for p in poses]
    rng = np.random.default_rng(24)
    deltas = (rng.standard_normal((N_TARGETS, n_vert, 6)) * 0.01).astype(np.float32)
    d = device.Device(0)
    d.upload_scene(sc); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"])
    d.upload_rig(rest, bones, weights, n_bones)
    d.upload_morph_targets(deltas)
    calls = {"pose": (lambda k: d.pose(poses[k]), None)}
    for a in ACTIVE:
        calls[f"pose_morph, {a:2d} active"] = (lambda k, a=a: d.pose_morph(poses[k], weights_of(a, k)), 152 + 24 * a)
    calls["pose_dualquat,  0 active"] = (lambda k: d.pose_dualquat(dqs[k], weights_of(0, k)), 136)
    calls["pose_dualquat,  4 active"] = (lambda k: d.pose_dualquat(dqs[k], weights_of(4, k)), 136 + 24 * 4)
    dev_ms, wall_ms = {c: [] for c in calls}, {c: [] for c in calls}
    burst, single = {c: [] for c in calls}, {c: [] for c in calls}
    for r in range(rounds + 1):  # (round 0 warms up: code objects, the staging buffer, the pinned copies)
        for c, (fn, per_vertex) in calls.items():
            d.timer_begin(); fn(r & 1); ms = d.timer_end()
            t0 = time.perf_counter(); fn(~r & 1); wall = 1e3 * (time.perf_counter() - t0)
            one, many = (d.deform_burst_ms(1), d.deform_burst_ms(reps)) if per_vertex else (d.skin_burst_ms(1), d.skin_burst_ms(reps))
            if r:
                dev_ms[c].append(ms); wall_ms[c].append(wall); single[c].append(one); burst[c].append(many)
    # the timed calls did the work they stand for: no active target leaves what a pose leaves, and 16 active ones what the CPU statement says
    d.pose(poses[0]); a = d.read_scene("root").copy()
    d.pose_morph(poses[0], weights_of(0, 0)); assert np.array_equal(a, d.read_scene("root"))
    d.pose_morph(poses[0], weights_of(16, 0)); a = d.read_scene("nrms").copy()
    d.update_vertices(host.deform_vertices(rest, bones, weights, poses[0], 0, deltas, weights_of(16, 0))); assert np.array_equal(a, d.read_scene("nrms"))
    block = [f"{name}: {n_vert} vertices, {n_bones} bones, {N_TARGETS} targets of {n_vert * 24 / 1e6:.1f} MB each",
             f"  {'call':26s} {'device ms':>28s} {'wall ms':>28s}"]
    for c in calls:
        block.append(f"  {c:26s} {med(dev_ms[c]):>28s} {med(wall_ms[c]):>28s}")
    block.append(f"  {'kernel alone':26s} {'one launch, ms':>28s} {'burst of %d, ms' % reps:>28s}   MB   of the HBM figure: one launch, burst")
    for c, (fn, per_vertex) in calls.items():
        nbytes = n_vert * (per_vertex or 152)
        share = lambda ms: nbytes / (np.median(ms) * 1e-3) / HBM * 100
        block.append(f"  {c:26s} {med(single[c]):>28s} {med(burst[c]):>28s} {nbytes / 1e6:6.1f}   {share(single[c]):5.1f} %  {share(burst[c]):5.1f} %")
    block.append("")
    lines += block
    print("\n".join(block), flush=True)
    d.close()
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
