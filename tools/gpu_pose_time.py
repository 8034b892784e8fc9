"""What a pose costs on the GPU box: glrtx_pose (csrc/skin.hip.h + the refit) against the two ways the same vertices could reach the refit before it, and the
skinning kernel alone against its compulsory traffic.

One process, one context per scene (headline, c5 = 100k random triangles) at 1920x1080; the rig is rigid by material, the pose a small turn and shift per bone.
  call, device ms      glrtx_timer_begin / _end (HIP events on the context's stream) around ONE call, for the same pose:
                         pose             glrtx_pose: n_bones x 48 bytes up, the skinning kernel, the refit's three kernels, the 7-word read-back
                         update (device)  glrtx_update_vertices_device from a tensor that already holds the skinned vertices
                         update (host)    glrtx_update_vertices from host memory: n_vert x 60 bytes across PCIe first
                       a warm-up round, then --rounds rounds, the three calls alternating within a round; median [min .. max] of the rounds
  call, wall ms        the same calls under the host clock (they block until the refit has run), the same alternation
  kernel alone         glrtx_debug_skin_burst: --reps launches back to back between one pair of events after a warm-up pass, and one launch (reps = 1, still
                       behind the hook's warm-up launch); against 152 bytes a vertex (60 rest + 32 rig in, 60 out; the matrices are cache-resident) at the HBM
                       figure the project uses (6.29 TB/s, the measured float4-copy rate).  Both run with the kernel's data where the launch before left it (46 MB
                       for config 5 fit the 256 MB Infinity Cache); "pose - update (device)", the difference of the two device medians, is the kernel with
                       the matrix upload in place: behind a refit and in front of one.
Writes the table to profiles/r23_pose_time.txt (or --out) and prints it.

    python tools/gpu_pose_time.py [--scenes headline,c5] [--rounds 3] [--reps 20] [--out profiles/r23_pose_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, rig, scenes  # noqa: E402

HBM = 6.29e12  # bytes / s: the measured float4-copy rate
BYTES_PER_VERTEX = 60 + 32 + 60


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


names = arg("--scenes", "headline,c5").split(",")
rounds, reps = int(arg("--rounds", 3)), int(arg("--reps", 20))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r23_pose_time.txt"))


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


def med(xs):
    return f"{np.median(xs):8.3f} [{np.min(xs):.3f} .. {np.max(xs):.3f}]"


torch.cuda.init()
lines = [f"glrtx_pose on one MI355X at 1920x1080: one process, one context a scene, a warm-up round then {rounds} rounds, the calls alternating; kernel bursts of {reps};",
         f"bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]
for name in names:
    sc, params = scenes.CONFIGS[name](width=1920, height=1080)
    rest = np.ascontiguousarray(np.asarray(sc["vert"], np.float32).reshape(-1, 15))
    obj, n_bones = by_material(sc)
    bones, weights = rig.rigid(obj)
    poses = [pose_of(n_bones, k) for k in range(2)]
    skinned = [host.skin_vertices(rest, bones, weights, p) for p in poses]
    d = device.Device(0)
    d.upload_scene(sc); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"])
    d.upload_rig(rest, bones, weights, n_bones)
    tv = [torch.from_numpy(v).cuda() for v in skinned]
    torch.cuda.synchronize()
    calls = {"pose": lambda k: d.pose(poses[k]), "update (device)": lambda k: d.update_vertices(tv[k]), "update (host)": lambda k: d.update_vertices(skinned[k])}
    dev_ms, wall_ms = {c: [] for c in calls}, {c: [] for c in calls}
    for r in range(rounds + 1):  # (round 0 warms up: code objects, the staging buffer, the pinned copies)
        for c, fn in calls.items():
            d.timer_begin(); fn(r & 1); ms = d.timer_end()
            t0 = time.perf_counter(); fn(~r & 1); wall = 1e3 * (time.perf_counter() - t0)
            if r:
                dev_ms[c].append(ms); wall_ms[c].append(wall)
    # the three leave the same scene behind (the tests pin that byte for byte; here the root box is enough of a check that the timed calls did the same work)
    d.pose(poses[0]); a = d.read_scene("root").copy()
    d.update_vertices(skinned[0]); assert np.array_equal(a, d.read_scene("root"))
    burst, single = [], []
    for r in range(rounds + 1):
        d.pose(poses[r & 1])
        one = d.skin_burst_ms(1)
        many = d.skin_burst_ms(reps)
        if r:
            single.append(one); burst.append(many)
    n_vert = rest.shape[0]
    nbytes = n_vert * BYTES_PER_VERTEX
    share = lambda ms: f"{nbytes / (np.median(ms) * 1e-3) / HBM * 100:5.1f} % of the HBM figure"
    lines += [f"{name}: {n_vert} vertices, {n_bones} bones, vertex upload {n_vert * 60 / 1e6:.1f} MB, kernel traffic {nbytes / 1e6:.1f} MB",
              f"  pose, device ms                   {med(dev_ms['pose'])}",
              f"  update (device vertices)          {med(dev_ms['update (device)'])}",
              f"  update (host vertices)            {med(dev_ms['update (host)'])}",
              f"  pose, wall ms                     {med(wall_ms['pose'])}",
              f"  update (device vertices), wall    {med(wall_ms['update (device)'])}",
              f"  update (host vertices), wall      {med(wall_ms['update (host)'])}",
              f"  pose - update (device), device ms {np.median(dev_ms['pose']) - np.median(dev_ms['update (device)']):8.3f}   {share([np.median(dev_ms['pose']) - np.median(dev_ms['update (device)'])])}",
              f"  kernel alone, burst of {reps:<3d} (ms)   {med(burst)}   {share(burst)}",
              f"  kernel alone, one launch (ms)     {med(single)}   {share(single)}", ""]
    print("\n".join(lines[-11:]), flush=True)
    d.close()
    del tv
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
