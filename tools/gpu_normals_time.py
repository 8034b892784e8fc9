"""What rebuilding normals costs on the GPU box (csrc/normals.hip.h; include/glrtx.h "Rebuilding normals"), against its compulsory traffic and against the calls
it sits beside.  tools/gpu_deform_time.py's method: one process, one context a mesh, a warm-up round then --rounds rounds with the variants alternated inside
every round; median [min .. max] of the rounds.

  meshes                headline (30 756 vertices, 5160 classes), c5 (100k random triangles: 300 000 vertices, all singleton classes), icosphere(7) (327 680
                        triangles, 983 040 vertices, classes of 5 and 6; a lamp quad beside it), and two fans of 100 000 triangles: one whose hub class
                        lists 1000 of them (four chunks on one lane) against one of hubs of 8 faces each -- the same size without the long list
  rebuild alone         glrtx_debug_normals_burst: --reps rebuilds back to back between one pair of events after a warm-up pass, and one rebuild (reps = 1),
                        against the header's compulsory bytes -- 68 a triangle, 20 a class, 20 a face-list entry, 32 a vertex -- at the HBM figure the project
                        uses (6.29 TB/s, the measured float4-copy rate)
  pose, switch on / off glrtx_timer_begin / _end (HIP events on the context's stream) around ONE glrtx_pose of a one-bone rig, with glrtx_set_pose_normals on and
                        off in turn; the kernel alone by glrtx_debug_skin_burst
  position update       one glrtx_update_positions_device of a torch tensor (n, 3), one glrtx_update_vertices_device of ready-made vertices (n, 15), one
                        glrtx_update_positions from host memory and one glrtx_update_vertices from host memory, in turn, timed the same way
Writes the table to profiles/r26_normals_time.txt (or --out; --append adds to it) and prints it.  Run one mesh a process, each under its own time limit:

    timeout -k 10 300 python tools/gpu_normals_time.py --meshes headline
    timeout -k 10 300 python tools/gpu_normals_time.py --meshes c5 --append     [--rounds 5] [--reps 20] [--out profiles/r26_normals_time.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, rig, scenes  # noqa: E402

HBM = 6.29e12  # bytes / s: the measured float4-copy rate


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


names = arg("--meshes", "headline,c5,icosphere7,fan1000,fan8").split(",")
rounds, reps = int(arg("--rounds", 5)), int(arg("--reps", 20))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r26_normals_time.txt"))
append = "--append" in sys.argv


def fans(n_tri, per_hub, long_hub=0):
    """n_tri triangles in fans of per_hub faces around one hub each; with long_hub, the first long_hub triangles share ONE hub instead."""
    k = np.arange(n_tri)
    hub = np.where(k < long_hub, 0, long_hub + (k - long_hub) // per_hub) if long_hub else k // per_hub
    ang = 2 * np.pi * (k % 1000) / 1000.0
    centre = np.stack([3.0 * (hub % 100), 3.0 * (hub // 100), np.zeros(n_tri)], -1)
    rim0 = centre + np.stack([np.cos(ang), np.sin(ang), np.full(n_tri, -0.1)], -1)
    rim1 = centre + np.stack([np.cos(ang + 0.005), np.sin(ang + 0.005), np.full(n_tri, -0.1)], -1)
    pos = np.stack([centre, rim0, rim1], 1)
    nrm = np.broadcast_to([0.0, 0.0, 1.0], pos.shape)
    return pos, nrm


def mesh_scene(pos, nrm):
    b = scenes.SceneBuilder()
    b.add_mesh(pos, nrm, b.add_material(scenes.diffuse((0.7, 0.7, 0.7))))
    b.add_mesh(*scenes.quad((-1, 50, -1), (2, 0, 0), (0, 0, 2)), b.add_material(scenes.emitter((10.0, 10.0, 10.0))))
    return b.build("lbvh")


def make(name):
    if name in scenes.CONFIGS:
        return scenes.CONFIGS[name](width=256, height=144)[0]
    if name == "icosphere7":
        return mesh_scene(*scenes.icosphere(7, 1.0, (0.0, 0.0, 0.0)))
    if name == "fan1000":
        return mesh_scene(*fans(100_000, 8, long_hub=1000))
    if name == "fan8":
        return mesh_scene(*fans(100_000, 8))
    raise ValueError(name)


def med(xs):
    return f"{np.median(xs) * 1e3:8.1f} [{np.min(xs) * 1e3:.1f} .. {np.max(xs) * 1e3:.1f}]"


def timed(d, fn):
    d.timer_begin(); fn(); return d.timer_end()


torch.cuda.init()
lines = [] if append else [
    f"Rebuilding normals on one MI355X: one process and one context a mesh, a warm-up round then {rounds} rounds, the variants alternated inside a round;",
    f"bursts of {reps}; times in microseconds, median [min .. max]; bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]
for name in names:
    sc = make(name)
    rest = np.ascontiguousarray(np.asarray(sc["vert"], np.float32).reshape(-1, 15))
    tri = np.ascontiguousarray(np.asarray(sc["tri"], np.float32).reshape(-1, 4))
    n_vert, n_tri = rest.shape[0], tri.shape[0]
    cls, flip, n_classes = host.normal_topology(rest, tri)
    sizes = np.bincount(cls)
    c = tri[:, 0:3].astype(np.int64)
    k = np.sort(cls[c], 1)
    entries = int(n_tri + (k[:, 1] != k[:, 0]).sum() + (k[:, 2] != k[:, 1]).sum())  # a triangle is listed once by each distinct class of its corners
    longest = int(np.bincount(np.concatenate([k[:, 0], k[(k[:, 1] != k[:, 0]), 1], k[(k[:, 2] != k[:, 1]), 2]])).max())
    nbytes = 68 * n_tri + 20 * n_classes + 20 * entries + 32 * n_vert
    moved = [rest[:, 0:3] * np.float32(s) for s in (1.01, 0.99)]
    V = [host.rebuild_normals(host.positions_to_vertices(rest, p), tri, cls, flip) for p in moved]
    tp, tv = [torch.from_numpy(p.copy()).cuda() for p in moved], [torch.from_numpy(v).cuda() for v in V]
    torch.cuda.synchronize()
    bones, weights = rig.rigid(np.zeros(n_vert, np.int32))
    poses = [np.array([[s, 0, 0, 0, 0, s, 0, 0, 0, 0, s, 0]], np.float32) for s in (1.01, 0.99)]
    d = device.Device(0)
    d.upload_scene(sc); d.set_partition(0, 1, 16); d.resize(256, 144)
    d.upload_rig(rest, bones, weights, 1)
    d.upload_normal_topology(rest, tri)
    keys = ("rebuild, one", "rebuild, burst", "skin kernel, burst", "pose, switch off", "pose, switch on", "update_positions_device", "update_vertices_device",
            "update_positions (host)", "update_vertices (host)")
    t = {key: [] for key in keys}
    for r in range(rounds + 1):  # (round 0 warms up: code objects, the staging buffers)
        i = r & 1
        row = {}
        d.set_pose_normals(False); row["pose, switch off"] = timed(d, lambda: d.pose(poses[i]))
        d.set_pose_normals(True); row["pose, switch on"] = timed(d, lambda: d.pose(poses[i]))
        row["skin kernel, burst"] = d.skin_burst_ms(reps)
        row["update_positions_device"] = timed(d, lambda: d.update_positions(tp[i]))
        row["update_vertices_device"] = timed(d, lambda: d.update_vertices(tv[i]))
        row["update_positions (host)"] = timed(d, lambda: d.update_positions(moved[i]))
        row["update_vertices (host)"] = timed(d, lambda: d.update_vertices(V[i]))
        row["rebuild, one"], row["rebuild, burst"] = d.normals_burst_ms(1), d.normals_burst_ms(reps)
        if r:
            for key in keys:
                t[key].append(row[key])
    # the timed calls did the work they stand for
    d.update_positions(tp[0]); a = d.read_scene("nrms").copy()
    d.update_vertices(V[0])
    assert np.array_equal(a, d.read_scene("nrms"))
    share = lambda ms: nbytes / (np.median(ms) * 1e-3) / HBM * 100
    block = [f"{name}: {n_vert} vertices, {n_tri} triangles, {n_classes} classes (largest {int(sizes.max())} members), {entries} face-list entries (longest list "
             f"{longest}); compulsory bytes of a rebuild {nbytes / 1e6:.2f} MB"]
    for key in keys:
        tail = f"   {share(t[key]):5.1f} % of the HBM figure" if key.startswith("rebuild") else ""
        block.append(f"  {key:28s} {med(t[key]):>36s} us{tail}")
    block.append("")
    lines += block
    print("\n".join(block), flush=True)
    d.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
