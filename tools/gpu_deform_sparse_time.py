"""What a sparse morph-target set costs on the GPU box against the dense path with the same targets densified, in the same run, and against its compulsory
traffic.  tools/gpu_deform_time.py's method.

One process, one context per scene (headline, c5 = 100k random triangles) at 1920x1080; the rig is rigid by material, the pose a small turn and shift per bone.
256 targets of small random deltas, each covering a contiguous 3 % of the vertices (target k starts where k * 0.37 % of the vertices end, so neighbours overlap
and a listed vertex is listed by about eight targets of 256).  The sets, uploaded in turn within every round (a rig holds one set at a time):
  sparse, 64 targets     the first 64, with the first 0 / 1 / 16 / 64 active
  sparse, 256 targets    all of them, the first 16 active
  sparse, one entry      64 targets of which only the last lists one vertex, target 0 active: deform_sparse_kernel over rows that are all empty but one
  dense, 64 targets      the yardstick: the unchanged dense path (deform_kernel<false>) with the first 64 densified, the same 0 / 1 / 16 / 64 active
  call, device ms        glrtx_timer_begin / _end (HIP events on the context's stream) around ONE glrtx_pose_morph: a warm-up round, then --rounds rounds;
                         median [min .. max] of the rounds
  kernel alone           glrtx_debug_deform_burst after the call: --reps launches back to back between one pair of events after a warm-up pass, and one launch
                         (reps = 1); against (152 + 4) bytes a vertex plus 32 an entry of the set for the sparse kernel and 152 + 24 x active bytes a vertex
                         for the dense one, at the HBM figure the project uses (6.29 TB/s, the measured float4-copy rate)
Writes the table to profiles/r25_deform_sparse_time.txt (or --out; --append adds to it) and prints it.  Run one scene a process, each under its own time limit:

    timeout -k 10 300 python tools/gpu_deform_sparse_time.py --scenes headline
    timeout -k 10 300 python tools/gpu_deform_sparse_time.py --scenes c5 --append      [--rounds 3] [--reps 20] [--out profiles/r25_deform_sparse_time.txt]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python"))
import torch  # noqa: E402  (initialise torch's HIP runtime before libglrtx's: tests/conftest.py)
from glrt_amd import device, host, rig, scenes  # noqa: E402

HBM = 6.29e12  # bytes / s: the measured float4-copy rate
N_TARGETS, N_DENSE = 256, 64
COVER, STEP = 0.03, 0.0037


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


names = arg("--scenes", "headline,c5").split(",")
rounds, reps = int(arg("--rounds", 3)), int(arg("--reps", 20))
out_path = arg("--out", os.path.join(ROOT, "profiles", "r25_deform_sparse_time.txt"))
append = "--append" in sys.argv


def by_material(sc):
    tri = np.asarray(sc["tri"], np.float32).reshape(-1, 4)
    obj = np.zeros(np.asarray(sc["vert"]).size // 15, np.int32)
    for k in range(3):
        obj[tri[:, k].astype(np.int64)] = tri[:, 3].astype(np.int32)
    return obj, int(np.asarray(sc["mat"]).size // 18)


def pose_of(n_bones, k):
    """tools/gpu_deform_time.py's: bone b turned about y by a few degrees and shifted a little; k picks one of two poses."""
    out = np.zeros((n_bones, 3, 4), np.float32)
    for b in range(n_bones):
        th = np.deg2rad(1.0 + (b % 7) + 3.0 * k)
        c, s = np.cos(th), np.sin(th)
        out[b, :, :3] = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]).astype(np.float32)
        out[b, :, 3] = np.float32(0.01 * (k + 1)) * np.array([1, 0.5, -1], np.float32)
    return out.reshape(n_bones, 12)


def weights_of(n_targets, active, k):
    w = np.zeros(n_targets, np.float32)
    w[:active] = np.float32(0.02 * (k + 1))
    return w


def med(xs):
    return f"{np.median(xs):8.4f} [{np.min(xs):.4f} .. {np.max(xs):.4f}]"


torch.cuda.init()
lines = [] if append else [
    f"glrtx_pose_morph over sparse and dense morph-target sets on one MI355X at 1920x1080: one process and one context a scene, a warm-up round then {rounds} rounds,",
    f"the sets uploaded in turn within a round; kernel bursts of {reps}; bytes against the HBM figure {HBM / 1e12:.2f} TB/s", ""]
for name in names:
    sc, params = scenes.CONFIGS[name](width=1920, height=1080)
    rest = np.ascontiguousarray(np.asarray(sc["vert"], np.float32).reshape(-1, 15))
    n_vert = rest.shape[0]
    obj, n_bones = by_material(sc)
    bones, weights = rig.rigid(obj)
    poses = [pose_of(n_bones, k) for k in range(2)]
    rng = np.random.default_rng(25)
    cover = max(1, int(COVER * n_vert))
    first = (np.arange(N_TARGETS) * max(1, int(STEP * n_vert))) % (n_vert - cover + 1)
    vertex = np.concatenate([np.arange(f, f + cover, dtype=np.uint32) for f in first])
    offsets = (np.arange(N_TARGETS + 1, dtype=np.uint64) * np.uint64(cover))
    deltas = (rng.standard_normal((N_TARGETS * cover, 6)) * 0.01).astype(np.float32)
    dense = np.zeros((N_DENSE, n_vert, 6), np.float32)
    for k in range(N_DENSE):
        dense[k, first[k]:first[k] + cover] = deltas[k * cover:(k + 1) * cover]
    one_off = np.zeros(N_DENSE + 1, np.uint64); one_off[-1] = 1
    sets = {  # name -> (upload, n_targets, entries, [active, ...])
        "sparse,  64 targets": (lambda: d.upload_morph_targets_sparse(offsets[:N_DENSE + 1], vertex[:N_DENSE * cover], deltas[:N_DENSE * cover]), N_DENSE,
                                N_DENSE * cover, (0, 1, 16, 64)),
        "sparse, 256 targets": (lambda: d.upload_morph_targets_sparse(offsets, vertex, deltas), N_TARGETS, N_TARGETS * cover, (16,)),
        "sparse, one entry  ": (lambda: d.upload_morph_targets_sparse(one_off, np.zeros(1, np.uint32), deltas[:1]), N_DENSE, 1, (1,)),
        "dense,   64 targets": (lambda: d.upload_morph_targets(dense), N_DENSE, None, (0, 1, 16, 64)),
    }
    d = device.Device(0)
    d.upload_scene(sc); d.set_partition(0, 1, 16); d.resize(params["width"], params["height"])
    d.upload_rig(rest, bones, weights, n_bones)
    keys = [(s, a) for s, (_, _, _, acts) in sets.items() for a in acts]
    dev_ms, single, burst = {k: [] for k in keys}, {k: [] for k in keys}, {k: [] for k in keys}
    for r in range(rounds + 1):  # (round 0 warms up: code objects, the staging buffer, the pinned copies)
        for s, (upload, n_targets, _, acts) in sets.items():
            upload()
            for a in acts:
                d.timer_begin(); d.pose_morph(poses[r & 1], weights_of(n_targets, a, r & 1)); ms = d.timer_end()
                one, many = d.deform_burst_ms(1), d.deform_burst_ms(reps)
                if r:
                    dev_ms[s, a].append(ms); single[s, a].append(one); burst[s, a].append(many)
    # the timed calls did the work they stand for: the sparse set and its densified twin leave what the CPU statement says (they differ only where a dense + 0
    # meets a negative zero of the rest pose: include/glrtx.h, relation 2)
    w16 = weights_of(N_DENSE, 16, 0)
    sets["sparse,  64 targets"][0](); d.pose_morph(poses[0], w16); a = d.read_scene("nrms").copy()
    d.update_vertices(host.deform_vertices_sparse(rest, bones, weights, poses[0], 0, offsets[:N_DENSE + 1], vertex[:N_DENSE * cover], deltas[:N_DENSE * cover], w16))
    assert np.array_equal(a, d.read_scene("nrms"))
    block = [f"{name}: {n_vert} vertices, {n_bones} bones, targets of {cover} vertices ({100 * cover / n_vert:.1f} %); device bytes of a set: dense 64 targets "
             f"{N_DENSE * n_vert * 24 / 1e6:.1f} MB, sparse 64 targets {(4 * (n_vert + 1) + 32 * N_DENSE * cover) / 1e6:.1f} MB, sparse 256 targets "
             f"{(4 * (n_vert + 1) + 32 * N_TARGETS * cover) / 1e6:.1f} MB",
             f"  {'set, active':30s} {'call, device ms':>32s} {'kernel: one launch, ms':>32s} {'burst of %d, ms' % reps:>32s}     MB   of the HBM figure: one launch, burst"]
    for (s, a) in keys:
        entries = sets[s][2]
        nbytes = n_vert * (152 + 24 * a) if entries is None else n_vert * 156 + 32 * entries
        if entries is not None and a == 0:
            nbytes = n_vert * 152  # (no active weight: deform_kernel<false> with no active target runs, and reads no entry)
        share = lambda ms: nbytes / (np.median(ms) * 1e-3) / HBM * 100
        block.append(f"  {s + ', %2d active' % a:30s} {med(dev_ms[s, a]):>32s} {med(single[s, a]):>32s} {med(burst[s, a]):>32s} {nbytes / 1e6:6.1f}   "
                     f"{share(single[s, a]):5.1f} %  {share(burst[s, a]):5.1f} %")
    block.append("")
    lines += block
    print("\n".join(block), flush=True)
    d.close()
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "a" if append else "w") as f:
    f.write("\n".join(lines) + "\n")
print(f"wrote {out_path}")
