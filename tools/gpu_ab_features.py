"""A/B timing of glrtx_render_features between builds of libglrtx.so INSIDE ONE PROCESS, as tools/gpu_ab_inproc.py does for frames: every variant gets a context
of its own, all on one stream created here, and the timed bursts go round the variants in turn.  A burst is `--calls` feature passes between one pair of HIP
events on that stream; the figure is microseconds per pass (the counter's memset included); the host's time to issue a pass is printed beside it.

    python tools/gpu_ab_features.py [--config headline] [--calls 50] [--rounds 30] [--out FILE] NAME=path/to/lib.so ...

Forms, each timed for every variant: the plain pass, G on (glrtx_track_motion), a texture set, textures + G, material maps, maps + G.  Every diffuse material
is bound to a 64 x 64 float texture and, for the maps forms, every diffuse and conductor material to a flat normal map.  Before timing, the planes of every
variant are compared with the first variant's, bit for bit.  Name the same library twice (under two file names) to see the spread of the measurement itself.
Set GLRTX_COMPACT_NODES=0/1 to time the other instantiation of the tree kernel."""
import ctypes
import hashlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "opengl-raytracer_amd", "python")); sys.path.insert(0, os.path.join(ROOT, "tools"))
from gpu_ab_inproc import load_device_module  # noqa: E402
from glrt_amd import scenes  # noqa: E402

FORMS = [("plain", False, False, False), ("G", True, False, False), ("textures", False, True, False), ("textures + G", True, True, False),
         ("maps", False, True, True), ("maps + G", True, True, True)]  # (name, geom, tex, maps)


def main():
    a = sys.argv[1:]
    config, calls, rounds, out, variants = "headline", 50, 30, None, []
    while a:
        x = a.pop(0)
        if x == "--config": config = a.pop(0)
        elif x == "--calls": calls = int(a.pop(0))
        elif x == "--rounds": rounds = int(a.pop(0))
        elif x == "--out": out = a.pop(0)
        else: variants.append(x)
    sc, pr = scenes.CONFIGS[config]()
    types = sc["mat"].reshape(-1, 18)[:, 0].astype(np.int32)
    rng = np.random.default_rng(7)
    textures = [(np.tile(np.float32([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear"),
                (rng.uniform(0.1, 0.9, (64, 64, 3)).astype(np.float32), "rgba32f", "repeat", "bilinear")]
    albedo = np.where(types == 2, 1, -1).astype(np.int32)
    normal = np.where((types == 2) | (types == 3), 0, -1).astype(np.int32)

    hip = ctypes.CDLL("libamdhip64.so")
    stream, ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(stream), 1) == 0  # hipStreamNonBlocking
    assert hip.hipEventCreate(ctypes.byref(ev0)) == 0 and hip.hipEventCreate(ctypes.byref(ev1)) == 0
    V = []
    for i, v in enumerate(variants):
        name, path = v.split("=", 1)
        m = load_device_module(f"f{i}", os.path.join(ROOT, path))
        d = m.Device(); d.upload_scene(sc); d.resize(pr["width"], pr["height"]); d.set_stream(stream.value)
        V.append(dict(name=name, d=d, us={f[0]: [] for f in FORMS}, sha={}))

    def bind(d, geom, tex, maps):
        d.track_motion(geom)
        d.upload_textures(textures if tex else None, albedo if tex else None)
        if maps: d.bind_material_maps(normal=normal)

    def burst(d):
        assert hip.hipEventRecord(ev0, stream) == 0
        t0 = time.perf_counter()
        for _ in range(calls): d.render_features(pr)
        issue_us = (time.perf_counter() - t0) * 1e6 / calls  # the host's share: far below the device's figure when the device is what is measured
        assert hip.hipEventRecord(ev1, stream) == 0 and hip.hipEventSynchronize(ev1) == 0
        ms = ctypes.c_float()
        assert hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1) == 0
        return ms.value * 1000.0 / calls, issue_us

    lines = [f"glrtx_render_features, {config} ({pr['width']} x {pr['height']}), {len(V)} variants in one process on one stream, {calls} passes per burst, {rounds} rounds, "
             f"microseconds per pass; differences are per round, against {variants[0].split('=')[0]}"]
    for fname, geom, tex, maps in FORMS:
        for v in V:
            bind(v["d"], geom, tex, maps)
            v["d"].render_features(pr); v["d"].sync()
            planes = list(v["d"].read_features()) + ([v["d"].read_features_geom()] if geom else [])
            v["sha"][fname] = hashlib.sha1(b"".join(np.ascontiguousarray(p).view(np.uint8).tobytes() for p in planes)).hexdigest()
        same = all(v["sha"][fname] == V[0]["sha"][fname] for v in V)
        for r in range(rounds + 2):  # two warm-up rounds
            order = list(range(len(V)))
            order = order[r % len(V):] + order[:r % len(V)]  # rotate who goes first
            for k in order:
                us, issue_us = burst(V[k]["d"])
                if r >= 2: V[k]["us"][fname].append(us); V[k]["issue"] = issue_us
        base = np.asarray(V[0]["us"][fname])
        lines.append(f"---- {fname}: planes {'identical' if same else 'DIFFER'}")
        for v in V:
            us = np.asarray(v["us"][fname]); diff = (us - base) / base * 100.0
            q = np.percentile(diff, [25, 50, 75])
            lines.append(f"{v['name']:10s} median {np.median(us):8.2f}  min {us.min():8.2f} us   vs {V[0]['name']}: median {q[1]:+.2f} %  (quartiles {q[0]:+.2f} .. {q[2]:+.2f});  host issue {v['issue']:.1f} us a pass")
        print("\n".join(lines[-len(V) - 1:]), flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f: f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
