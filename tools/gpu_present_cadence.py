"""Presentation cadence at the 1080p headline (C2 scene, 8 bounces, 1 spp), in ONE context (contexts differ by up to 3 %: profiles/r04_context_regimes.txt).
Three forms of 48 frames, alternated over --passes passes, wall time per frame from the first call until the last image / the last sync:
  (a) a burst of 48 glrtx_render calls, no presentation (the headline's fed burst; nothing reads the accumulator)
  (b) the same burst with presentation (glrtx_present_enable): every image acquired and released on this thread -- with a ring of 48 (whole burst) and of 8
      (the host waits for the oldest image whenever the ring is full)
  (c) today's loop: glrtx_render, glrtx_sync, glrtx_resolve_rgba8 per frame (the reference's cadence, window.cpp:157-164)
Prints a table (and writes it to --out FILE if given).  --trace: only a few bursts of (a) and (b) (for rocprofv3 --kernel-trace --stats: the fused pass
accumulate_present_feed_kernel against accumulate_feed_kernel)."""
import argparse
import pathlib
import statistics
import sys
import time

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT)); sys.path.insert(0, str(ROOT / "opengl-raytracer_amd" / "python"))
import numpy as np  # noqa: E402
from glrt_amd import device, host, scenes  # noqa: E402

N = 48


def burst(d, params, f0, ring=0):
    seeds = [host.frame_seed(f0 + i) for i in range(N)]
    if ring:
        d.present_enable(ring, 2.2, True)
    t0 = time.perf_counter()
    got = 0
    for i, sd in enumerate(seeds):
        if ring and i - got >= ring:  # ring full: the oldest image first
            img = d.present_acquire(wait=True); d.present_release(img); got += 1
        d.render(dict(params, seed=sd))
        if ring:
            img = d.present_acquire(wait=False)
            if img is not None:
                d.present_release(img); got += 1
    while ring and got < N:
        img = d.present_acquire(wait=True); d.present_release(img); got += 1
    d.sync()
    ms = (time.perf_counter() - t0) * 1e3 / N
    if ring:
        d.present_enable(0)
    return ms


def synced(d, params, f0):
    out = np.zeros((1080, 1920, 4), np.uint8)
    t0 = time.perf_counter()
    for i in range(N):
        d.render(dict(params, seed=host.frame_seed(f0 + i)))
        d.sync()
        d.L.glrtx_resolve_rgba8(d.h, out.ctypes.data, 1920 * 4, 2.2, 1)
    return (time.perf_counter() - t0) * 1e3 / N


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=4)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", type=pathlib.Path, default=None, help="also write the table to this file")
    a = ap.parse_args()
    scene, params = scenes.CONFIGS["headline"]()
    d = device.Device(0)
    d.upload_scene(scene); d.resize(1920, 1080); d.clear()
    if a.trace:
        for k in range(3):
            burst(d, params, 100 * k)
            burst(d, params, 100 * k + 50, ring=N)
        print("trace bursts done")
        return
    forms = {"a_burst": lambda f0: burst(d, params, f0), "b_present_ring48": lambda f0: burst(d, params, f0, ring=48),
             "b_present_ring8": lambda f0: burst(d, params, f0, ring=8), "c_sync_resolve": lambda f0: synced(d, params, f0)}
    for name, fn in forms.items():  # warm-up
        fn(0)
    res = {k: [] for k in forms}
    st_feed = {}
    for p in range(a.passes):
        for k, (name, fn) in enumerate(forms.items()):
            d.reset_stats()
            res[name].append(fn(1000 * (p + 1) + 100 * k))
            st = d.stats()
            st_feed[name] = (int(st.kernel_launches), int(st.feed_appended))
    ps_ms = d.present_stats().pass_ms_last
    lines = [f"1920x1080 headline (C2, depth 8, 1 spp), {N} frames per form, one context, {a.passes} passes alternating the forms; wall ms per frame",
             f"{'form':20s} {'median':>8s} {'min':>8s} {'max':>8s}  launches/feed_appended (last pass)   passes"]
    for name, v in res.items():
        lines.append(f"{name:20s} {statistics.median(v):8.3f} {min(v):8.3f} {max(v):8.3f}  {st_feed[name][0]:4d} / {st_feed[name][1]:4d}                    "
                     + " ".join(f"{x:.3f}" for x in v))
    a_med = statistics.median(res["a_burst"])
    for name in ("b_present_ring48", "b_present_ring8", "c_sync_resolve"):
        lines.append(f"{name} / a_burst = {statistics.median(res[name]) / a_med:.3f}")
    lines.append(f"last presenting pass (fused accumulate + resolve, HIP events): {ps_ms:.4f} ms")
    text = "\n".join(lines)
    print(text)
    if a.out is not None:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(text + "\n")


if __name__ == "__main__":
    main()
