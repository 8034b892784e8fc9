#!/usr/bin/env python3
"""The fixtures of tests/test_reference_live.py: every scene and accumulator that test puts through the reference's unmodified shaders, with what the reference
made of it on Mesa llvmpipe (oracle/glref, the same runner as make_golden.py and make_golden_screen.py).  The test compares the oracle with these records, so it
runs wherever the repository is checked out; this script is how they are made again.  Build container only (needs the reference checkout and Mesa's swrast_dri.so):

    make -C oracle && python tests/golden/make_golden_live.py

tests/golden/live/<group>.npz, one record per case, its arrays stored as "<key>__<field>":
  render groups (configs, fuzz, hostile, shadow_hostile): vert tri mat light bvh c2w s2c scalars fparams (load_golden's fields) + out_rgb out_count
  screen groups (screen, screen_hostile):                 rgb count gammas (NaN: the shader's default, 2.2) + out (RGBA8 per gamma, row 0 = bottom row)
The records sit in a subdirectory so that conftest.golden_names() does not take them for fixtures of test_oracle_golden.py.
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parents[1]
OUT = HERE / "live"
for p in (ROOT, ROOT / "tests", ROOT / "opengl-raytracer_amd" / "python", HERE):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

# the six configurations of test_oracle_bit_exact_vs_live_reference: (config, builder kwargs, param overrides)
CASES = [
    ("c1", dict(width=96, height=64, max_depth=6, n_samples=2), {}),
    ("c1", dict(width=64, height=64, max_depth=3, n_samples=1), dict(aperture=0.2, focal=9.0, seed=(0.91, 0.33))),
    ("c2", dict(width=96, height=54, max_depth=8, n_samples=1, subdiv=1), dict(seed=(0.5, 0.25))),
    ("c3", dict(width=64, height=36, max_depth=2, n=800), {}),
    ("c4", dict(width=64, height=36, max_depth=8, n_samples=4, subdiv=1), {}),
    ("c5", dict(width=64, height=36, max_depth=4, n=5000), dict(seed=(0.123, 0.987))),
]
N_SHADOW_HOSTILE = 32
RENDER_FIELDS = ("vert", "tri", "mat", "light", "bvh", "c2w", "s2c", "scalars", "fparams", "out_rgb", "out_count")


def render_inputs():
    """{group: [(key, scene, params)]}: the inputs of the render tests, in test order."""
    from fuzz_scenes import CASES as FUZZ_CASES, case_scene_and_params, shadow_hostile
    from glrt_amd import scenes
    from hostile_cases import cases as hostile_cases
    configs = []
    for i, (cfg, kw, over) in enumerate(CASES):
        sc, pr = scenes.CONFIGS[cfg](**kw)
        configs.append((f"case{i}", sc, dict(pr, **over)))
    sc, pr = scenes.config_c1(48, 48, max_depth=5, n_samples=1, subdiv=1)
    rng = np.random.default_rng(5)
    for j in range(6):
        configs.append((f"seeds{j}", sc, dict(pr, seed=tuple(float(np.float32(v)) for v in rng.uniform(0, 1, 2)))))
    fuzz = [(f"seed{c[0]}",) + tuple(case_scene_and_params(c)) for c in FUZZ_CASES]
    hostile = [(f"hostile{i}", sc, p) for i, (tag, sc, p) in enumerate(hostile_cases())]
    shadow = []
    for seed in range(N_SHADOW_HOSTILE):
        _, sc, pr = shadow_hostile(seed)
        shadow.append((f"seed{seed}", sc, pr))
    return {"configs": configs, "fuzz": fuzz, "hostile": hostile, "shadow_hostile": shadow}


def screen_inputs():
    """{group: [(key, rgb, count, gammas)]}: the inputs of the resolve-pass tests, in test order (a gamma of None: the shader's default)."""
    from glrt_amd import scenes
    from make_golden_screen_r04 import extreme_accumulator
    from oracle import pt_oracle
    screen = []
    rng = np.random.default_rng(99)
    for h, w in ((128, 256), (32, 32)):
        rgb = (rng.random((h, w, 3), dtype=np.float32) ** 2 * 60).astype(np.float32)
        cnt = rng.integers(1, 65, (h, w)).astype(np.float32)
        screen.append((f"random{h}x{w}", rgb, cnt, (2.2, 1.8, 1.0, 3.0)))
    sc, pr = scenes.config_c2(64, 32, max_depth=4, n_samples=8, subdiv=1)
    acc, _ = pt_oracle.render(sc, pr)
    screen.append(("render", acc[..., :3].copy(), acc[..., 3].copy(), (None,)))
    hostile = []
    acc = extreme_accumulator()
    rng = np.random.default_rng(404)
    for it in range(12):
        a = acc.copy()
        rng.shuffle(a.reshape(-1, 4))  # another arrangement of the same texels
        gamma = float(rng.choice([2.2, 1.0, 0.45, 1e-20, 1e20, 3.0, 1e-45, 3e38, float(rng.uniform(0.1, 5))]))
        hostile.append((f"arrangement{it}", a[..., :3].copy(), a[..., 3].copy(), (gamma,)))
    return {"screen": screen, "screen_hostile": hostile}


def load(group):
    """{key: {field: array}} of tests/golden/live/<group>.npz."""
    z = np.load(OUT / f"{group}.npz")
    out = {}
    for name in z.files:
        key, field = name.split("__")
        out.setdefault(key, {})[field] = z[name]
    return out


def render_record(rec):
    """(scene, params, rgb, count) of a render record, the params as load_golden builds them."""
    scene = {k: rec[k] for k in ("vert", "tri", "mat", "light", "bvh")}
    w, h, depth, spp = (int(v) for v in rec["scalars"])
    sx, sy, ap, fo = (float(v) for v in rec["fparams"])
    params = dict(c2w=rec["c2w"], s2c=rec["s2c"], width=w, height=h, max_depth=depth, n_samples=spp, seed=(sx, sy), aperture=ap, focal=fo)
    return scene, params, rec["out_rgb"], rec["out_count"]


def main():
    from oracle.glref import GLRef
    g = GLRef()
    OUT.mkdir(exist_ok=True)
    for group, items in render_inputs().items():
        arrays = {}
        for key, sc, p in items:
            rgb, cnt = g.render_reference(sc, p)
            rec = dict(vert=sc["vert"], tri=sc["tri"], mat=sc["mat"], light=sc["light"], bvh=sc["bvh"],
                       c2w=np.asarray(p["c2w"], np.float32).reshape(16), s2c=np.asarray(p["s2c"], np.float32).reshape(16),
                       scalars=np.array([p["width"], p["height"], p["max_depth"], p["n_samples"]], np.int32),
                       fparams=np.array([p["seed"][0], p["seed"][1], p.get("aperture", 0.0), p.get("focal", 1.0)], np.float32),
                       out_rgb=rgb, out_count=cnt)
            arrays.update({f"{key}__{f}": np.asarray(rec[f]) for f in RENDER_FIELDS})
        np.savez_compressed(OUT / f"{group}.npz", **arrays)
        print(f"{group}: {len(items)} records")
    for group, items in screen_inputs().items():
        arrays = {}
        for key, rgb, cnt, gammas in items:
            out = [g.render_screen(rgb, cnt) if gm is None else g.render_screen(rgb, cnt, gm) for gm in gammas]
            arrays.update({f"{key}__rgb": rgb, f"{key}__count": cnt, f"{key}__out": np.stack(out),
                           f"{key}__gammas": np.array([np.nan if gm is None else gm for gm in gammas], np.float64)})
        np.savez_compressed(OUT / f"{group}.npz", **arrays)
        print(f"{group}: {len(items)} records")


if __name__ == "__main__":
    main()
