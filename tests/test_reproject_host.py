"""The reprojection's CPU statement (libglrt_host.so: glrt_reproject) against its numpy statement (tests/reproject_math.py), bit for bit, on oracle-rendered
accumulators under three camera moves and on hostile arrays; and what an unmoved camera must keep."""
import numpy as np
import pytest

import reproject_math as rm
from fuzz_scenes import CASES, case_scene_and_params
from glrt_amd import host, scenes

MOVES = [("pan", 2.0), ("dolly", 0.5), ("orbit", 3.0)]
CFGS = [dict(max_history=32, depth_tolerance=0.02, normal_tolerance=0.9), dict(max_history=2, depth_tolerance=0.2, normal_tolerance=-1.0)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _numpy(acc, n0, a0, n1, a1, prev, cur, cfg):
    W, S = host.mat4_inverse(prev["c2w"]), host.mat4_inverse(prev["s2c"])
    return rm.reproject(acc, n0, a0, n1, a1, W, S, rm.origin(prev["c2w"]), cur, **cfg)


def _check(acc, n0, a0, n1, a1, prev, cur, cfg, what):
    got, carried, hits = host.reproject(acc, n0, a0, n1, a1, prev, cur, **cfg)
    ref, carried2, hits2 = _numpy(acc, n0, a0, n1, a1, prev, cur, cfg)
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} pixels differ; first {np.argwhere(bad)[0].tolist()}"
    assert (carried, hits) == (carried2, hits2), (what, carried, hits, carried2, hits2)
    assert carried == int((got[..., 3] != 0).sum()) and hits == int((a1[..., 3].view(np.int32) >= 0).sum())
    return got, carried, hits


def _oracle_accum(scene, params, frames):
    from oracle import pt_oracle
    acc = None
    for f in range(frames):
        acc, _ = pt_oracle.render(scene, dict(params, seed=host.frame_seed(f)), accum=acc)
    return acc


def _scene_case(name):
    if name == "c1":
        scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    else:
        scene, params = case_scene_and_params(CASES[name])
    return scene, params, params["width"], params["height"]


@pytest.mark.parametrize("name", ["c1", 0, 4, 7], ids=lambda c: c if c == "c1" else f"fuzz{CASES[c][0]}-{CASES[c][2]}")
def test_equals_numpy_on_rendered_accumulators(name):
    scene, params, w, h = _scene_case(name)
    acc = _oracle_accum(scene, params, 3)
    n0, a0 = host.render_features(scene, params, w, h)
    total = 0
    for kind, amount in MOVES:
        cur = rm.move_camera(params, kind, amount)
        n1, a1 = host.render_features(scene, cur, w, h)
        for cfg in CFGS:
            _, carried, _ = _check(acc, n0, a0, n1, a1, params, cur, cfg, f"{name} {kind} {cfg}")
            total += carried
    assert total > 0  # (the moves are small: history survives somewhere)


@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (5, 130), (1, 1), (70, 49)])
def test_equals_numpy_on_hostile_arrays(rows, width):
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, n1, a1 = rm.hostile_arrays(rows, width, rows * 1000 + width)
    away = rm.move_camera(params, "pan", 180.0)  # the old camera looks the other way: s.w <= 0 for every point in front of the new one
    cfgs = CFGS + [dict(max_history=1000, depth_tolerance=1e3, normal_tolerance=-2.0), dict(max_history=1, depth_tolerance=1e-40, normal_tolerance=1e-40),
                   dict(max_history=2 ** 31 - 1, depth_tolerance=3e38, normal_tolerance=-3e38)]
    some = 0
    for cur in (params, rm.move_camera(params, "pan", 1.0), rm.move_camera(params, "dolly", 0.3), rm.move_camera(params, "orbit", 2.0)):
        for cfg in cfgs:
            some += _check(acc, n0, a0, n1, a1, params, cur, cfg, f"{width}x{rows} {cfg}")[1]
    assert some > 0 or rows * width == 1
    for cfg in cfgs:
        got, carried, _ = _check(acc, n0, a0, n1, a1, away, params, cfg, f"{width}x{rows} looking away {cfg}")
        assert carried == 0 and not got.any()


def test_refusals():
    z = np.ones((3, 5, 4), np.float32)
    _, params = scenes.config_c1(5, 3, max_depth=4, subdiv=1)
    host.reproject(z, z, z, z, z, params, params)
    for bad in (dict(max_history=0), dict(max_history=-3), dict(depth_tolerance=0.0), dict(depth_tolerance=-1.0), dict(depth_tolerance=float("nan")),
                dict(depth_tolerance=float("inf")), dict(normal_tolerance=float("nan")), dict(normal_tolerance=float("-inf"))):
        with pytest.raises(RuntimeError):
            host.reproject(z, z, z, z, z, params, params, **bad)
    for key in ("c2w", "s2c"):
        with pytest.raises(RuntimeError):
            host.reproject(z, z, z, z, z, dict(params, **{key: np.zeros(16, np.float32)}), params)  # a singular previous camera
    host.reproject(z, z, z, z, z, params, dict(params, c2w=np.zeros(16, np.float32)))  # (the new camera is not inverted)
    with pytest.raises(ValueError):
        host.reproject(z, z, z[:2], z, z, params, params)


def _unmoved_expectation(acc, n0, a0, cfg):
    """Pixels of an unmoved camera whose four neighbours (and themselves) pass the id, normal, depth and count tests against them: whatever u - x rounds to,
    every tap that can get weight carries the pixel's surface, so with equal counts the count must come back exactly."""
    rows, width = acc.shape[:2]
    ids = a0[..., 3].view(np.int32)
    ok = np.zeros((rows, width), bool)
    ok[1:-1, 1:-1] = True
    for dy, dx in ((0, 0), (0, 1), (0, -1), (1, 0), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)):
        P = (slice(1, rows - 1), slice(1, width - 1))
        Q = (slice(1 + dy, rows - 1 + dy), slice(1 + dx, width - 1 + dx))
        dot = (n0[P][..., :3] * n0[Q][..., :3]).sum(-1)
        ok[P] &= (ids[P] >= 0) & (ids[Q] == ids[P]) & (dot >= cfg["normal_tolerance"] + 1e-3) & (acc[Q][..., 3] == acc[P][..., 3]) & \
                 (np.abs(n0[Q][..., 3] - n0[P][..., 3]) <= 0.9 * cfg["depth_tolerance"] * n0[P][..., 3])  # (e = the pixel's own distance up to rounding)
    return ok


@pytest.mark.parametrize("statement", ["numpy", "host"])
def test_unmoved_camera_keeps_its_counts(statement):
    """c1 at 96x64, 5 frames, the same camera twice.  The numpy statement alone is checked first (parametrised before the CPU statement): every hit pixel
    carries history (carried == hit_pixels), and every pixel whose four neighbours pass the tests keeps exactly min(count, max_history)."""
    scene, params, w, h = _scene_case("c1")
    acc = _oracle_accum(scene, params, 5)
    n0, a0 = host.render_features(scene, params, w, h)
    for cfg in CFGS:
        if statement == "numpy":
            out, carried, hits = _numpy(acc, n0, a0, n0, a0, params, params, cfg)
        else:
            out, carried, hits = host.reproject(acc, n0, a0, n0, a0, params, params, **cfg)
        assert carried == hits and hits > 0.5 * w * h, (carried, hits)
        ok = _unmoved_expectation(acc, n0, a0, cfg)
        print(f"{statement} {cfg}: carried {carried} of {hits} hit pixels; {int(ok.sum())} pixels with all neighbours passing")
        assert ok.sum() >= (2000 if cfg["depth_tolerance"] >= 0.1 else 100)  # (at 96x64 a neighbour on the floor is often more than 2 % farther away)
        want = np.minimum(acc[..., 3], np.float32(cfg["max_history"]))
        assert np.array_equal(out[..., 3][ok], want[ok]), int((out[..., 3][ok] != want[ok]).sum())
        # the oracle gives every pixel the same count, so here the count must survive wherever anything is carried at all: rint(sum(w c) / sum(w)) = c
        got_n = out[..., 3][out[..., 3] != 0]
        assert (acc[..., 3] == 5).all() and (got_n == min(5, cfg["max_history"])).all()
        mean_old = acc[ok][:, :3] / acc[ok][:, 3:4]
        mean_new = out[ok][:, :3] / out[ok][:, 3:4]
        # the mean moves only by the bilinear blend over |u - x| <~ 1e-4 of a pixel (the depth test rejects nothing here)
        assert np.allclose(mean_new, mean_old, rtol=0, atol=2e-3 * max(1.0, float(np.abs(mean_old).max())))
