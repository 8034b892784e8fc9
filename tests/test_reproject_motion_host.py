"""The motion-aware reprojection's CPU statements (libglrt_host.so) without a GPU: glrt_reproject_motion against its numpy statement
(tests/reproject_motion_math.py), bit for bit, on hostile arrays and on oracle renders of the headline around a vertex move; glrt_render_features_geom's
geometry plane against glrt_trace_rays, word for word, on a tree and on a vine; and what unmoved geometry must keep."""
import numpy as np
import pytest

import reproject_math as rm
import reproject_motion_math as rmm
from denoise_math import centre_rays
from glrt_amd import host, scenes

CFGS = [dict(max_history=32, depth_tolerance=0.02, normal_tolerance=0.9), dict(max_history=2, depth_tolerance=0.2, normal_tolerance=-1.0)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _numpy(acc, n0, a0, g1, a1, vert_prev, tri, prev, cfg):
    W, S = host.mat4_inverse(prev["c2w"]), host.mat4_inverse(prev["s2c"])
    return rmm.reproject_motion(acc, n0, a0, g1, a1, vert_prev, tri, W, S, rm.origin(prev["c2w"]), **cfg)


def _check(acc, n0, a0, g1, a1, vert_prev, tri, prev, cfg, what):
    got, carried, hits = host.reproject_motion(acc, n0, a0, g1, a1, vert_prev, tri, prev, **cfg)
    ref, carried2, hits2 = _numpy(acc, n0, a0, g1, a1, vert_prev, tri, prev, cfg)
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


def moved_scene(scene, vert):
    """The scene with new vertices and its tree refitted (topology kept: triangle indices name the same material points)."""
    vert = np.ascontiguousarray(vert, np.float32).reshape(-1, 15)
    return dict(scene, vert=vert.reshape(np.asarray(scene["vert"]).shape), bvh=host.refit_bvh(vert, scene["tri"], scene["bvh"]).reshape(np.asarray(scene["bvh"]).shape))


def lifted(scene, material, dy):
    v = np.array(np.asarray(scene["vert"], np.float32).reshape(-1, 15))
    v[rmm.vertices_of_material(scene, material), 1] += np.float32(dy)
    return v


# ---- 1. glrt_reproject_motion against the numpy statement
@pytest.mark.parametrize("rows,width", [(37, 61), (16, 16), (5, 130), (1, 1), (70, 49)])
def test_equals_numpy_on_hostile_arrays(rows, width):
    _, params = scenes.config_c1(width, rows, max_depth=4, subdiv=1)
    acc, n0, a0, g1, a1, vert, tri = rmm.hostile_arrays(rows, width, rows * 1000 + width)
    cfgs = CFGS + [dict(max_history=1000, depth_tolerance=1e3, normal_tolerance=-2.0), dict(max_history=1, depth_tolerance=1e-40, normal_tolerance=1e-40),
                   dict(max_history=2 ** 31 - 1, depth_tolerance=3e38, normal_tolerance=-3e38)]
    some = 0
    for prev in (params, rm.move_camera(params, "pan", 1.0), rm.move_camera(params, "dolly", 0.3), rm.move_camera(params, "orbit", 2.0)):
        for cfg in cfgs:
            some += _check(acc, n0, a0, g1, a1, vert, tri, prev, cfg, f"{width}x{rows} {cfg}")[1]
    assert some > 0 or rows * width == 1
    away = rm.move_camera(params, "pan", 180.0)  # the old camera looks the other way: s.w <= 0 for every point in front of it
    for cfg in cfgs:
        got, carried, _ = _check(acc, n0, a0, g1, a1, vert, tri, away, cfg, f"{width}x{rows} looking away {cfg}")
        assert carried == 0 and not got.any()
    # a carried range that ends early: every index from there on is out of range, on both sides
    for n_tri in (0, 1, tri.shape[0] // 2):
        _check(acc, n0, a0, g1, a1, vert, tri[:n_tri], params, CFGS[1], f"{width}x{rows} {n_tri} triangles carried")


def test_equals_numpy_on_headline_renders():
    """Oracle renders of the headline at 192x108 before a move; the planes after it: one sphere lifted, everything turned, and nothing moved."""
    W, H = 192, 108
    scene, pa = scenes.config_headline(W, H)
    acc = _oracle_accum(scene, pa, 3)
    n0, a0 = host.render_features(scene, pa, W, H)
    v0 = np.asarray(scene["vert"], np.float32).reshape(-1, 15)
    total = 0
    for what, v1 in (("lift", lifted(scene, 5, 0.3)), ("turn", rmm.rotate_vertices(v0, -3.0)), ("still", v0)):
        _, a1, g1 = host.render_features_geom(moved_scene(scene, v1), pa, W, H)
        for cfg in CFGS:
            _, carried, hits = _check(acc, n0, a0, g1, a1, v0, scene["tri"], pa, cfg, f"headline {what} {cfg}")
            total += carried
            assert carried > 0.5 * hits, (what, carried, hits)
    assert total > 0


def test_refusals():
    z = np.ones((3, 5, 4), np.float32)
    z[..., 0] = 0
    _, params = scenes.config_c1(5, 3, max_depth=4, subdiv=1)
    vert, tri = np.zeros((3, 15), np.float32), np.array([[0, 1, 2, 0]], np.float32)
    host.reproject_motion(z, z, z, z, z, vert, tri, params)
    for bad in (dict(max_history=0), dict(max_history=-3), dict(depth_tolerance=0.0), dict(depth_tolerance=-1.0), dict(depth_tolerance=float("nan")),
                dict(depth_tolerance=float("inf")), dict(normal_tolerance=float("nan")), dict(normal_tolerance=float("-inf"))):
        with pytest.raises(RuntimeError):
            host.reproject_motion(z, z, z, z, z, vert, tri, params, **bad)
    for key in ("c2w", "s2c"):
        with pytest.raises(RuntimeError):
            host.reproject_motion(z, z, z, z, z, vert, tri, dict(params, **{key: np.zeros(16, np.float32)}))
    with pytest.raises(RuntimeError, match="-2"):
        host.reproject_motion(z, z, z, z, z, vert, np.array([[0, 1, 3, 0]], np.float32), params)  # a vertex index out of range
    with pytest.raises(ValueError):
        host.reproject_motion(z, z, z[:2], z, z, vert, tri, params)


def test_unmoved_geometry_equals_the_static_call_where_it_counts():
    """Nothing moved and the camera stayed: every hit pixel carries history, and the counts are the static call's (the point is the same up to rounding, so
    the four taps and their tests are; the means differ by the rounding of the point alone)."""
    scene, params = scenes.config_c1(96, 64, max_depth=4, subdiv=1)
    acc = _oracle_accum(scene, params, 5)
    n0, a0, g0 = host.render_features_geom(scene, params, 96, 64)
    for cfg in CFGS:
        out, carried, hits = host.reproject_motion(acc, n0, a0, g0, a0, scene["vert"], scene["tri"], params, **cfg)
        ref, carried_s, hits_s = host.reproject(acc, n0, a0, n0, a0, params, params, **cfg)
        assert carried == hits == hits_s == carried_s and hits > 0.5 * 96 * 64
        got_n = out[..., 3][out[..., 3] != 0]
        assert (got_n == min(5, cfg["max_history"])).all()
        both = (out[..., 3] != 0) & (ref[..., 3] != 0)
        assert np.allclose(out[both][:, :3] / out[both][:, 3:4], ref[both][:, :3] / ref[both][:, 3:4], rtol=0, atol=2e-3 * float(np.abs(ref[both]).max()))


# ---- 2. the geometry plane against the ray queries
def _chain_scene():
    return scenes.config_c3(96, 64, n=3000)


@pytest.mark.parametrize("name", ["headline", "chain"])
def test_geometry_plane_is_the_ray_query(name):
    scene, params = scenes.config_headline(192, 108) if name == "headline" else _chain_scene()
    w, h = params["width"], params["height"]
    n, a, g = host.render_features_geom(scene, params, w, h)
    n_ref, a_ref = host.render_features(scene, params, w, h)
    assert np.array_equal(_bits(n), _bits(n_ref)) and np.array_equal(_bits(a), _bits(a_ref))
    t, tri, u, v = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], centre_rays(params, w, h))
    hit = tri >= 0
    assert hit.sum() > 0.1 * w * h and (~hit).sum() > 0  # (the chain scene's triangles cover 13 % of its image)
    G = g.reshape(-1, 4)
    assert np.array_equal(G[:, 0].view(np.int32), tri)
    assert np.array_equal(_bits(G[hit, 1]), _bits(u[hit])) and np.array_equal(_bits(G[hit, 2]), _bits(v[hit]))
    assert not G[~hit, 1:].any() and not _bits(G[:, 3]).any()
    assert np.array_equal(_bits(n.reshape(-1, 4)[hit, 3]), _bits(t[hit]))
    assert np.array_equal((a[..., 3].view(np.int32) >= 0).reshape(-1), hit)
    assert host.lib().glrt_render_features_geom(None, 0, None, 0, None, 0, None, 0, None, None, 4, 4, 0, 1, 16, None, None, None) == -1
