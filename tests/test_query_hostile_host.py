"""glrt_trace_rays, the CPU statement of the ray queries, on the rays a picking / visibility / height-probe host sends (query_rays.py: axial_rays,
in_plane_rays, feature_rays, range_edge_rays, scaled_rays): exactly axis-aligned directions, rays in box face planes and through box corners, through
vertices and edge midpoints, head-on at coincident faces, range limits one ulp either side of a hit, directions scaled by 2^+-13 .. 2^+-140.

Against a numpy brute force over all triangles and a numpy restatement of the slab test (query_rays.reach), under every builder.  Unlike
test_query_host.py there is NO allowance for lost hits: every hit of the brute force that the statement does not report must lie behind a fork whose box
the restated slab test rejects (query_rays.check_against_brute_force lists the five checks).

Observed over the 27 scenes below, closest hit (any hit in brackets): rays on which the brute force has a hit that the statement does not report --
axial 289 (151) of 6480, in_plane 23 (7) of 6480, feature 74 (6) of 6480, range_edge 210 (86) of 17820, scaled 175 (85) of 12960 -- up to 4.5 % of a set,
above the 1 % that test_query_host.py allows, and every one of them explained by a failing box: mostly rays in a box's face plane, whose NaN slab
product makes them miss that box."""
import numpy as np
import pytest

import query_rays as qr
from fuzz_scenes import fuzz_scene
from glrt_amd import host

BUILDERS = ["sah", "sahl", "lbvh", "chain", "reference", "sah-reinsert"]
FLAGS = {"plain": {}, "axis_aligned": dict(axis_aligned=True), "duplicates": dict(duplicates=True), "degenerate": dict(degenerate=True)}
SHAPES = ["one_child", "one_child_chains", "comb"]  # trees with absent children and the deepest stack (test_compact_nodes.py: KINDS)


def _trace(scene, rays, any_hit=False):
    return host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], rays, any_hit)


def _check(scene, verbose=None):
    """Every hostile set on `scene`, both modes.  Returns {set: counts of the closest-hit run}."""
    out = {}
    for name, rays in qr.hostile_sets(scene).items():
        bf = qr.brute_force(scene, rays)
        for any_hit in (False, True):
            c = qr.check_against_brute_force(scene, rays, _trace(scene, rays, any_hit), bf, any_hit)
            print(f"{verbose or ''} {name} any={int(any_hit)}: {c}")
            if not any_hit:
                out[name] = c
    return out


@pytest.mark.parametrize("flags", list(FLAGS))
@pytest.mark.parametrize("builder", BUILDERS)
def test_fuzz_scenes(builder, flags):
    _check(fuzz_scene(41, 90, builder, **FLAGS[flags]), f"{builder} {flags}")


@pytest.mark.parametrize("kind", SHAPES)
def test_trees_with_absent_children(kind):
    from test_compact_nodes import _scene
    _check(_scene(kind), kind)


# Shares observed on SHARE_SCENES together (the generators are seeded: these are constants), per set: searched rays, rays that meet a NaN slab product
# in a fork they reach, hits on a triangle's edge (u == 0, v == 0 or inv * (U + V) == 1), hits whose distance another reachable triangle shares.
# The floors asserted are HALF of each: room for a numpy version whose random stream differs, none for a generator that silently goes empty.
OBSERVED = {
    "axial": dict(searched=1.0, nan=0.4594, edge=0.0146, tie=0.1292),
    "in_plane": dict(searched=1.0, nan=0.3406, edge=0.0031, tie=0.2052),
    "feature": dict(searched=0.976, nan=0.0, edge=0.0281, tie=0.3063),       # (not searched: the normal of a zero-area triangle is a zero direction)
    "range_edge": dict(searched=0.9091, nan=0.0, edge=0.0174, tie=0.2288),   # (not searched: tmax = 1e-42, one variant in eleven)
    "scaled": dict(searched=0.7469, nan=0.2031, edge=0.0052, tie=0.1068),    # (not searched: 2^+-140 leaves infinite or zero directions)
}
SHARE_SCENES = [("sah", "plain"), ("lbvh", "axis_aligned"), ("sah", "duplicates"), ("reference", "degenerate")]


def _observe():
    tot = {}
    for builder, flags in SHARE_SCENES:
        scene = fuzz_scene(41, 90, builder, **FLAGS[flags])
        for name, rays in qr.hostile_sets(scene).items():
            s = qr.shares(scene, rays, _trace(scene, rays), qr.brute_force(scene, rays))
            for k, v in s.items():
                tot.setdefault(name, {}).setdefault(k, []).append(float(v))
    return {name: {k: float(np.mean(v)) for k, v in d.items()} for name, d in tot.items()}


def test_the_sets_are_hostile():
    """The sets do what they are for, so that the tests above cannot pass on empty inputs: per set, each share of OBSERVED is at least half of what was
    observed when the sets were written."""
    got = _observe()
    print({n: {k: round(v, 4) for k, v in d.items()} for n, d in got.items()})
    for name, want in OBSERVED.items():
        for k, v in want.items():
            assert got[name][k] >= 0.5 * v, f"{name}: share of {k} rays {got[name][k]:.4f}, observed {v:.4f} when the set was written"


def test_range_edges_exclude_and_include_the_hit():
    """tmax = t excludes the hit at t (t < tmax), next(t) includes it; tmin = t excludes it (t > tmin), prev(t) includes it -- on the statement itself."""
    scene = fuzz_scene(41, 90, "sah")
    pool = qr.feature_rays(scene, 400)
    t, tri, _, _ = _trace(scene, pool)
    hit = tri >= 0
    assert hit.sum() > 100
    base, t, tri = pool[hit], t[hit], tri[hit]
    n = len(base)
    v = qr.range_edge_rays(scene, base, t)
    rt, rtri = (x.reshape(11, n) for x in _trace(scene, v)[:2])
    for row in (0, 1, 4):  # tmax = prev(t), tmax = t, tmin = t: the hit is out of range; whatever is found instead lies on the far side of it
        assert ((rtri[row] != tri) | (rt[row] != t)).all()
    assert (rt[0][rtri[0] >= 0] < t[rtri[0] >= 0]).all() and (rt[4][rtri[4] >= 0] > t[rtri[4] >= 0]).all()
    for row in (2, 3, 9):  # tmax = next(t), tmin = prev(t), tmax = FLT_MAX: the same hit
        assert np.array_equal(rtri[row], tri) and np.array_equal(qr.bits(rt[row]), qr.bits(t))
    assert (rtri[10] == -1).all() and (qr.bits(rt[10]) == 0).all()  # a denormal tmax reads as +0: tmax <= tmin, not searched, echoed as read


def test_interleave_builds_the_lane_masks():
    live, dead = np.full((5, 8), 1, np.float32), np.full((3, 8), 2, np.float32)
    pats = qr.lane_patterns()
    for name, mask in pats.items():
        b = qr.interleave(live, dead, name)
        assert b.shape == (len(mask), 8) and np.array_equal(b[:, 0] == 1, mask), name
    chunk = lambda name, c: pats[name][64 * c:64 * (c + 1)]
    assert [int((~chunk(f"dead{k}_start", 1)).sum()) for k in (15, 16, 17)] == [15, 16, 17]
    assert [int((~chunk(f"dead{k}_scattered", 2)).sum()) for k in (15, 16, 17)] == [15, 16, 17]
    assert chunk("one_live_lane31", 3).sum() == 1 and chunk("one_live_lane31", 3)[31]
    assert sorted(len(pats[f"tail{k}_dead"]) % 64 for k in (1, 15, 16, 17, 63)) == [1, 15, 16, 17, 63]
    assert {len(pats[f"chunks{k}"]) // 64 for k in (3, 4, 5, 11, 12, 13)} == {3, 4, 5, 11, 12, 13}
    scene = fuzz_scene(41, 90, "sah")
    d = qr.dead_rays(scene, 90)
    assert (_trace(scene, d)[1] == -1).all() and not qr.reach(scene, d, d[:, 7])[0].any()  # dead: not searched, or the root box is missed
