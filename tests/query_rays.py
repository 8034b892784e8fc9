"""Ray sets and a brute-force statement for the ray-query tests (glrt_trace_rays / glrtx_trace_rays)."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(np.float32).max
CHUNK = 64  # rays a wave of the device's query kernel claims at a time (csrc/query.hip.h: kChunk)


def _pos(scene):
    return np.asarray(scene["vert"], F32).reshape(-1, 15)[:, :3]


def _tris(scene):
    t = np.asarray(scene["tri"], F32).reshape(-1, 4)[:, :3].astype(np.int64)
    p = _pos(scene)
    return p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ftz(x):
    """Denormals as the zero of their sign: how the device and the CPU statement (FTZ | DAZ) read every input and write every result."""
    b = bits(x)
    return np.where((b & np.uint32(0x7F800000)) == 0, b & np.uint32(0x80000000), b).astype(np.uint32).view(F32)


def pack(o, d, tmin, tmax):
    n = o.shape[0]
    r = np.zeros((n, 8), F32)
    r[:, 0:3] = o
    r[:, 3] = tmin
    r[:, 4:7] = d
    r[:, 7] = tmax
    return r


def camera_rays(params, width=None, height=None, tmin=1e-4, tmax=1e8):
    """Pinhole rays through pixel centres, from the renderer's camera matrices (c2w, s2c: column-major float[16])."""
    w = width or params["width"]
    h = height or params["height"]
    c2w = np.asarray(params["c2w"], np.float64).reshape(4, 4).T
    s2c = np.asarray(params["s2c"], np.float64).reshape(4, 4).T
    y, x = np.mgrid[0:h, 0:w]
    ndc = np.stack([(x.ravel() + 0.5) / w * 2 - 1, (y.ravel() + 0.5) / h * 2 - 1, np.ones(w * h), np.ones(w * h)], 1)
    p = ndc @ s2c.T
    p = p[:, :3] / p[:, 3:4]
    d = p @ c2w[:3, :3].T
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o = np.broadcast_to(c2w[:3, 3], d.shape)
    return pack(o.astype(F32), d.astype(F32), tmin, tmax)


def surface_points(scene, n, rng):
    v0, v1, v2 = _tris(scene)
    k = rng.integers(0, v0.shape[0], n)
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    p = v0[k] + a[:, None] * (v1[k] - v0[k]) + b[:, None] * (v2[k] - v0[k])
    nrm = np.cross(v1[k] - v0[k], v2[k] - v0[k]).astype(np.float64)
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-30), np.array([0.0, 0.0, 1.0]))
    return p.astype(F32), nrm


def incoherent_rays(scene, n, seed=1, tmin=1e-4, tmax=1e8):
    """Cosine-distributed directions about the surface normal (either side at random), from random points on the surfaces."""
    rng = np.random.default_rng(seed)
    p, nrm = surface_points(scene, n, rng)
    nrm = nrm * np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)[:, None]
    u1, u2 = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    r, phi = np.sqrt(u1), 2 * np.pi * u2
    local = np.stack([r * np.cos(phi), r * np.sin(phi), np.sqrt(np.maximum(0.0, 1 - u1))], 1)
    a = np.where(np.abs(nrm[:, :1]) > 0.9, np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t = np.cross(a, nrm)
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    b = np.cross(nrm, t)
    d = local[:, :1] * t + local[:, 1:2] * b + local[:, 2:3] * nrm
    return pack(p, d.astype(F32), tmin, tmax)


def shadow_rays(scene, n, seed=2):
    """From random surface points to random points on the light triangles (all triangles when the scene has none): direction = the unnormalised
    difference, tmin = 1e-4, tmax = 1 - 1e-4."""
    rng = np.random.default_rng(seed)
    p, _ = surface_points(scene, n, rng)
    light = np.asarray(scene["light"], F32).reshape(-1, 4)
    pos = _pos(scene)
    if light.shape[0]:
        lt = light[:, :3].astype(np.int64)
        k = rng.integers(0, lt.shape[0], n)
        l0, l1, l2 = pos[lt[k, 0]], pos[lt[k, 1]], pos[lt[k, 2]]
    else:
        v0, v1, v2 = _tris(scene)
        k = rng.integers(0, v0.shape[0], n)
        l0, l1, l2 = v0[k], v1[k], v2[k]
    a, b = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    flip = a + b > 1
    a, b = np.where(flip, 1 - a, a), np.where(flip, 1 - b, b)
    q = (l0 + a[:, None] * (l1 - l0) + b[:, None] * (l2 - l0)).astype(F32)
    return pack(p, (q - p).astype(F32), 1e-4, 1.0 - 1e-4)


def special_rays():
    """Rays that need no search: NaN / infinite components, zero directions, tmax <= tmin; plus a denormal tmin."""
    nan, inf = F32(np.nan), F32(np.inf)
    rows = []
    base = [0.0, 0.0, 5.0, 1e-4, 0.0, 0.0, -1.0, 1e8]
    for i in range(8):
        for bad in (nan, inf, -inf):
            r = list(base)
            r[i] = bad
            rows.append(r)
    rows.append([0.0, 0.0, 5.0, 1e-4, 0.0, 0.0, 0.0, 1e8])       # zero direction
    rows.append([0.0, 0.0, 5.0, 1e-4, -0.0, 0.0, -0.0, 1e8])     # signed zeros
    rows.append([0.0, 0.0, 5.0, 2.0, 0.0, 0.0, -1.0, 2.0])       # tmax == tmin
    rows.append([0.0, 0.0, 5.0, 3.0, 0.0, 0.0, -1.0, 1.0])       # tmax < tmin
    rows.append([0.0, 0.0, 5.0, -1e8, 0.0, 0.0, -1.0, -2e8])     # both negative, reversed
    return np.asarray(rows, F32)


def brute_force(scene, rays, block=512):
    """Every triangle against every ray, in float32 with the device's operation order, no fused multiply-adds and denormals flushed (inputs and every
    result).  Returns (hit mask (n, T), t (n, T), u, v, inv * (U + V)): hit[i, k] when triangle k passes the renderer's test with tmin < t < tmax."""
    v0, v1, v2 = (ftz(x) for x in _tris(scene))
    e1, e2 = ftz(v1 - v0), ftz(v2 - v0)
    rays = ftz(np.asarray(rays, F32).reshape(-1, 8))
    z = ftz

    def dot3(a, b):
        return z(z(z(a[..., 2] * b[..., 2]) + z(a[..., 1] * b[..., 1])) + z(a[..., 0] * b[..., 0]))

    def cross(a, b):
        return np.stack([z(z(a[..., 1] * b[..., 2]) - z(a[..., 2] * b[..., 1])), z(z(a[..., 2] * b[..., 0]) - z(a[..., 0] * b[..., 2])),
                         z(z(a[..., 0] * b[..., 1]) - z(a[..., 1] * b[..., 0]))], -1)

    out = []
    for s in range(0, max(len(rays), 1), block):
        r = rays[s:s + block]
        o, d = r[:, None, 0:3], r[:, None, 4:7]
        tmin, tmax = r[:, 3:4], r[:, 7:8]
        with np.errstate(all="ignore"):
            shape = (len(r), len(v0), 3)
            p = cross(np.broadcast_to(d, shape), np.broadcast_to(e2[None], shape))
            det = dot3(np.broadcast_to(e1[None], shape), p)
            inv = z(np.where(np.isinf(det), F32(np.nan), F32(1.0) / det).astype(F32))
            tv = z(o - v0[None])
            U = dot3(tv, p)
            u = z(U * inv)
            q = cross(tv, np.broadcast_to(e1[None], shape))
            V = dot3(np.broadcast_to(d, shape), q)
            v = z(V * inv)
            t = z(dot3(np.broadcast_to(e2[None], shape), q) * inv)
            w = z(inv * z(U + V))
            hit = ~((F32(-1e-4) < det) & (det < F32(1e-4))) & ~((u < 0) | (1 < u)) & ~((v < 0) | (1 < w)) & (t > tmin) & (t < tmax)
        out.append((hit, t, u, v, w))
    return tuple(np.concatenate([o[k] for o in out], 0) for k in range(5))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Comparisons shared by the host and the device tests


def check_real_hits(scene, rays, res, bf):
    """Every reported hit is a triangle the brute force accepts, with bit-equal t, u, v; a miss echoes tmax (as the query reads it: a denormal as
    the zero of its sign, include/glrtx.h) with tri = -1 and u = v = 0."""
    hit, t, u, v = bf[:4]
    rt, rtri, ru, rv = res
    idx = np.nonzero(rtri >= 0)[0]
    k = rtri[idx]
    assert hit[idx, k].all(), "a reported hit that the triangle test rejects"
    assert np.array_equal(bits(rt[idx]), bits(t[idx, k]))
    assert np.array_equal(bits(ru[idx]), bits(u[idx, k]))
    assert np.array_equal(bits(rv[idx]), bits(v[idx, k]))
    miss = rtri < 0
    assert (rtri[miss] == -1).all()
    assert np.array_equal(bits(rt[miss]), bits(ftz(rays[miss, 7]))) and (ru[miss] == 0).all() and (rv[miss] == 0).all()


def compare(d, scene, rays, what, any_hit):
    """The device's four words per ray == the CPU statement's, bit for bit."""
    from glrt_amd import host
    got = np.stack([np.asarray(x).view(np.uint32) for x in d.trace_rays(rays, any_hit=any_hit)], 1)
    ref = np.stack([np.asarray(x).view(np.uint32) for x in host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], rays, any_hit)], 1)
    if not np.array_equal(got, ref):
        bad = np.nonzero((got != ref).any(1))[0]
        i = bad[0]
        raise AssertionError(f"{what} any={any_hit}: {len(bad)} of {len(rays)} rays differ; first {i}: ray {rays[i].tolist()} device {got[i].tolist()} "
                             f"cpu {ref[i].tolist()}")


# ---------------------------------------------------------------------------------------------------------------------------------------------
# The tree and the slab test restated in numpy (no device, no C): which leaves a ray may reach


def tree(scene):
    """The wire tree (9 floats per node: box lo, box hi, children.x, children.y, leaf triangle or < 0): (nodes (n, 9), forks in top-down order,
    leaf node of every triangle (-1: in no leaf), visiting rank of every triangle: depth first from node 0, children.y before children.x)."""
    b = np.asarray(scene["bvh"], F32).reshape(-1, 9)
    n_tri = np.asarray(scene["tri"]).size // 4
    leaf_of = np.full(n_tri, -1, np.int64)
    rank = np.full(n_tri, np.iinfo(np.int64).max, np.int64)
    forks, stack, r = [], [0] if len(b) else [], 0
    while stack:
        nd = stack.pop()
        if b[nd, 8] < 0:
            forks.append(nd)
            for c in (6, 7):  # children.x is pushed first: children.y is visited first
                if b[nd, c] >= 0:
                    stack.append(int(b[nd, c]))
        else:
            k = int(b[nd, 8])
            leaf_of[k], rank[k] = nd, r
            r += 1
    return b, forks, leaf_of, rank


def searched(rays):
    """Rays the query searches at all: every component finite, a direction other than zero, tmin < tmax (after the flush of denormals)."""
    r = ftz(np.asarray(rays, F32).reshape(-1, 8))
    return np.isfinite(r).all(1) & (r[:, 4:7] != 0).any(1) & (r[:, 3] < r[:, 7])


def _gmin(a, b):  # GLSL min as the query evaluates it: the other operand when one is NaN
    return np.where(b != b, a, np.where(a < b, a, b))


def _gmax(a, b):
    return np.where(b != b, a, np.where(a > b, a, b))


def reach(scene, rays, limit):
    """The slab test of every fork's own box (host/query.cpp; raytrace.frag:259-274, :298) in float32 with the statement's NaN rule, flushed inputs and
    results and the IEEE 1 / d, under the search limit `limit` (per ray).  Returns (reached (n, T): every ancestor fork of triangle k's leaf passes
    min(t1, limit) >= t0 -- with limit = tmax this is every leaf a search can visit, with a smaller limit a subset of it --, nan (n,): some reached fork
    has a NaN among its six slab products)."""
    b, forks, leaf_of, _ = tree(scene)
    r = ftz(np.asarray(rays, F32).reshape(-1, 8))
    n = len(r)
    o, d = r[:, 0:3], r[:, 4:7]
    lim = ftz(np.broadcast_to(np.asarray(limit, F32), (n,)))
    ok = np.zeros((max(len(b), 1), n), bool)
    ok[0] = searched(rays)
    nan = np.zeros(n, bool)
    with np.errstate(all="ignore"):
        inv = ftz(F32(1.0) / d)
        for nd in forks:
            box = ftz(b[nd, 0:6])
            f = ftz(ftz(box[None, 3:6] - o) * inv)
            g = ftz(ftz(box[None, 0:3] - o) * inv)
            t1 = _gmin(_gmax(f[:, 0], g[:, 0]), _gmin(_gmax(f[:, 1], g[:, 1]), _gmax(f[:, 2], g[:, 2])))
            t0 = _gmax(_gmin(f[:, 0], g[:, 0]), _gmax(_gmin(f[:, 1], g[:, 1]), _gmin(f[:, 2], g[:, 2])))
            here = ok[nd]
            nan |= here & (np.isnan(f) | np.isnan(g)).any(1)
            below = here & (_gmin(t1, lim) >= t0)
            for c in (6, 7):
                if b[nd, c] >= 0:
                    ok[int(b[nd, c])] = below
    reached = np.where(leaf_of[None, :] >= 0, ok[np.maximum(leaf_of, 0)].T, False)
    return reached, nan


def check_against_brute_force(scene, rays, res, bf, any_hit):
    """What a result of glrt_trace_rays must satisfy against the brute force and the restated slab tests, with no allowance for lost hits:
      1. check_real_hits;
      2. no reported hit is closer than the brute force's closest;
      3. every hit the brute force has below the reported t (any hit, where a miss was reported) lies behind a fork whose box fails the restated slab test
         under the reported t: a lost hit whose ancestors all pass is a traversal error;
      4. the reported triangle's own ancestors all pass under tmax (nothing is found in a subtree the search may not enter);
      5. order: among triangles hit at exactly the reported t whose ancestors pass under it, the reported one comes first in the visiting order; in
         any-hit mode, where the limit stays at tmax until the first hit, the result is exactly the first brute-force hit among the reachable leaves.
    Returns counts: rays, found, lost (rays on which the brute force has a closer hit, or a hit where a miss was reported -- all explained), ties."""
    hit, t = bf[0], bf[1]
    rt, rtri = np.asarray(res[0]), np.asarray(res[1])
    check_real_hits(scene, rays, res, bf)
    n = len(rays)
    big = np.iinfo(np.int64).max
    found = rtri >= 0
    idx = np.arange(n)
    rank = tree(scene)[3]
    reach_max, _ = reach(scene, rays, rays[:, 7])
    assert reach_max[idx[found], rtri[found]].all(), "a hit in a subtree whose box the ray misses"
    if any_hit:
        cand = hit & reach_max
        want = np.where(cand.any(1), np.where(cand, rank[None, :], big).argmin(1), -1)
        bad = np.nonzero(want != rtri)[0]
        assert bad.size == 0, (f"any hit: {bad.size} rays differ from the first reachable hit of the visiting order; first: ray {rays[bad[0]].tolist()} "
                               f"reported {rtri[bad[0]]}, expected {want[bad[0]]}")
        lost = hit.any(1) & ~found
        ties = np.zeros(n, bool)
    else:
        first = np.where(hit, t, np.inf).min(1)
        assert (rt[found] >= first[found]).all(), "a hit closer than the closest one"
        reach_rep, _ = reach(scene, rays, rt)
        closer = hit & (t < rt[:, None])  # (a miss reports tmax: every brute-force hit lies below it)
        unexplained = closer & reach_rep
        bad = np.nonzero(unexplained.any(1))[0]
        assert bad.size == 0, (f"{bad.size} rays lose a hit that no box explains; first: ray {rays[bad[0]].tolist()} reported t {float(rt[bad[0]])!r} "
                               f"tri {rtri[bad[0]]}; closer triangles whose ancestors all pass: {np.nonzero(unexplained[bad[0]])[0].tolist()}")
        lost = closer.any(1)
        tied = hit & (t == rt[:, None]) & reach_rep & found[:, None]
        tied[idx[found], rtri[found]] = False
        ties = tied.any(1)
        best = np.where(tied, rank[None, :], big).min(1)
        mine = np.where(found, rank[np.maximum(rtri, 0)], -1)
        bad = np.nonzero(ties & (best < mine))[0]
        assert bad.size == 0, (f"{bad.size} ties go to a triangle visited later; first: ray {rays[bad[0]].tolist()} reported {rtri[bad[0]]}")
    return dict(rays=n, found=int(found.sum()), lost=int(lost.sum()), ties=int(ties.sum()))


def shares(scene, rays, res, bf):
    """How hostile a set is (closest-hit result `res`): the shares of rays that are searched, that meet a NaN slab product in a fork they reach, whose hit
    lies on a triangle's edge (u == 0, v == 0 or inv * (U + V) == 1), and whose hit distance is shared by another reachable triangle."""
    rt, rtri = np.asarray(res[0]), np.asarray(res[1])
    n = max(len(rays), 1)
    _, nan = reach(scene, rays, rays[:, 7])
    found = rtri >= 0
    i, k = np.nonzero(found)[0], rtri[found]
    edge = (bf[2][i, k] == 0) | (bf[3][i, k] == 0) | (bf[4][i, k] == 1)
    reach_rep, _ = reach(scene, rays, rt)
    tied = bf[0] & (bf[1] == rt[:, None]) & reach_rep & found[:, None]
    tied[i, k] = False
    return dict(searched=searched(rays).sum() / n, nan=nan.sum() / n, edge=edge.sum() / n, tie=tied.any(1).sum() / n)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Hostile sets: what a picking / visibility / height-probe host sends, where a slab test and a triangle test go wrong


def _bounds(scene):
    p = _pos(scene)
    lo, hi = p.min(0), p.max(0)
    return lo, hi, np.maximum(hi - lo, F32(1e-3))


def _fork_boxes(scene):
    """Box bounds (lo, hi) of the tree's fork records, bit for bit; the scene's bounds when the tree has no fork."""
    b = np.asarray(scene["bvh"], F32).reshape(-1, 9)
    f = b[b[:, 8] < 0][:, 0:6]
    f = f[np.isfinite(f).all(1)]
    if len(f) == 0:
        lo, hi, _ = _bounds(scene)
        f = np.concatenate([lo, hi])[None]
    return f


def _edge_midpoints(scene):
    v0, v1, v2 = _tris(scene)
    h = F32(0.5)
    return np.concatenate([(v0 + v1) * h, (v1 + v2) * h, (v2 + v0) * h]).astype(F32)


def _outside(scene, n, rng):
    """Origins on shells around the scene, 1 .. 2 diagonals from its centre."""
    lo, hi, ext = _bounds(scene)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return ((lo + hi) * 0.5 + u * np.linalg.norm(ext) * rng.uniform(1.0, 2.0, (n, 1))).astype(F32)


def axial_rays(scene, n, seed=21, tmin=1e-4, tmax=1e8):
    """Directions +-e_x, +-e_y, +-e_z (zero slots +0, or -0), or with exactly one zero component; origins random in the bounds grown by half, or with the two
    coordinates across the ray copied from fork box bounds (the ray runs in a box's face plane: 0 * inf), or from a vertex / an edge's midpoint."""
    rng = np.random.default_rng(seed)
    lo, hi, ext = _bounds(scene)
    i = np.arange(n)
    kind, flavour = i % 3, (i // 3) % 3
    main = rng.integers(0, 3, n)
    other = (main + rng.integers(1, 3, n)) % 3
    d = np.zeros((n, 3), F32)
    d[kind == 1] = F32(-0.0)
    d[i, main] = rng.choice(np.array([-1.0, 1.0], F32), n)
    two = kind == 2
    d[i[two], other[two]] = (rng.uniform(0.1, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(F32)[two]
    neg = two & (rng.uniform(0, 1, n) < 0.5)
    d[i[neg], (3 - main - other)[neg]] = F32(-0.0)
    o = (lo - 0.5 * ext + rng.uniform(0, 1, (n, 3)) * 2.0 * ext).astype(F32)
    # the last two flavours start upstream of the scene (three in four), so that the ray crosses it
    up = (flavour > 0) & (rng.uniform(0, 1, n) < 0.75)
    start = np.where(d[i, main] > 0, lo[main] - ext[main] * rng.uniform(0.1, 0.5, n), hi[main] + ext[main] * rng.uniform(0.1, 0.5, n)).astype(F32)
    o[i[up], main[up]] = start[up]
    ta, tb = (main + 1) % 3, (main + 2) % 3
    boxes = _fork_boxes(scene)
    fk = rng.integers(0, len(boxes), n)
    side_a, side_b = 3 * rng.integers(0, 2, n), 3 * rng.integers(0, 2, n)
    f1 = flavour == 1
    o[i[f1], ta[f1]] = boxes[fk, ta + side_a][f1]
    o[i[f1], tb[f1]] = boxes[fk, tb + side_b][f1]
    pos = _pos(scene)
    pts = np.concatenate([pos, _edge_midpoints(scene)])
    pk = np.where(rng.uniform(0, 1, n) < 0.5, rng.integers(0, len(pos), n), rng.integers(0, len(pts), n))
    f2 = flavour == 2
    o[i[f2], ta[f2]] = pts[pk, ta][f2]
    o[i[f2], tb[f2]] = pts[pk, tb][f2]
    return pack(o, d, tmin, tmax)


def in_plane_rays(scene, n, seed=22, tmin=1e-4, tmax=1e8):
    """Half: oblique in two axes and zero in the third, the origin's coordinate on that axis a fork box bound (the ray lies in a box's face plane); half:
    from outside towards fork box corners (direction = the float32 difference)."""
    rng = np.random.default_rng(seed)
    lo, hi, ext = _bounds(scene)
    boxes = _fork_boxes(scene)
    i = np.arange(n)
    o = _outside(scene, n, rng)
    fk = rng.integers(0, len(boxes), n)
    corner = np.stack([boxes[fk, a + 3 * rng.integers(0, 2, n)] for a in range(3)], 1)
    target = (lo + rng.uniform(0, 1, (n, 3)) * ext).astype(F32)
    plane = i % 2 == 0
    target[~plane] = corner[~plane]
    axis = rng.integers(0, 3, n)
    o[i[plane], axis[plane]] = corner[i, axis][plane]
    d = (target - o).astype(F32)
    d[i[plane], axis[plane]] = np.where(rng.uniform(0, 1, n) < 0.5, F32(0.0), F32(-0.0))[plane]
    return pack(o, d, tmin, tmax)


def feature_rays(scene, n, seed=23, tmin=1e-4, tmax=1e8):
    """From outside towards vertices, edge midpoints and centroids (direction = the unnormalised float32 difference), and along the geometric normal through
    centroids: head-on hits, exact ties where the scene holds every triangle twice."""
    rng = np.random.default_rng(seed)
    _, _, ext = _bounds(scene)
    v0, v1, v2 = _tris(scene)
    cen = ((v0 + v1 + v2) / F32(3.0)).astype(F32)
    i = np.arange(n)
    share = i % 4
    o = _outside(scene, n, rng)
    pos, mid = _pos(scene), _edge_midpoints(scene)
    k = rng.integers(0, len(v0), n)
    target = np.where((share == 0)[:, None], pos[rng.integers(0, len(pos), n)], np.where((share == 1)[:, None], mid[rng.integers(0, len(mid), n)], cen[k]))
    d = (target - o).astype(F32)
    nrm = np.cross((v1 - v0)[k].astype(np.float64), (v2 - v0)[k].astype(np.float64))
    ln = np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm = np.where(ln > 0, nrm / np.maximum(ln, 1e-300), 0.0) * rng.choice([-1.0, 1.0], (n, 1))
    along = share == 3
    o[along] = (cen[k] + nrm * np.linalg.norm(ext) * rng.uniform(0.5, 2.0, (n, 1))).astype(F32)[along]
    d[along] = (-nrm).astype(F32)[along]
    return pack(o, d, tmin, tmax)


def range_edge_rays(scene, rays, t):
    """Eleven variants of every ray around its closest-hit distance t (from the CPU statement): tmax in {prev(t), t, next(t)}, tmin in {prev(t), t, next(t)},
    tmin in {-0.0, -1e30, 1e-42 (a denormal)}, tmax in {FLT_MAX, 1e-42}."""
    rays = np.asarray(rays, F32).reshape(-1, 8)
    t = np.asarray(t, F32)
    around = [np.nextafter(t, F32(-np.inf)), t, np.nextafter(t, F32(np.inf))]
    out = []
    for col, values in ((7, around), (3, around), (3, [F32(-0.0), F32(-1e30), F32(1e-42)]), (7, [FLT_MAX, F32(1e-42)])):
        for v in values:
            r = rays.copy()
            r[:, col] = v
            out.append(r)
    return np.concatenate(out)


SCALES = (13, -13, 40, -40, 100, -100, 140, -140)


def scaled_rays(rays, k):
    """The same rays with d * 2^k, tmin * 2^-k, tmax * 2^-k (float32: large |k| leaves denormal, zero or infinite components)."""
    r = np.asarray(rays, F32).reshape(-1, 8).copy()
    with np.errstate(all="ignore"):
        r[:, 4:7] = np.ldexp(r[:, 4:7], k)
        r[:, 3] = np.ldexp(r[:, 3], -k)
        r[:, 7] = np.ldexp(r[:, 7], -k)
    return r


def dead_rays(scene, n, seed=24):
    """Rays that never become active in the device's kernel: those that need no search (special_rays) and rays whose line passes the scene at a diagonal's
    distance or more (they miss the root box; a box BEHIND the origin would pass the slab test, as in the reference)."""
    rng = np.random.default_rng(seed)
    lo, hi, _ = _bounds(scene)
    o = _outside(scene, n, rng)
    out = pack(o, np.cross(o - (lo + hi) * F32(0.5), rng.normal(size=(n, 3))).astype(F32), 1e-4, 1e8)
    sp = special_rays()
    out[::3] = sp[np.arange(len(out[::3])) % len(sp)]
    return out


def lane_patterns():
    """name -> bool mask over a batch (True: a searched ray, False: a dead one), chunk by chunk of 64 lanes: what the refill of the device's kernel
    (csrc/query.hip.h: trace_tree, kRefillMin = 16) never sees in a homogeneous batch."""
    lane = np.arange(CHUNK)
    full, none = np.ones(CHUNK, bool), np.zeros(CHUNK, bool)
    p = {"alternate": np.tile(lane % 2 == 0, 8), "dead_chunks_between": np.concatenate([full, none, none, full, none, full, full, none, full])}
    for k in (0, 31, 63):
        p[f"one_live_lane{k}"] = np.tile(lane == k, 6)
    for k in (15, 16, 17):
        p[f"dead{k}_start"] = np.tile(lane >= k, 5)
        p[f"dead{k}_end"] = np.tile(lane < CHUNK - k, 5)
        m = full.copy()
        m[(np.arange(k) * 37 + 5) % CHUNK] = False
        p[f"dead{k}_scattered"] = np.tile(m, 5)
    for tail in (1, 15, 16, 17, 63):  # a partial last chunk
        for kind, m in (("dead", np.zeros(tail, bool)), ("live", np.ones(tail, bool)), ("mixed", np.arange(tail) % 3 == 0)):
            p[f"tail{tail}_{kind}"] = np.concatenate([full, lane % 2 == 0, m])
    for chunks in (3, 4, 5, 11, 12, 13):  # below, at and above four chunks (one per wave) per 256-thread workgroup, for one and for several workgroups
        p[f"chunks{chunks}"] = np.tile(lane % 5 != 0, chunks)
    return p


def interleave(live, dead, pattern):
    """One batch from a pool of searched rays and a pool of dead ones (both cycled), by a mask over the batch (True: the next live ray) or the name of one
    of lane_patterns()."""
    mask = lane_patterns()[pattern] if isinstance(pattern, str) else np.asarray(pattern, bool)
    out = np.zeros((len(mask), 8), F32)
    out[mask] = live[np.arange(int(mask.sum())) % len(live)]
    out[~mask] = dead[np.arange(int((~mask).sum())) % len(dead)]
    return out


def hostile_sets(scene, n=240):
    """name -> rays: every hostile set on one scene (range_edge around the CPU statement's closest hits; scaled at every exponent of SCALES)."""
    from glrt_amd import host
    sets = {"axial": axial_rays(scene, n), "in_plane": in_plane_rays(scene, n), "feature": feature_rays(scene, n)}
    pool = np.concatenate([sets["feature"], sets["axial"], sets["in_plane"]])
    t, tri, _, _ = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], pool)
    hit = np.nonzero(tri >= 0)[0][:max(n // 4, 1)]
    sets["range_edge"] = range_edge_rays(scene, pool[hit], t[hit])
    base = np.concatenate([s[:n // 12] for s in (sets["feature"], sets["axial"], sets["in_plane"])])
    sets["scaled"] = np.concatenate([scaled_rays(base, k) for k in SCALES])
    return sets
