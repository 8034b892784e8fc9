"""The compact node array (glrtx.hip: pack_compact): 48-byte records at breadth-first positions, children of the fork of rank k
at positions 2k + 1 / 2k + 2, a rank table per 32 positions.  Host only: it must hold exactly the tree of the 64-byte array -- the same boxes, the
same triangle records, the same chaining -- so that a traversal of either visits the same records in the same order.  Checked two ways: a
structural walk that pairs every 64-byte ref with its position, and a ray walk (the step's slab and triangle tests restated in float32) over
both layouts.  Also the launch rule: the rank table's LDS against four workgroups per CU."""
import numpy as np
import pytest

from glrt_amd import device, scenes

REF_FIN = np.int32(-2**31)


def _i(x):
    return int(np.float32(x).view(np.int32))


class Old:
    """The 64-byte layout: fork records (glrtx_debug_pack_forks) and leaf records by id."""

    def __init__(self, sc):
        from test_host import _pack
        rc, self.forks, self.root, self.stack = _pack(sc)
        assert rc == 0
        _, _, self.leaves = device.pack_compact(sc)
        self.refs = self.forks.view(np.int32)[:, [3, 7]] if len(self.forks) else np.zeros((0, 2), np.int32)

    def is_fork(self, ref):
        return ref >= 0

    def fork(self, ref):  # (lo L, hi L, lo R, hi R), (ref L, ref R)
        f = self.forks[ref]
        return (f[0:3], f[4:7], f[8:11], f[12:15]), (int(self.refs[ref, 0]), int(self.refs[ref, 1]))

    def leaf(self, ref):  # (v0, e1, e2, id, next)
        idx = ~ref
        r = self.leaves[idx]
        return r[0:3], r[4:7], r[8:11], idx, _i(r[7])


class Compact:
    def __init__(self, sc):
        self.recs, self.ranks, _ = device.pack_compact(sc)
        self.root = 0

    def is_fork(self, p):
        return (int(self.ranks[p >> 5, 0]) >> (p & 31)) & 1 == 1

    def rank(self, p):
        bits = int(self.ranks[p >> 5, 0]) & ((1 << (p & 31)) - 1)
        return int(self.ranks[p >> 5, 1]) + bin(bits).count("1")

    def fork(self, p):
        r = self.recs[p]
        k = self.rank(p)
        return (r[0:3], r[4:7], r[8:11], np.array([r[3], r[7], r[11]], np.float32)), (2 * k + 1, 2 * k + 2)

    def leaf(self, p):
        r = self.recs[p]
        return r[0:3], r[4:7], r[8:11], _i(r[3]), _i(r[7])


def _scene(kind, n=600):
    if kind == "two_triangles":
        return scenes.config_c3(16, 16, n=2, bvh="sah")[0]
    if kind == "one_triangle":
        return scenes.config_c3(16, 16, n=1, bvh="sah")[0]
    if kind in ("one_child", "one_child_chains"):
        from test_host import _with_one_child_forks
        sc, _ = scenes.config_c1(16, 16, subdiv=1)
        return _with_one_child_forks(sc, 24, 5, chain=1 if kind == "one_child" else 3)
    if kind == "comb":  # a chain of forks: every leaf pushed, stack depth n - 1
        sc, _ = scenes.config_c3(16, 16, n=63, bvh="chain")
        nodes = sc["bvh"].reshape(-1, 9).copy()
        fk = nodes[:, 8] < 0
        nodes[fk, 6], nodes[fk, 7] = nodes[fk, 7].copy(), nodes[fk, 6].copy()
        return dict(sc, bvh=nodes.reshape(-1, 3))
    if kind == "leaf_pairs":  # a full tree whose bottom level is all leaf pairs
        return scenes.config_c3(16, 16, n=256, bvh="lbvh")[0]
    if kind == "headline":
        return scenes.config_headline(16, 16)[0]
    sc, _ = scenes.config_c1(16, 16, subdiv=2)
    return scenes.rebuild_bvh(sc, kind)


KINDS = ["sah", "lbvh", "sahl", "reference", "sah-reinsert", "two_triangles", "one_triangle", "one_child", "one_child_chains", "comb", "leaf_pairs", "headline"]


@pytest.mark.parametrize("kind", KINDS)
def test_compact_array_holds_the_same_tree(kind):
    sc = _scene(kind)
    old, new = Old(sc), Compact(sc)
    n_pos = new.recs.shape[0]
    assert new.ranks.shape[0] == (n_pos + 31) // 32
    seen = set()
    todo = [(old.root, 0)]
    while todo:
        r, p = todo.pop()
        assert 0 <= p < n_pos and p not in seen
        seen.add(p)
        assert old.is_fork(r) == new.is_fork(p), (r, p)
        if old.is_fork(r):
            bo, (l, rr) = old.fork(r)
            bn, (pl, pr) = new.fork(p)
            for a, b in zip(bo, bn):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            todo += [(l, pl), (rr, pr)]
        else:
            *to, ido, nxo = old.leaf(r)
            *tn, idn, nxn = new.leaf(p)
            for a, b in zip(to, tn):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            assert ido == idn
            assert (nxo == REF_FIN) == (nxn == REF_FIN)
            if nxo != REF_FIN:
                todo.append((nxo, nxn))
    assert len(seen) == n_pos  # every position is reachable: nothing but the tree
    forks = sum(new.is_fork(p) for p in range(n_pos))
    assert forks == len(old.forks) and int(new.ranks[-1, 1]) + bin(int(new.ranks[-1, 0])).count("1") == forks


def _walk(L, ray, root_box):
    """The step's state machine (pt_kernel.hip.h: trav_step) in float32: returns the records visited (fork: its boxes' bits, leaf: its id) and the hit."""
    f = np.float32
    o, d = ray
    inv = (f(1.0) / d).astype(np.float32)
    th, tri, vis = f(1e8), 0, []

    def box(lo, hi):
        a = (lo - o) * inv
        b = (hi - o) * inv
        t1 = np.min(np.maximum(a, b))
        t0 = np.max(np.minimum(a, b))
        return bool(min(t1, th) >= t0), t0

    if root_box is not None and not box(*root_box)[0]:
        return vis, tri
    cur, stack = L.root, []
    while True:
        pop = True
        if L.is_fork(cur):
            bxs, (l, r) = L.fork(cur)
            vis.append(("f", b"".join(x.tobytes() for x in bxs)))
            bl, t0l = box(bxs[0], bxs[1])
            br, _ = box(bxs[2], bxs[3])
            if bl and br:
                stack.append((t0l, l))
            cur = r if br else l
            pop = not (bl or br)
        else:
            v0, e1, e2, tid, nxt = L.leaf(cur)
            vis.append(("l", tid))
            t = o - v0
            p = np.cross(d, e2).astype(np.float32)
            det = f(f(e1[2] * p[2] + e1[1] * p[1]) + e1[0] * p[0])
            if abs(det) >= f(1e-4):
                ia = f(1.0) / det
                u = f(f(f(t[2] * p[2] + t[1] * p[1]) + t[0] * p[0]) * ia)
                q = np.cross(t, e1).astype(np.float32)
                v = f(f(f(d[2] * q[2] + d[1] * q[1]) + d[0] * q[0]) * ia)
                tt = f(f(f(e2[2] * q[2] + e2[1] * q[1]) + e2[0] * q[0]) * ia)
                if 0 <= u <= 1 and v >= 0 and u + v <= 1 and tt > f(1e-4) and tt < th:
                    th, tri = tt, tid
            cur = nxt
            pop = nxt == REF_FIN
        if pop:
            cur = None
            while stack:
                t0, ref = stack.pop()
                if not t0 > th:
                    cur = ref
                    break
            if cur is None:
                return vis, tri


@pytest.mark.parametrize("kind", ["sah", "lbvh", "reference", "one_child_chains", "comb", "two_triangles"])
def test_rays_visit_the_same_records_in_both_layouts(kind):
    sc = _scene(kind)
    old, new = Old(sc), Compact(sc)
    v = sc["vert"].reshape(-1, 15)[:, 0:3]
    lo, hi = v.min(0), v.max(0)
    b = sc["bvh"].reshape(-1, 9)
    root_box = (b[0, 0:3], b[0, 3:6]) if len(b) and b[0, 8] < 0 else None
    rng = np.random.default_rng(7)
    hits = 0
    with np.errstate(all="ignore"):
        for _ in range(150):
            o = (lo + (hi - lo) * rng.uniform(-0.3, 1.3, 3)).astype(np.float32)
            tgt = (lo + (hi - lo) * rng.uniform(0, 1, 3)).astype(np.float32)
            d = (tgt - o).astype(np.float32)
            d /= np.float32(np.linalg.norm(d))
            va, ta = _walk(old, (o, d), root_box)
            vb, tb = _walk(new, (o, d), root_box)
            assert va == vb and ta == tb
            hits += ta != 0
    assert kind in ("two_triangles", "comb") or hits > 0  # (small random triangles: rays rarely hit them)


def test_positions_are_the_forks_children_the_root_and_the_chained_leaves():
    """Also the deepest tree the upload takes (a comb of 64 triangles: 63 stack entries)."""
    for kind in ("comb", "sah", "one_child"):
        recs, ranks, _ = device.pack_compact(_scene(kind))
        forks = sum(bin(int(w)).count("1") for w in ranks[:, 0])
        tail = sum(1 for p in range(len(recs)) if not (int(ranks[p >> 5, 0]) >> (p & 31)) & 1 and _i(recs[p, 7]) != REF_FIN)
        assert len(recs) == 2 * forks + 1 + tail, kind
    from test_host import _pack
    assert _pack(_scene("comb"))[0] == 0


def _lds_base(stack_entries, n_mat, n_light):
    """launch_wgwf's LDS per workgroup without the rank table: head (materials, lights) | stacks | ctl | root box | camera | seeds | light-test bits."""
    head = 3 * n_mat * 16 if n_mat <= 256 else 0
    head += 6 * n_light * 16 if 0 < n_light <= 64 else 0
    return head + 2 * stack_entries * 256 * 4 + 32 * 4 + 2 * 16 + 36 * 4 + 64 * 8 + 4096 // 8


def test_headline_rank_table_fits_with_four_workgroups_and_config5_does_not():
    sc, _ = scenes.config_headline(16, 16)
    from test_host import _pack
    se = _pack(sc)[3]
    recs, ranks, _ = device.pack_compact(sc)
    n_mat, n_light = sc["mat"].size // 18, sc["light"].size // 4
    lds = _lds_base(se, n_mat, n_light) + 8 * ranks.shape[0]
    assert 4 * lds <= 160 * 1024, (lds, recs.shape[0])
    sc5, _ = scenes.config_c5(16, 16)
    se5 = _pack(sc5)[3]
    _, ranks5, _ = device.pack_compact(sc5)
    assert 4 * (_lds_base(se5, sc5["mat"].size // 18, sc5["light"].size // 4) + 8 * ranks5.shape[0]) > 160 * 1024
