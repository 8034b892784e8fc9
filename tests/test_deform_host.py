"""The deform pass's CPU statement (libglrt_host.so: glrt_deform_vertices) without a GPU: against its numpy statement (tests/deform_math.py) bit for bit on
hostile cases, the consequences the contract draws (include/glrtx.h "Deforming": no active target is Posing; an inactive target is not read; a negated bone
changes nothing), what dual quaternions are for (a twist keeps its radius where linear blending loses it), and glrt_dualquat_from_matrix against the rigid
transform it stands for."""
import ctypes as C

import numpy as np
import pytest

import deform_math as dm
import skin_math as sm
from glrt_amd import host, rig
from test_skin_host import BONES, SIZES

TARGETS = [0, 1, 3, 64]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _seed(n_vert, n_bones):
    return 1000 * n_vert + n_bones


def _assert_same(got, ref, what):
    bad = _bits(got) != _bits(ref)
    assert not bad.any(), (f"{what}: {int(bad.any(1).sum())} vertices differ; first {np.argwhere(bad)[0].tolist()}: "
                           f"{got[tuple(np.argwhere(bad)[0])]!r} vs {ref[tuple(np.argwhere(bad)[0])]!r}")


GRID = [(n, nb, mode) for n in SIZES for nb in BONES for mode in (0, 1)]


@pytest.mark.parametrize("n_vert,n_bones,mode", GRID, ids=[f"{n}v{b}b-{'dq' if m else 'mat'}" for n, b, m in GRID])
def test_equals_numpy_on_hostile_cases(n_vert, n_bones, mode):
    for n_targets in TARGETS:
        rest, bones, weights, data, deltas, mw = dm.hostile_case(n_vert, n_bones, mode, n_targets, _seed(n_vert, n_bones))
        got = host.deform_vertices(rest, bones, weights, data, mode, deltas, mw)
        _assert_same(got, dm.deform(rest, bones, weights, data, mode, deltas, mw), f"{n_targets} targets")
        moved = [0, 1, 2, 3, 4, 5, 9, 10, 11, 12, 13, 14]
        nan = np.isnan(got[:, moved])
        assert (_bits(got[:, moved])[nan] == 0x7FC00000).all()  # a stored NaN is canonical
        assert (_bits(got[:, 6:9]) == _bits(rest[:, 6:9])).all()  # uv: the words, whatever they are


def test_the_hostile_cases_are_hostile():
    """What the grid claims to cover is in it: unit, non-unit, all-zero and 1e20 dual quaternions; antipodal pairs on one vertex; pairs with h exactly 0 and with
    h < 0; both arms of the dual quaternion's l > 0; zero, +-denormal, negative and above-one morph weights; an inactive target full of NaN and Inf."""
    n, nb = 1000, 300
    rest, bones, weights, q, deltas, mw = dm.hostile_case(n, nb, 1, 64, _seed(n, nb))
    norm = np.linalg.norm(q[:, 0:4].astype(np.float64), axis=1)
    assert (np.abs(norm - 1) < 1e-6).any() and ((norm > 1.2) & (norm < 10)).any() and (norm == 0).any() and (norm > 1e19).any()
    pair = (_bits(q[bones[:, 0]]) == _bits(np.negative(q[bones[:, 1]]))).all(1) & (norm[bones[:, 0]] > 0)
    assert pair.sum() >= n // 10
    s, h = dm.signs(bones, weights, q)
    assert (h == 0).any() and (h < 0).any() and (h > 0).any() and np.isnan(h).any()
    assert ((h[:, 1] == 0) & (norm[bones[:, 0]] == 1) & (norm[bones[:, 2]] == 1)).any()  # two unit rotations at right angles in the 4-space: h exactly 0
    flipped = _bits(s) != _bits(weights)
    assert flipped[:, 1:].any() and not flipped[:, 0].any()
    B = dm.dualquat_matrix(bones, weights, q)
    assert np.isfinite(B).all((1, 2)).any()
    zero_blend = (q[bones] == 0).all((1, 2))
    assert zero_blend.any()  # l == 0: the entries stay as they are, L is the identity
    assert (B[zero_blend][:, :, :3] == np.eye(3, dtype=np.float32)).all()
    tiny = (np.abs(mw) < np.float32(2.0 ** -126))
    assert (mw == 0).any() and (tiny & (mw > 0)).any() and (tiny & (mw < 0)).any() and (mw < -0.5).any() and (mw > 1).any()
    assert np.isnan(deltas[tiny]).any() and np.isinf(deltas[tiny]).any()
    live = deltas[~tiny]
    assert np.isnan(live).any() and np.isinf(live).any() and ((np.abs(live) < np.float32(2.0 ** -126)) & (live != 0)).any()
    assert dm.active_targets(mw) == [int(k) for k in np.flatnonzero(~tiny)]


@pytest.mark.parametrize("n_vert,n_bones", [(n, nb) for n in SIZES for nb in BONES], ids=[f"{n}v{b}b" for n in SIZES for b in BONES])
def test_matrices_without_targets_are_posing(n_vert, n_bones):
    rest, bones, weights, mats = sm.hostile_rig(n_vert, n_bones, _seed(n_vert, n_bones))
    _assert_same(host.deform_vertices(rest, bones, weights, mats, 0), host.skin_vertices(rest, bones, weights, mats), "mode 0, no targets")


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("n_targets", [1, 3, 64])
def test_inactive_targets_are_not_read(mode, n_targets):
    """Every weight a zero or a denormal, every delta NaN or Inf (0 * NaN would be NaN): the output of no targets at all, bit for bit."""
    n, nb = 257, 5
    rest, bones, weights, data, _, _ = dm.hostile_case(n, nb, mode, 0, _seed(n, nb))
    deltas = np.full((n_targets, n, 6), np.nan, np.float32)
    deltas[:, ::3] = np.inf
    deltas[:, 1::3] = -1e30
    mw = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-45], np.float32)[np.arange(n_targets) % 5]
    _assert_same(host.deform_vertices(rest, bones, weights, data, mode, deltas, mw), host.deform_vertices(rest, bones, weights, data, mode), "all inactive")
    _assert_same(dm.deform(rest, bones, weights, data, mode, deltas, mw), dm.deform(rest, bones, weights, data, mode), "all inactive, numpy")


def _ring():
    """64 vertices on the unit circle at z = 0.5 with radial normals, each hung on two bones with {0.5, 0.5}: the mid ring of a joint."""
    th = np.arange(64) * (2 * np.pi / 64)
    rest = np.zeros((64, 15), np.float32)
    rest[:, 0], rest[:, 1], rest[:, 2] = np.cos(th), np.sin(th), 0.5
    rest[:, 3], rest[:, 4] = np.cos(th), np.sin(th)
    bones = np.tile(np.array([0, 1, 0, 0], np.int32), (64, 1))
    weights = np.tile(np.array([0.5, 0.5, 0.0, 0.0], np.float32), (64, 1))
    half_turn = np.array([-1, 0, 0, 0, 0, -1, 0, 0, 0, 0, 1, 0], np.float32)  # 180 degrees about z
    return rest, bones, weights, np.stack([rig.IDENTITY, half_turn])


TWIST_BOUND = 2 * 1.18e-7


def test_a_twist_keeps_its_radius():
    """Bones: the identity and a half turn about z.  Linear blending puts every vertex of the ring on the axis, radius exactly 0; the dual-quaternion form turns
    the ring by a quarter and keeps it a ring.  tests/deform_math.py gives max |radius - 1| = 1.18e-7 on this input and keeps z exactly (L22 = 1 - 2 (0 + 0));
    the bound is twice that."""
    rest, bones, weights, mats = _ring()
    lbs = host.deform_vertices(rest, bones, weights, mats, 0)
    assert (np.hypot(lbs[:, 0], lbs[:, 1]) == 0).all() and (lbs[:, 2] == 0.5).all()
    dq = rig.dualquat(mats)
    assert dq.tolist() == [[0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0]]
    out = host.deform_vertices(rest, bones, weights, dq, 1)
    _assert_same(out, dm.deform(rest, bones, weights, dq, 1), "ring")
    radius = np.hypot(out[:, 0].astype(np.float64), out[:, 1].astype(np.float64))
    print(f"max |radius - 1| = {np.abs(radius - 1).max():.3e}, max |z - 0.5| = {np.abs(out[:, 2] - 0.5).max():.3e}")
    assert np.abs(radius - 1).max() <= TWIST_BOUND
    assert np.abs(out[:, 2].astype(np.float64) - 0.5).max() <= TWIST_BOUND
    # a quarter turn: (x, y) -> (-y, x)
    assert np.abs(out[:, 0] + rest[:, 1]).max() <= 2 * TWIST_BOUND and np.abs(out[:, 1] - rest[:, 0]).max() <= 2 * TWIST_BOUND
    n = out[:, 3:6].astype(np.float64)
    assert np.abs(np.linalg.norm(n, axis=1) - 1).max() < 1e-6 and np.abs(n[:, 2]).max() < 1e-6


def _rotations(n, rng):
    A = rng.standard_normal((n, 3, 3))
    R = np.linalg.qr(A)[0]
    return R * np.sign(np.linalg.det(R))[:, None, None]


def _unit_rig(n_vert, n_bones, seed):
    """Ordinary vertices, four distinct-ish bones a vertex with convex weights, unit dual quaternions of random rigid motions."""
    rng = np.random.default_rng(seed)
    rest = rng.standard_normal((n_vert, 15)).astype(np.float32)
    bones = rng.integers(0, n_bones, (n_vert, 4)).astype(np.int32)
    w = rng.random((n_vert, 4))
    weights = (w / w.sum(1, keepdims=True)).astype(np.float32)
    M = np.concatenate([_rotations(n_bones, rng), rng.standard_normal((n_bones, 3, 1))], 2).astype(np.float32)
    return rest, bones, weights, rig.dualquat(M)


def test_negating_a_bone_changes_nothing():
    """q and -q are the same rigid motion, and the sign step makes the statement see them as the same: negating all eight floats of any subset of bones changes
    no output bit -- unless an h is exactly 0, where h < 0 cannot tell the two apart; the rig is asserted to have none (min |h| 6.5e-4 here)."""
    n, nb = 20000, 50
    rest, bones, weights, q = _unit_rig(n, nb, 5)
    _, h = dm.signs(bones, weights, q)
    print(f"min |h| = {np.abs(h).min():.3e}")
    assert np.abs(h).min() > 0
    ref = host.deform_vertices(rest, bones, weights, q, 1)
    rng = np.random.default_rng(6)
    for subset in (np.arange(nb) % 2 == 0, rng.random(nb) < 0.5, np.ones(nb, bool), np.arange(nb) == 7):
        q2 = np.where(subset[:, None], np.negative(q), q)
        _assert_same(host.deform_vertices(rest, bones, weights, q2, 1), ref, f"{int(subset.sum())} bones negated")
    _assert_same(dm.deform(rest[:500], bones[:500], weights[:500], np.negative(q), 1), ref[:500], "numpy, all negated")


RIGID_K_MEASURED = 4.65  # max of err / (2^-24 (|p| + |t|)) that tests/deform_math.py shows on _rigid_input()
RIGID_K = 2 * RIGID_K_MEASURED


def _rigid_input():
    rng = np.random.default_rng(2024)
    nb, per = 50, 400
    R = _rotations(nb, rng)
    t = rng.standard_normal((nb, 3)) * 3
    rest = (rng.standard_normal((nb * per, 15)) * 2).astype(np.float32)
    obj = np.repeat(np.arange(nb), per).astype(np.int32)
    return rest, obj, R, t, np.concatenate([R, t[:, :, None]], 2).astype(np.float32).reshape(nb, 12)


def test_a_one_bone_dualquat_pose_is_the_rigid_transform():
    """50 random rotations with translations, 400 vertices each: glrt_dualquat_from_matrix of the float32 matrix, then the dual-quaternion statement, against
    R p + t in float64.  |error| <= k 2^-24 (|p| + |t|), k = 2 x 4.65 (the numpy statement's own maximum on this input, measured and doubled)."""
    rest, obj, R, t, M = _rigid_input()
    bones, weights = rig.rigid(obj)
    q = rig.dualquat(M)
    assert q.shape == (50, 8) and (q[:, 3] >= 0).all()
    assert np.abs(np.linalg.norm(q[:, 0:4].astype(np.float64), axis=1) - 1).max() < 1e-7
    assert np.abs(np.einsum("nk,nk->n", q[:, 0:4].astype(np.float64), q[:, 4:8].astype(np.float64))).max() < 1e-6  # r . d = 0: a rigid motion
    p = rest[:, 0:3].astype(np.float64)
    want = np.einsum("nij,nj->ni", R[obj], p) + t[obj]
    scale = 2.0 ** -24 * (np.linalg.norm(p, axis=1) + np.linalg.norm(t[obj], axis=1))
    for name, out in (("numpy", dm.deform(rest, bones, weights, q, 1)), ("cpu", host.deform_vertices(rest, bones, weights, q, 1))):
        k = np.linalg.norm(out[:, 0:3].astype(np.float64) - want, axis=1) / scale
        print(f"{name}: max k = {k.max():.3f}")
        assert k.max() <= RIGID_K, name
    # and the helper alone: identity, sign, a pure translation
    assert rig.identity_dualquats(3).tolist() == [[0, 0, 0, 1, 0, 0, 0, 0]] * 3
    assert host.dualquat_from_matrix(rig.IDENTITY).tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    assert host.dualquat_from_matrix([1, 0, 0, 2, 0, 1, 0, 4, 0, 0, 1, -6]).tolist() == [0, 0, 0, 1, 1, 2, -3, 0]
    turn = host.dualquat_from_matrix([-1, 0, 0, 0, 0, 1, 0, 0, 0, 0, -1, 0])  # a half turn about y: r.w == 0, either sign would do; y comes out positive
    assert turn[0:4].tolist() == [0, 1, 0, 0]


def test_refusals():
    rest, bones, weights, mats, deltas, mw = dm.hostile_case(10, 3, 0, 3, 1)
    for bad in (np.where(bones == 2, 3, bones), np.where(bones == 0, -1, bones)):
        with pytest.raises(RuntimeError):
            host.deform_vertices(rest, bad, weights, mats, 0, deltas, mw)
    for v in (np.nan, np.inf, -np.inf):
        w2 = mw.copy(); w2[1] = v
        with pytest.raises(RuntimeError):
            host.deform_vertices(rest, bones, weights, mats, 0, deltas, w2)
    L = host.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = bones.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros_like(rest)
    big = np.zeros(65, np.float32)
    call = L.glrt_deform_vertices
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(mw), 3, fp(out)) == 0
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, None, None, 0, fp(out)) == 0
    assert call(None, 10, ip, fp(weights), fp(mats), 3, 0, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, None, fp(weights), fp(mats), 3, 0, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, ip, None, fp(mats), 3, 0, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), None, 3, 0, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, None, None, 0, None) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 0, 0, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 65537, 0, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 2, None, None, 0, fp(out)) == -1  # mode
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, -1, None, None, 0, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(big), 65, fp(out)) == -1  # more than GLRT_MAX_MORPH_TARGETS
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(mw), -1, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, None, fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), None, 3, fp(out)) == -1
