"""The CPU statements of firefly re-weighting (libglrt_host.so: glrt_fold_cascades, glrt_reweight) against their numpy statements (tests/reweight_math.py),
bit for bit, and the three consequences of the contract (include/glrtx.h "Firefly re-weighting"): samples at or below `start` make C_0 the accumulator's own
chain and the resolve the plain mean; a lone bright sample is dropped where its neighbourhood holds nothing at its level; a finite C with integer counts
resolves to a finite image."""
import numpy as np
import pytest

import reweight_math as rw
from glrt_amd import host

SIZES = [(37, 61), (16, 16), (17, 33), (5, 130), (1, 1), (70, 49)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_but_nan_payloads(got, ref):
    """Fold outputs: a NaN must be a NaN in both, every other value the same bits."""
    gn, rn = np.isnan(got), np.isnan(ref)
    return np.array_equal(gn, rn) and np.array_equal(_bits(got)[~gn], _bits(ref)[~rn])


def test_hostile_samples_hold_what_they_promise():
    v = rw.hostile_samples(6, 37, 61, 3)
    l = rw.lum(v[..., 0], v[..., 1], v[..., 2])
    for bk in rw.bounds(1.0):
        for t in (np.nextafter(bk, np.float32(0)), bk, np.nextafter(bk, np.float32(np.inf))):
            assert (l == t).any(), (bk, t)
    f = v[..., :3]
    assert (l == 0).any() and (l < 0).any() and np.isnan(l).any() and np.isposinf(l).any() and (l > 1e29).any()
    assert ((f != 0) & (np.abs(f) < 2.0 ** -126)).any()
    C = rw.hostile_cascades(37, 61, 4)
    w = C[..., 3]
    assert (w == 0).any() and ((w != 0) & (np.abs(w) < 2.0 ** -126)).any() and np.isnan(w).any() and (w != np.floor(w))[np.isfinite(w)].any()


@pytest.mark.parametrize("rows,width", SIZES)
def test_fold_statements_agree_on_hostile_samples(rows, width):
    for start in (1.0, 0.375, 2.0 ** -20, 2.0 ** 20):
        v = rw.hostile_samples(5, rows, width, rows * 1000 + width, start)
        C0 = rw.hostile_cascades(rows, width, rows * 7 + width)
        acc0 = C0[0] + C0[1]
        for C_in, acc_in in ((np.zeros_like(C0), np.zeros_like(acc0)), (C0, acc0)):
            gc, ga = host.fold_cascades(C_in, v, accum=acc_in, start=start)
            rc, ra = rw.fold_cascades(C_in, acc_in, v, start)
            assert _same_but_nan_payloads(gc, rc), f"C {width}x{rows} start {start}"
            assert _same_but_nan_payloads(ga, ra), f"accumulator {width}x{rows} start {start}"
            assert _same_but_nan_payloads(host.fold_cascades(C_in, v, start=start), rc)


@pytest.mark.parametrize("rows,width", SIZES)
def test_resolve_statements_agree_on_hostile_planes(rows, width):
    v = rw.hostile_samples(4, rows, width, rows * 1000 + width + 1)
    planes = [rw.hostile_cascades(rows, width, rows * 1000 + width), host.fold_cascades(None, v),
              host.fold_cascades(rw.hostile_cascades(rows, width, rows * 31 + width), v)]
    for C in planes:
        for kappa in (4.0, 1.0, 16.0, 0.3, 1e-38, 3e38):
            got, ref = host.reweight(C, kappa), rw.reweight(C, kappa)
            bad = _bits(got) != _bits(ref)
            assert not bad.any(), f"{width}x{rows} kappa {kappa}: {int(bad.any(-1).sum())} pixels differ; first {np.argwhere(bad)[0].tolist()}"
            assert (got[..., 3] == 1).all()
            n = rw.counts_above(C)[0]
            dead = rw.tiny(n) | np.isnan(n)
            assert not got[dead][:, :3].any()


def test_refusals():
    lib = host.lib()
    C = np.zeros((6, 2, 2, 4), np.float32)
    out = np.zeros((2, 2, 4), np.float32)
    v = np.zeros((1, 2, 2, 4), np.float32)
    fp = host._fp
    for kappa in (0.0, -1.0, np.nan, np.inf):
        assert lib.glrt_reweight(fp(C), 2, 2, kappa, fp(out)) != 0, kappa
    for start in (0.0, np.nan, np.inf, 2.0 ** -21, 2.0 ** 21, -1.0):
        assert lib.glrt_fold_cascades(fp(C), None, fp(v), 1, 2, 2, start) != 0, start
    assert lib.glrt_reweight(None, 2, 2, 4.0, fp(out)) != 0 and lib.glrt_reweight(fp(C), 2, 2, 4.0, None) != 0
    assert lib.glrt_reweight(fp(C), 0, 2, 4.0, fp(out)) != 0 and lib.glrt_reweight(fp(C), 2, 65537, 4.0, fp(out)) != 0
    assert lib.glrt_fold_cascades(None, None, fp(v), 1, 2, 2, 1.0) != 0 and lib.glrt_fold_cascades(fp(C), None, None, 1, 2, 2, 1.0) != 0
    assert lib.glrt_fold_cascades(fp(C), None, fp(v), -1, 2, 2, 1.0) != 0
    assert lib.glrt_fold_cascades(fp(C), None, None, 0, 2, 2, 1.0) == 0 and not C.any()


def test_consequence_1_dim_samples_resolve_to_the_plain_mean():
    rng = np.random.default_rng(11)
    for start in (1.0, 2.0 ** 20):
        v = np.zeros((7, 19, 23, 4), np.float32)
        v[..., :3] = (rng.random((7, 19, 23, 3)) * start * 0.99).astype(np.float32)  # lum <= 0.99 * start * (0.2126 + 0.7152 + 0.0722)
        v[..., 3] = 1
        v[0, 0, 0, :3] = (start, start, start) if rw.lum(np.float32(start), np.float32(start), np.float32(start)) <= start else 0
        v[1, 1, 1, :3] = (-2.0, 0.5, -0.0)
        v[2, 2, 2, :3] = 1e-40
        assert (rw.lum(v[..., 0], v[..., 1], v[..., 2]) <= np.float32(start)).all()
        for fold, resolve in ((lambda: host.fold_cascades(None, v, accum=np.zeros_like(v[0]), start=start), host.reweight),
                              (lambda: rw.fold_cascades(np.zeros((6,) + v.shape[1:], np.float32), np.zeros_like(v[0]), v, start), rw.reweight)):
            C, acc = fold()
            assert np.array_equal(_bits(C[0]), _bits(acc)) and not C[1:].any()
            D = resolve(C, 4.0)
            assert np.array_equal(_bits(D[..., :3]), _bits(acc[..., :3] / acc[..., 3:4]))


def test_consequence_2_a_lone_bright_sample_is_dropped():
    v = np.full((9, 5, 5, 4), 0.5, np.float32)
    v[..., 3] = 1
    v[8, 2, 2, :3] = 5000.0
    for C in (host.fold_cascades(None, v, start=1.0), rw.fold_cascades(np.zeros((6, 5, 5, 4), np.float32), np.zeros((5, 5, 4), np.float32), v, 1.0)[0]):
        assert C[:, 2, 2, 3].tolist() == [8, 0, 0, 0, 1, 0]
        for D in (host.reweight(C, 4.0), rw.reweight(C, 4.0)):
            centre = np.float32(4.0) / np.float32(9.0)
            assert (_bits(D[2, 2, :3]) == _bits(centre)).all(), D[2, 2]
            others = np.ones((5, 5), bool)
            others[2, 2] = False
            assert (D[others][:, :3] == np.float32(0.5)).all()


def test_consequence_3_finite_planes_with_integer_counts_resolve_to_a_finite_image():
    """(Colours up to 1e30: six of them cannot overflow a float.)"""
    rng = np.random.default_rng(13)
    C = np.zeros((6, 33, 41, 4), np.float32)
    C[..., 3] = rng.integers(0, 4, (6, 33, 41))
    C[..., :3] = rng.lognormal(0.0, 8.0, (6, 33, 41, 3)).clip(0, 1e30) * rng.choice([-1.0, 1.0], (6, 33, 41, 3))
    C[:, 5:9, 5:9] = 0  # pixels without a sample
    C[3, 20, 20, :3] = 1e30
    for kappa in (1e-38, 0.5, 4.0, 3e38):
        for D in (host.reweight(C, kappa), rw.reweight(C, kappa)):
            assert np.isfinite(D).all()
            assert not D[5:9, 5:9, :3].any()


def test_counts_and_energy_are_kept_by_the_fold():
    rng = np.random.default_rng(17)
    n = 11
    v = np.zeros((n, 29, 37, 4), np.float32)
    v[..., :3] = (rng.lognormal(0.0, 3.5, (n, 29, 37, 1)) * rng.uniform(0.2, 1.8, (n, 29, 37, 3))).astype(np.float32)
    v[..., 3] = 1
    C, acc = host.fold_cascades(None, v, accum=np.zeros_like(v[0]))
    assert (C[..., 3].sum(0) == n).all() and (acc[..., 3] == n).all()
    assert (C[1:, ..., 3].sum((1, 2)) > 0).all(), "every cascade took samples"
    s = C[..., :3].astype(np.float64).sum(0)
    assert np.allclose(s, acc[..., :3], rtol=1e-4, atol=0)
    # the split: a sample contributes exactly 1 to sum_k lum(C_k) / b_k (to rounding) as long as it is below the top bound
    b = np.array(rw.bounds(1.0), np.float64)
    lc = 0.2126 * C[..., 0].astype(np.float64) + 0.7152 * C[..., 1] + 0.0722 * C[..., 2]
    l = 0.2126 * v[..., 0].astype(np.float64) + 0.7152 * v[..., 1] + 0.0722 * v[..., 2]
    expect = np.where(l <= 1.0, l, np.where(l >= b[5], l / b[5], 1.0)).sum(0)
    assert np.allclose((lc / b[:, None, None]).sum(0), expect, rtol=1e-4)
