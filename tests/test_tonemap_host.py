"""Tone mapping without a GPU (include/glrtx.h "Tone mapping"): the CPU statement (glrt_exposure_measure / glrt_tonemap, host/tonemap.cpp) and the numpy
statement (tests/tonemap_math.py) agree on every word -- histogram, counted, kept, mean_log2, target, exposure, T -- and on every byte, the numpy side's bytes
being the resolve's checker on T (oracle.pt_oracle.resolve)."""
import numpy as np
import pytest

import tonemap_math as tm
from glrt_amd import host
from oracle import pt_oracle

ROWS, WIDTH = 13, 67
WINDOWS = [(0, 1000), (500, 950), (999, 1000)]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def hostile():
    return tm.hostile_array(ROWS, WIDTH, 19)


def assert_measurement(got, want):
    assert np.array_equal(got["hist"], want["hist"])
    assert (got["counted"], got["kept"]) == (want["counted"], want["kept"])
    for k in ("mean_log2", "target", "exposure"):
        assert bits(got[k]) == bits(want[k]), (k, got[k], want[k])


def test_the_hostile_array_holds_what_the_contract_rules_on(hostile):
    a = hostile
    w = a[..., 3]
    assert (w == 0).any() and np.isnan(w).any() and np.isinf(w).any() and (w < 0).any() and ((np.abs(w) < 1e-38) & (w != 0)).any()
    assert np.isnan(a[..., :3]).any() and np.isinf(a[..., :3]).any() and (a[..., :3] < 0).any()
    h = tm.histogram(a)
    assert h[0] > 0 and h[255] > 0 and h.sum() < ROWS * WIDTH  # below 2^-16, above 2^16, and pixels that are not counted
    l = tm.lum(tm.mean_of(a))
    edge = (l.view(np.uint32) & np.uint32(0x000FFFFF)) == 0
    assert edge.sum() >= 4  # luminances exactly on a bin edge


@pytest.mark.parametrize("low,high", WINDOWS)
@pytest.mark.parametrize("prev", [None, 0.37])
def test_measure_agrees_on_hostile_arrays(hostile, low, high, prev):
    kw = dict(key=0.18, low_permille=low, high_permille=high, adapt=0.25)
    assert_measurement(host.exposure_measure(hostile, prev, **kw), tm.measure(hostile, prev, **kw))


def test_bins_are_eight_an_octave_from_two_to_the_minus_sixteen():
    """Bin k of octave e holds the mantissas [1 + k / 8, 1 + (k + 1) / 8): the top three mantissa bits, not a logarithm."""
    l = np.array([2.0 ** -16, 2.0 ** -16 * 1.13, 1.0, 1.126, 1.99, 2.0 ** 15 * 1.99, 2.0 ** 16, 1e30, 2.0 ** -17, 1e-30], np.float32)
    a = np.ones((1, l.size, 4), np.float32)
    a[0, :, :3] = l[:, None]
    # lum of a grey pixel may differ from g by an ulp: check against the statement's own luminance
    lum = tm.lum(a[..., :3])[0]
    m, e = np.frexp(lum.astype(np.float64))  # lum = m * 2^e, m in [0.5, 1)
    want = np.clip(8 * (e - 1 + 16) + np.floor(8 * (2 * m - 1)), 0, 255).astype(int)
    assert list(want) == [0, 1, 128, 129, 135, 255, 255, 255, 0, 0]
    got = host.exposure_measure(a)["hist"]
    assert np.array_equal(got, np.bincount(want, minlength=256))
    assert np.array_equal(got, tm.histogram(a))


def test_one_bin_and_no_counted_pixel():
    flat = np.empty((ROWS, WIDTH, 4), np.float32)
    flat[...] = (0.9, 0.6, 0.3, 2.0)
    for low, high in WINDOWS:
        g, w = host.exposure_measure(flat, None, low_permille=low, high_permille=high), tm.measure(flat, None, low_permille=low, high_permille=high)
        assert_measurement(g, w)
        assert np.count_nonzero(g["hist"]) == 1 and g["hist"].max() == ROWS * WIDTH and g["kept"] > 0
        k = int(np.argmax(g["hist"]))
        assert g["mean_log2"] == np.float32((2 * k + 1) / 16 - 16)  # the bin's centre, whatever the window
    none = np.zeros((ROWS, WIDTH, 4), np.float32)
    none[..., :3] = 1.0  # (count 0: every pixel is dead)
    none[0, 0] = (-1.0, -1.0, -1.0, 1.0)  # alive, luminance < 0: not counted
    first = host.exposure_measure(none, None)
    assert_measurement(first, tm.measure(none, None))
    assert first["counted"] == 0 and first["kept"] == 0 and first["target"] == 1.0 and first["exposure"] == 1.0 and first["mean_log2"] == 0.0
    later = host.exposure_measure(none, 0.37, adapt=0.5)
    assert_measurement(later, tm.measure(none, 0.37, adapt=0.5))
    assert later["target"] == np.float32(0.37) and later["exposure"] == np.float32(0.37)
    # one counted pixel under 500 / 950: N = 1, lo = hi = 0 -- a window that keeps nothing
    one = none.copy()
    one[1, 1] = (1.0, 1.0, 1.0, 1.0)
    g = host.exposure_measure(one, None)
    assert_measurement(g, tm.measure(one, None))
    assert g["counted"] == 1 and g["kept"] == 0 and g["exposure"] == 1.0


def test_a_three_measurement_adaptation_sequence(hostile):
    imgs = [hostile, hostile * np.array([0.125, 0.125, 0.125, 1.0], np.float32), tm.hostile_array(ROWS, WIDTH, 5)]  # (the second: three stops darker)
    Eh = En = None
    seen = []
    for a in imgs:
        g, w = host.exposure_measure(a, Eh, adapt=0.25), tm.measure(a, En, adapt=0.25)
        assert_measurement(g, w)
        if Eh is not None:
            assert g["exposure"] != g["target"]  # a quarter of the way, not a jump
        Eh, En = g["exposure"], w["exposure"]
        seen.append(float(Eh))
    assert len(set(seen)) == 3


@pytest.mark.parametrize("op", [0, 1, 2])
@pytest.mark.parametrize("auto", [0, 1])
@pytest.mark.parametrize("flip", [0, 1])
def test_curve_and_bytes_agree_on_hostile_arrays(hostile, op, auto, flip):
    E = tm.measure(hostile)["exposure"]
    kw = dict(op=op, auto_exposure=auto, exposure=1.7, E=E, white=3.0)
    T, b = host.tonemap(hostile, gamma=2.2, flip_y=flip, **kw)
    Tn = tm.tonemap(hostile, **kw)
    assert np.array_equal(bits(T), bits(Tn))
    assert np.array_equal(b, pt_oracle.resolve(Tn, 2.2, bool(flip)))
    assert not np.isnan(T).any() and (T[..., :3] >= 0).all() and (T[..., 3] == 1).all()
    assert (T[tm.dead_of(hostile)][:, :3] == 0).all()


def test_clamp_at_unit_exposure_is_the_plain_resolve():
    rng = np.random.default_rng(3)
    a = np.zeros((ROWS, WIDTH, 4), np.float32)
    a[..., 3] = rng.integers(1, 9, (ROWS, WIDTH))
    a[..., :3] = rng.lognormal(-1.0, 2.0, (ROWS, WIDTH, 3)) * a[..., 3:4]
    a[2, 3] = 0  # a dead pixel whose sums are zeros
    _, b = host.tonemap(a, op=0, exposure=1.0, gamma=2.2, flip_y=1)
    assert np.array_equal(b, pt_oracle.resolve(a, 2.2, True))


def test_the_curves_do_what_they_are_for():
    a = np.ones((1, 5, 4), np.float32)
    a[0, :, :3] = np.array([0.0, 0.18, 1.0, 4.0, 1e6], np.float32)[:, None]
    r = host.tonemap(a, op=1, white=4.0)[0][0, :, 0]
    assert r[0] == 0 and r[3] == 1.0 and np.all(np.diff(r) > 0)  # Reinhard: the white point maps to 1
    c = host.tonemap(a, op=2)[0][0, :, 0]
    assert c[0] == 0 and np.all(np.diff(c[:4]) > 0) and 0.95 < c[3] < 1.0 < c[4] < 1.04  # (the fit tends to 2.51 / 2.43)
    bright = host.tonemap(a, op=2, auto_exposure=1, E=0.01, exposure=1.0)[0][0, :, 0]
    assert np.all(bright[1:4] < c[1:4])


BAD = [dict(key=0.0), dict(key=float("nan")), dict(adapt=0.0), dict(adapt=1.5), dict(low_permille=950, high_permille=500), dict(low_permille=500, high_permille=500),
       dict(low_permille=-1), dict(high_permille=1001)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_bad_measurement_arguments_are_refused(bad):
    with pytest.raises(RuntimeError):
        host.exposure_measure(np.ones((2, 2, 4), np.float32), **bad)


@pytest.mark.parametrize("bad", [dict(op=3), dict(op=-1), dict(exposure=0.0), dict(exposure=float("inf")), dict(white=0.0), dict(white=1e-30), dict(gamma=0.0)],
                         ids=lambda b: ",".join(f"{k}={v}" for k, v in b.items()))
def test_bad_curve_arguments_are_refused(bad):
    with pytest.raises(RuntimeError):
        host.tonemap(np.ones((2, 2, 4), np.float32), **bad)
