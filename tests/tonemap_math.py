"""numpy statement of the tone-mapping passes (include/glrtx.h "Tone mapping"; csrc/tonemap.hip.h; host/tonemap.cpp).

Every fp32 operation is one IEEE float32 operation, correctly rounded, in the kernel's order; lp_exp (tests/volume_math.py) carries the only fused operations.
Denormals count as zeros of their sign on the way into and out of every operation (ftz).  The histogram and its window are integers; the mean is one double
quotient, one double difference and one rounding to float32.  The bytes behind T are the resolve's: oracle.pt_oracle.resolve(T, gamma, flip_y).
"""
from __future__ import annotations

import numpy as np

from adaptive_math import _op, ftz
from volume_math import lp_exp

f32 = np.float32
DEFAULTS = dict(op=0, source=0, auto_exposure=0, exposure=1.0, key=0.18, low_permille=500, high_permille=950, adapt=1.0, white=4.0, gamma=2.2, flip_y=1)
LN2 = f32(float.fromhex("0x1.62e430p-1"))


def add(a, b): return _op(np.add, a, b)
def sub(a, b): return _op(np.subtract, a, b)
def mul(a, b): return _op(np.multiply, a, b)
def div(a, b): return _op(np.divide, a, b)


def dead_of(src):
    w = np.asarray(src, np.float32)[..., 3]
    return ((w.view(np.uint32) & np.uint32(0x7F800000)) == 0) | np.isnan(w)


def mean_of(src):
    s = np.ascontiguousarray(src, np.float32)
    return div(s[..., :3], s[..., 3:4])


def lum(c):
    return add(add(mul(f32(0.2126), c[..., 0]), mul(f32(0.7152), c[..., 1])), mul(f32(0.0722), c[..., 2]))


def histogram(src):
    """256 uint32 counts: bin k = clamp((bits(l) >> 20) - 888, 0, 255) of every live pixel whose luminance is a positive finite number."""
    src = np.ascontiguousarray(src, np.float32)
    l = lum(mean_of(src))
    with np.errstate(invalid="ignore"):
        ok = ~dead_of(src) & (l > 0) & ~np.isinf(l)
    k = np.clip((l[ok].view(np.uint32) >> np.uint32(20)).astype(np.int64) - 888, 0, 255)
    return np.bincount(k, minlength=256).astype(np.uint32)


def reduce(hist, key, low_permille, high_permille, adapt, prev=None):
    """The window, the mean and the exposure update.  prev: the previous E (None: a first measurement).  Returns dict(counted, kept, mean_log2, target, exposure)."""
    h = [int(v) for v in hist]
    N = sum(h)
    lo, hi = N * int(low_permille) // 1000, N * int(high_permille) // 1000
    c = K = S = 0
    for k in range(256):
        kept = max(0, min(c + h[k], hi) - max(c, lo))
        K += kept
        S += kept * (2 * k + 1)
        c += h[k]
    if K:
        mean = f32(np.float64(S) / np.float64(16 * K) - np.float64(16.0))
        target = mul(f32(key), ftz(lp_exp(mul(sub(f32(0), mean), LN2))))
    else:
        mean, target = f32(0), f32(1) if prev is None else f32(prev)
    E = target if prev is None else add(f32(prev), mul(sub(target, f32(prev)), f32(adapt)))
    return dict(counted=N, kept=K, mean_log2=f32(mean), target=f32(target), exposure=f32(E))


def measure(src, prev=None, key=DEFAULTS["key"], low_permille=DEFAULTS["low_permille"], high_permille=DEFAULTS["high_permille"], adapt=DEFAULTS["adapt"], **_):
    """One measurement of a (rows, width, 4) float32 image: reduce()'s dict plus hist."""
    hist = histogram(src)
    return dict(reduce(hist, key, low_permille, high_permille, adapt, prev), hist=hist)


def tonemap(src, op=0, auto_exposure=0, exposure=1.0, E=1.0, white=4.0, **_):
    """T, (rows, width, 4) float32 {y, 1}: the curve over src.rgb / src.w with s = auto_exposure ? E * exposure : exposure; dead pixels {0, 0, 0, 1}."""
    src = np.ascontiguousarray(src, np.float32)
    s = mul(f32(E), f32(exposure)) if auto_exposure else ftz(f32(exposure))
    x = mul(mean_of(src), s)
    with np.errstate(invalid="ignore"):
        x = np.where(x > 0, x, f32(0)).astype(np.float32)
        x = np.where(x < f32(65504), x, f32(65504)).astype(np.float32)
    one = f32(1)
    if op == 1:
        ww = mul(f32(white), f32(white))
        y = div(mul(x, add(one, div(x, ww))), add(one, x))
    elif op == 2:
        y = div(mul(x, add(mul(f32(2.51), x), f32(0.03))), add(mul(x, add(mul(f32(2.43), x), f32(0.59))), f32(0.14)))
    else:
        y = x
    T = np.ones(src.shape, np.float32)
    T[..., :3] = np.where(dead_of(src)[..., None], f32(0), y)
    return T


def hostile_array(rows, width, seed):
    """An HDR accumulator with everything the contract has a rule for: counts that are zero, denormal, NaN, Inf and negative; NaN, Inf and negative channels;
    grey pixels whose luminance sits on octave and bin edges; luminances below 2^-16 and above 2^16."""
    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 5, (rows, width)).astype(np.float32)
    a = np.zeros((rows, width, 4), np.float32)
    a[..., :3] = (rng.lognormal(-1.0, 3.0, (rows, width, 3)) * cnt[..., None]).astype(np.float32)
    a[..., 3] = cnt
    k = rng.permutation(rows * width)[:64]
    y, x = k // width, k % width
    def put(i, rgb=None, w=None):
        if rgb is not None: a[y[i], x[i], :3] = rgb
        if w is not None: a[y[i], x[i], 3] = w
    put(0, w=f32(0.0)); put(1, w=f32(-0.0)); put(2, w=f32(1e-40)); put(3, w=np.nan); put(4, w=np.inf); put(5, w=-np.inf); put(6, w=f32(-2.0))
    put(7, rgb=(np.nan, 1.0, 1.0)); put(8, rgb=(1.0, np.inf, 1.0)); put(9, rgb=(1.0, 1.0, -np.inf)); put(10, rgb=(-3.0, 0.5, 0.25)); put(11, rgb=(-1.0, -1.0, -1.0))
    put(12, rgb=(np.inf, np.inf, np.inf), w=np.inf); put(13, rgb=(0.0, 0.0, 0.0)); put(14, rgb=f32(1e-40)); put(15, rgb=f32(3e38), w=f32(1.0))
    put(16, rgb=f32(3e38), w=f32(1e-30)); put(17, rgb=f32(1e-30), w=f32(3e38))
    # luminances on the edges: grey g gives l = g * (0.2126 + 0.7152 + 0.0722) to within an ulp, so step through the neighbours of each edge
    i = 18
    for e in (-17, -16, -15, -1, 0, 1, 15, 16, 17):
        for ulp in (-2, 0, 2):
            g = (np.array([2.0 ** e], np.float32).view(np.uint32) + np.uint32(ulp & 0xFFFFFFFF)).view(np.float32)[0]
            put(i, rgb=g, w=f32(1.0)); i += 1
    for frac in (1, 3, 7):  # bin edges inside an octave: mantissas k / 8
        g = (np.array([1.0 + frac / 8.0], np.float32).view(np.uint32) - np.uint32(1)).view(np.float32)[0]
        put(i, rgb=g, w=f32(1.0)); i += 1
        put(i, rgb=f32(1.0 + frac / 8.0), w=f32(1.0)); i += 1
    put(i, rgb=f32(65504.0), w=f32(1.0)); i += 1
    put(i, rgb=f32(65536.0), w=f32(1.0)); i += 1
    assert i <= 64
    return a
