"""numpy statement of the volume branch's arithmetic (csrc/pt_kernel.hip.h: lp_log, lp_exp, lp_acos, vol_blackbody, vol_lookup).

The device restates the sequences Mesa llvmpipe generates for the reference's fragment shader, operation by operation; this module
states the same sequences once more in numpy, so that the stored llvmpipe sweeps (tests/golden/math_volume.npz) pin them on the CPU
and the device's debug export can be compared with both.  Every operation is rounded to float32 on its own, except the fused
multiply-adds, which are rounded once (fma32).
"""
from __future__ import annotations

import numpy as np

f32 = np.float32


def bits(u: int) -> np.float32:
    return np.array([u], np.uint32).view(np.float32)[0]


def fma32(a, b, c):
    """Correctly rounded float32 a * b + c.  The product is exact in float64; the float64 sum is rounded once, and where that rounding lands
    exactly on a float32 halfway point, the sign of its error (TwoSum) decides the direction."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    c = np.asarray(c, np.float32).astype(np.float64)
    a, b, c = np.broadcast_arrays(a, b, c)
    p = a * b
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        r = s.astype(np.float32)
        rd = r.astype(np.float64)
        toward = np.where(s > rd, np.inf, -np.inf).astype(np.float32)
        nb = np.nextafter(r, toward)
        mid = (rd + nb.astype(np.float64)) * 0.5
        tie = np.isfinite(s) & (err != 0) & (s != rd) & (s == mid)
        # at a tie the exact value lies on err's side of the halfway point
        up = np.where(err > 0, np.maximum(r, nb), np.minimum(r, nb))
        return np.where(tie, up, r).astype(np.float32)


def lp_log(x):
    x = np.asarray(x, np.float32)
    b = x.view(np.uint32)
    e = (((b & np.uint32(0x7F800000)) >> np.uint32(23)).astype(np.int32) - 127).astype(np.float32)
    m = ((b & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)).view(np.float32)
    with np.errstate(all="ignore"):
        y = (m - f32(1)) / (m + f32(1))
        y2 = y * y
        y4 = y2 * y2
        p0 = fma32(y4, bits(0x3ED03D59), bits(0x3F13D321))
        p1 = fma32(y4, bits(0x3ECE8316), bits(0x3F7637F9))
        p2 = fma32(y4, p0, bits(0x4038AA3B))
        p3 = fma32(p1, y2, p2)
        l2 = fma32(y, p3, e)
        l2 = np.where((x >= np.inf) | np.isnan(x), f32(np.inf), l2)
        l2 = np.where((x == 0) | np.isnan(x), f32(-np.inf), l2)
        l2 = np.where(~(x >= 0), f32(np.nan), l2)
        return (l2 * bits(0x3F317218)).astype(np.float32)


def lp_exp(x):
    x = np.asarray(x, np.float32)
    with np.errstate(all="ignore"):
        t = x * bits(0x3FB8AA3B)
        t = np.where(f32(128) < t, f32(128), t)
        lo = bits(0xC2FDFFFF)
        t = np.where(lo > t, lo, t).astype(np.float32)
        fl = np.floor(t)
        f = t - fl
        p2 = (((np.nan_to_num(fl).astype(np.int32) + 127).astype(np.uint32)) << np.uint32(23)).view(np.float32)
        z = f * f
        a = fma32(z, bits(0x3AF61905), bits(0x3D64AA23))
        b = fma32(z, bits(0x3C134806), bits(0x3E75EAD4))
        c = fma32(z, a, bits(0x3F31727B))
        d = fma32(z, b, f32(1))
        return (p2 * fma32(c, f, d)).astype(np.float32)


def lp_acos(x):
    x = np.asarray(x, np.float32)
    hpi = bits(0x3FC90FDB)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        s = np.sqrt(f32(1) - ax)
        p = ax * bits(0xBCC19A5F)
        p = bits(0x3DA68D87) + p
        p = ax * p
        p = bits(0xBE5BC094) + p
        p = ax * p
        p = hpi + p
        r = hpi - s * p
        sg = np.where((x == 0) | np.isnan(x), f32(0), np.copysign(f32(1), x)).astype(np.float32)
        return (hpi - sg * r).astype(np.float32)


# blackBody(T) at T = 100 * v (raytrace.frag:125-142 with temperatureLookup() * 1.0e2 inlined): the GLSL compiler folds h*c, 2*h*c*c,
# l^5 and (l*k)*100 into one constant each; the order below is that of the generated code.
BB_HC = 0x1675E7CD
BB_HCC2 = 0x25095070
BB_LK100 = (0x12857250, 0x1270A42A, 0x1244E369)  # (l*k) * 100 for l = 610, 550, 450 nm
BB_L5 = (0x0BDB450B, 0x0B82A8FA, 0x0ABF9FFC)


def blackbody(v):
    """v: the temperature grid's value (T / 100).  Returns (n, 3) float32."""
    v = np.asarray(v, np.float32)
    out = []
    with np.errstate(all="ignore"):
        for lk, l5 in zip(BB_LK100, BB_L5):
            q = bits(BB_HC) / (bits(lk) * v)
            e = lp_exp(q) + f32(-1)
            r = bits(BB_HCC2) / (bits(l5) * e)
            out.append(np.where(r > 0, r, f32(0)).astype(np.float32))
    return np.stack(out, -1)


def lookup(grid, bbox_min, bbox_max, pos):
    """textureLod(sampler3D, (pos - bboxMin) / (bboxMax - bboxMin), 0.0).x on an R32F texture: the magnification filter (trilinear),
    GL_REPEAT, texel centres at (i + 0.5) / n.  grid (nz, ny, nx), x fastest; pos (n, 3)."""
    g = np.asarray(grid, np.float32)
    nz, ny, nx = g.shape
    pos = np.asarray(pos, np.float32)
    lo = np.asarray(bbox_min, np.float32)
    hi = np.asarray(bbox_max, np.float32)
    idx, w = [], []
    with np.errstate(all="ignore"):
        uvw = (pos - lo) / (hi - lo)
        for ax, n in enumerate((nx, ny, nz)):
            s = uvw[:, ax]
            f = s - np.floor(s)
            c = f * f32(n) - f32(0.5)
            fl = np.floor(c)
            w.append((c - fl).astype(np.float32))
            i0 = np.where(~(c >= 0), n - 1, np.nan_to_num(fl).astype(np.int64))
            i1 = np.where(i0 != n - 1, i0 + 1, 0)
            idx.append((i0, i1))
        (x0, x1), (y0, y1), (z0, z1) = idx
        wx, wy, wz = w

        def lerp(t, a, b):
            return fma32(t, b - a, a)

        def plane(z):
            r0 = lerp(wx, g[z, y0, x0], g[z, y0, x1])
            r1 = lerp(wx, g[z, y1, x0], g[z, y1, x1])
            return lerp(wy, r0, r1)

        return lerp(wz, plane(z0), plane(z1))
