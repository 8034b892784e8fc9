"""The one-channel lookup and the alpha test of include/glrtx.h "Cutouts" in numpy: the third statement beside csrc/texture.hip.h (tex_lookup_channel,
cut_accepts) and host/texture.cpp (glrt_texture_channel), bit for bit.

Built on tests/texture_math.py, which states the coordinate, index and filter rules: channels 0 .. 2 decode as that file's `decode` does; channel 3 is the
texel's fourth float (rgba32f) or byte / 255.0f (BOTH 8-bit formats: alpha is never sRGB-decoded), filtered by the same expression.  Textures are given as
glrt_amd.host.pack_textures takes them; a three-channel array has the alpha pack_textures appends (1.0, or byte 255).
"""
from __future__ import annotations

import numpy as np

import texture_math as tm

F = np.float32


def decode_channel(arr, fmt, channel):
    """(h, w, 3 or 4) texels -> (h, w) float32 values of one channel, 0 .. 3."""
    a = np.asarray(arr)
    if a.shape[2] == 3:  # pack_textures' alpha
        a = np.concatenate([a, np.full(a.shape[:2] + (1,), 1.0 if fmt == tm.RGBA32F else 255, a.dtype)], axis=2)
    c = a[..., channel]
    if fmt == tm.RGBA32F:
        return c.astype(F)
    if fmt == tm.RGBA8_SRGB and channel < 3:
        return tm.SRGB[c.astype(np.int64)]
    return tm.div(c.astype(F), F(255.0))


def channel_one(arr, fmt, wrap, filt, channel, st):
    """One texture, one channel: st (n, 2) -> (n,) float32."""
    ws, wt = wrap if isinstance(wrap, (tuple, list)) else (wrap, wrap)
    tex = decode_channel(arr, fmt, channel)
    h, w = tex.shape
    st = np.asarray(st, F).reshape(-1, 2)
    x0, x1, fx = tm.axis(st[:, 0], w, ws, filt)
    y0, y1, fy = tm.axis(st[:, 1], h, wt, filt)
    t00 = tex[y0, x0]
    if filt != tm.BILINEAR:
        return t00.astype(F)
    t10, t01, t11 = tex[y0, x1], tex[y1, x0], tex[y1, x1]
    c0 = tm.add(t00, tm.mul(fx, tm.sub(t10, t00)))
    c1 = tm.add(t01, tm.mul(fx, tm.sub(t11, t01)))
    return tm.add(c0, tm.mul(fy, tm.sub(c1, c0)))


def channel(textures, which, channel, st):
    """textures: list of (array, format, wrap, filter); which (n,), channel (n,) or one number, st (n, 2) -> (n,) float32."""
    which = np.asarray(which, np.int64).reshape(-1)
    ch = np.broadcast_to(np.asarray(channel, np.int64), which.shape)
    st = np.asarray(st, F).reshape(-1, 2)
    out = np.zeros(which.size, F)
    for k, (arr, fmt, wrap, filt) in enumerate(textures):
        wr = tuple(tm._code(x) for x in wrap) if isinstance(wrap, (tuple, list)) else tm._code(wrap)
        for c in range(4):
            sel = (which == k) & (ch == c)
            if sel.any():
                out[sel] = channel_one(arr, tm._code(fmt), wr, tm._code(filt), c, st[sel])
    return out


def accepts(value, cutoff):
    """The test: accepted iff value >= cutoff; a NaN value rejects.  (A comparison reads a denormal as the zero of its sign.)"""
    with np.errstate(invalid="ignore"):
        return tm.ftz(value) >= tm.ftz(np.asarray(cutoff, F))
