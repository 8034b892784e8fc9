"""The texture lookup of include/glrtx.h "Textures" in numpy: the third statement beside csrc/texture.hip.h and host/texture.cpp, bit for bit.

Every operation is one float32 operation in the order the header writes it; `ftz` makes a denormal operand or result the zero of its sign, as the device's
arithmetic and the host's MXCSR mode do.  Textures are given as glrt_amd.host.pack_textures takes them.
"""
from __future__ import annotations

import numpy as np

F = np.float32
RGBA32F, RGBA8_UNORM, RGBA8_SRGB = 0, 1, 2
REPEAT, CLAMP = 0, 1
NEAREST, BILINEAR = 0, 1

# sRGB byte -> linear as float32 bit patterns (srgb_formula() below recomputes them from the piecewise formula in float64)
SRGB_BITS = np.array([
    0x00000000, 0x399f22b4, 0x3a1f22b4, 0x3a6eb40e, 0x3a9f22b4, 0x3ac6eb61, 0x3aeeb40e, 0x3b0b3e5d,
    0x3b1f22b4, 0x3b33070a, 0x3b46eb61, 0x3b5b518e, 0x3b70f18f, 0x3b83e1c6, 0x3b8fe616, 0x3b9c87fd,
    0x3ba9c9b6, 0x3bb7ad6f, 0x3bc6354a, 0x3bd56360, 0x3be539c1, 0x3bf5ba71, 0x3c0373b6, 0x3c0c6153,
    0x3c15a705, 0x3c1f45be, 0x3c293e6b, 0x3c3391f7, 0x3c3e4149, 0x3c494d44, 0x3c54b6c9, 0x3c607eb4,
    0x3c6ca5df, 0x3c792d22, 0x3c830aa9, 0x3c89af9f, 0x3c9085dc, 0x3c978dc6, 0x3c9ec7c2, 0x3ca63433,
    0x3cadd37d, 0x3cb5a602, 0x3cbdac21, 0x3cc5e63a, 0x3cce54ac, 0x3cd6f7d5, 0x3cdfd010, 0x3ce8ddba,
    0x3cf2212d, 0x3cfb9ac3, 0x3d02a56a, 0x3d0798dd, 0x3d0ca7e6, 0x3d11d2af, 0x3d171964, 0x3d1c7c30,
    0x3d21fb3c, 0x3d2796b2, 0x3d2d4ebb, 0x3d332381, 0x3d39152b, 0x3d3f23e4, 0x3d454fd2, 0x3d4b991d,
    0x3d51ffec, 0x3d588468, 0x3d5f26b6, 0x3d65e6fd, 0x3d6cc563, 0x3d73c20e, 0x3d7add24, 0x3d810b65,
    0x3d84b793, 0x3d88732e, 0x3d8c3e48, 0x3d9018f4, 0x3d940344, 0x3d97fd49, 0x3d9c0715, 0x3da020ba,
    0x3da44a4a, 0x3da883d6, 0x3daccd6f, 0x3db12727, 0x3db5910f, 0x3dba0b38, 0x3dbe95b3, 0x3dc33090,
    0x3dc7dbe0, 0x3dcc97b4, 0x3dd1641d, 0x3dd6412b, 0x3ddb2eee, 0x3de02d76, 0x3de53cd4, 0x3dea5d18,
    0x3def8e51, 0x3df4d090, 0x3dfa23e5, 0x3dff885e, 0x3e027f06, 0x3e05427f, 0x3e080ea2, 0x3e0ae377,
    0x3e0dc104, 0x3e10a753, 0x3e13966a, 0x3e168e51, 0x3e198f0f, 0x3e1c98ac, 0x3e1fab30, 0x3e22c6a1,
    0x3e25eb07, 0x3e29186a, 0x3e2c4ed0, 0x3e2f8e42, 0x3e32d6c5, 0x3e362862, 0x3e39831f, 0x3e3ce703,
    0x3e405417, 0x3e43ca60, 0x3e4749e6, 0x3e4ad2af, 0x3e4e64c3, 0x3e520029, 0x3e55a4e7, 0x3e595305,
    0x3e5d0a89, 0x3e60cb7a, 0x3e6495df, 0x3e6869be, 0x3e6c471f, 0x3e702e07, 0x3e741e7e, 0x3e78188b,
    0x3e7c1c33, 0x3e8014bf, 0x3e822039, 0x3e84308b, 0x3e8645b8, 0x3e885fc3, 0x3e8a7eb0, 0x3e8ca281,
    0x3e8ecb3b, 0x3e90f8df, 0x3e932b72, 0x3e9562f6, 0x3e979f6f, 0x3e99e0e0, 0x3e9c274c, 0x3e9e72b6,
    0x3ea0c321, 0x3ea31890, 0x3ea57307, 0x3ea7d288, 0x3eaa3716, 0x3eaca0b6, 0x3eaf0f68, 0x3eb18332,
    0x3eb3fc15, 0x3eb67a14, 0x3eb8fd34, 0x3ebb8576, 0x3ebe12de, 0x3ec0a56e, 0x3ec33d2a, 0x3ec5da14,
    0x3ec87c30, 0x3ecb2380, 0x3ecdd008, 0x3ed081ca, 0x3ed338c9, 0x3ed5f508, 0x3ed8b68a, 0x3edb7d52,
    0x3ede4963, 0x3ee11abf, 0x3ee3f169, 0x3ee6cd65, 0x3ee9aeb5, 0x3eec955b, 0x3eef815c, 0x3ef272b8,
    0x3ef56974, 0x3ef86593, 0x3efb6716, 0x3efe6e00, 0x3f00bd2b, 0x3f02460c, 0x3f03d1a5, 0x3f055ff7,
    0x3f06f104, 0x3f0884cd, 0x3f0a1b54, 0x3f0bb499, 0x3f0d509f, 0x3f0eef65, 0x3f1090ef, 0x3f12353d,
    0x3f13dc50, 0x3f15862a, 0x3f1732cc, 0x3f18e237, 0x3f1a946e, 0x3f1c4970, 0x3f1e0140, 0x3f1fbbde,
    0x3f21794d, 0x3f23398c, 0x3f24fc9f, 0x3f26c285, 0x3f288b41, 0x3f2a56d2, 0x3f2c253c, 0x3f2df67f,
    0x3f2fca9c, 0x3f31a194, 0x3f337b6a, 0x3f35581d, 0x3f3737b0, 0x3f391a24, 0x3f3aff7a, 0x3f3ce7b2,
    0x3f3ed2cf, 0x3f40c0d2, 0x3f42b1bc, 0x3f44a58e, 0x3f469c49, 0x3f4895ef, 0x3f4a9280, 0x3f4c91ff,
    0x3f4e946c, 0x3f5099c9, 0x3f52a216, 0x3f54ad56, 0x3f56bb88, 0x3f58ccaf, 0x3f5ae0cc, 0x3f5cf7df,
    0x3f5f11ea, 0x3f612eef, 0x3f634eee, 0x3f6571e9, 0x3f6797e0, 0x3f69c0d5, 0x3f6becca, 0x3f6e1bbf,
    0x3f704db5, 0x3f7282ae, 0x3f74baab, 0x3f76f5ae, 0x3f7933b6, 0x3f7b74c6, 0x3f7db8de, 0x3f800000,
], np.uint32)
SRGB = SRGB_BITS.view(np.float32)


def srgb_formula():
    """The piecewise sRGB decode of the 256 bytes in float64, rounded once to float32."""
    c = np.arange(256, dtype=np.float64) / 255.0
    return np.where(c <= 0.04045, c / 12.92, ((c + 0.055) / 1.055) ** 2.4).astype(np.float32)


def ftz(x):
    x = np.asarray(x, F)
    tiny = (x.view(np.uint32) & np.uint32(0x7F800000)) == 0
    return np.where(tiny, np.copysign(F(0), x), x).astype(F)


def _op(f, *a):
    with np.errstate(all="ignore"):
        return ftz(f(*[ftz(v) for v in a]))


def add(a, b): return _op(np.add, a, b)
def sub(a, b): return _op(np.subtract, a, b)
def mul(a, b): return _op(np.multiply, a, b)
def div(a, b): return _op(np.divide, a, b)
def floor(a): return _op(np.floor, a)


def coord(s, wrap):
    s = np.asarray(s, F)
    s = np.where(np.isfinite(s), s, F(0)).astype(F)
    s = ftz(s)  # (a comparison reads a denormal as zero too)
    if wrap == CLAMP:
        x = np.where(s > 0, s, F(0)).astype(F)
        return np.where(x < 1, x, F(1)).astype(F)
    return sub(s, floor(s))


def index_of(i, n, wrap):
    i = np.asarray(i, np.int64)
    if wrap == CLAMP:
        return np.clip(i, 0, n - 1)
    i = np.where(i < 0, i + n, i)
    return np.where(i >= n, i - n, i)


def axis(s, n, wrap, filt):
    a = mul(coord(s, wrap), F(n))
    if filt == BILINEAR:
        b = sub(a, F(0.5))
        fl = floor(b)
        f = sub(b, fl)
        i = fl.astype(np.int64)
        return index_of(i, n, wrap), index_of(i + 1, n, wrap), f
    i0 = index_of(floor(a).astype(np.int64), n, wrap)
    return i0, i0, np.zeros(a.shape, F)


def decode(arr, fmt):
    """(h, w, >= 3) texels -> (h, w, 3) float32 channel values."""
    a = np.asarray(arr)[..., :3]
    if fmt == RGBA32F:
        return a.astype(F)
    if fmt == RGBA8_SRGB:
        return SRGB[a.astype(np.int64)]
    return div(a.astype(F), F(255.0))


def lookup_one(arr, fmt, wrap, filt, st):
    """One texture: arr (h, w, 3 or 4), wrap a mode or (wrap_s, wrap_t), st (n, 2) -> rgb (n, 3) float32."""
    ws, wt = wrap if isinstance(wrap, (tuple, list)) else (wrap, wrap)
    tex = decode(arr, fmt)
    h, w = tex.shape[:2]
    st = np.asarray(st, F).reshape(-1, 2)
    x0, x1, fx = axis(st[:, 0], w, ws, filt)
    y0, y1, fy = axis(st[:, 1], h, wt, filt)
    t00 = tex[y0, x0]
    if filt != BILINEAR:
        return t00.astype(F)
    t10, t01, t11 = tex[y0, x1], tex[y1, x0], tex[y1, x1]
    fx, fy = fx[:, None], fy[:, None]
    c0 = add(t00, mul(fx, sub(t10, t00)))
    c1 = add(t01, mul(fx, sub(t11, t01)))
    return add(c0, mul(fy, sub(c1, c0)))


_CODES = dict(rgba32f=0, rgba8_unorm=1, rgba8_srgb=2, repeat=0, clamp=1, nearest=0, bilinear=1)


def _code(v):
    return _CODES[v] if isinstance(v, str) else int(v)


def lookup(textures, which, st):
    """textures: list of (array, format, wrap, filter); which (n,), st (n, 2) -> rgb (n, 3) float32."""
    which = np.asarray(which, np.int64).reshape(-1)
    st = np.asarray(st, F).reshape(-1, 2)
    out = np.zeros((which.size, 3), F)
    for k, (arr, fmt, wrap, filt) in enumerate(textures):
        sel = which == k
        if sel.any():
            wr = tuple(_code(x) for x in wrap) if isinstance(wrap, (tuple, list)) else _code(wrap)
            out[sel] = lookup_one(arr, _code(fmt), wr, _code(filt), st[sel])
    return out


def hit_st(vert, tri, hits):
    """(s, t) at hit records (n, 4) {wire triangle as int32 bits, u, v, 0}; a miss gives (0, 0)."""
    v = np.asarray(vert, F).reshape(-1, 15)
    t = np.asarray(tri, F).reshape(-1, 4)
    h = np.asarray(hits, F).reshape(-1, 4)
    ti = h[:, 0].copy().view(np.int32).astype(np.int64)
    ok = ti >= 0
    idx = t[np.where(ok, ti, 0), :3].astype(np.int64)
    u, w = h[:, 1], h[:, 2]
    w0 = sub(sub(F(1), u), w)
    out = []
    for c in (6, 7):
        a, b, d = v[idx[:, 0], c], v[idx[:, 1], c], v[idx[:, 2], c]
        out.append(add(add(mul(w0, a), mul(u, b)), mul(w, d)))
    return np.where(ok[:, None], np.stack(out, 1), F(0)).astype(F), ok, ti


def albedo(scene, textures, material_texture, hits):
    """What plane A holds (rgb) for hit records as plane G stores them: glrt_texture_albedo's statement."""
    t = np.asarray(scene["tri"], F).reshape(-1, 4)
    m = np.asarray(scene["mat"], F).reshape(-1, 18)
    bind = np.asarray(material_texture, np.int64).reshape(-1)
    st, ok, ti = hit_st(scene["vert"], t, hits)
    out = np.ones((st.shape[0], 3), F)
    mid = t[np.where(ok, ti, 0), 3].astype(np.int64)
    diffuse = ok & (m[mid, 0].astype(np.int64) == 2)
    out[diffuse] = m[mid[diffuse], 6:9]
    bound = diffuse & (bind[mid] >= 0)
    if bound.any():
        out[bound] = lookup(textures, bind[mid[bound]], st[bound])
    return out
