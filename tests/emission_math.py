"""The sampled-side rule of emission maps (include/glrtx.h "Emission maps") in numpy, one rounded fp32 operation at a time, denormals flushed -- the third
statement beside csrc/texture.hip.h (emit_light_st / emit_radiance) and host/texture.cpp (glrt_light_emission).  The lookup itself is texture_math's."""
from __future__ import annotations

import numpy as np

import texture_math as tm

F = np.float32


def light_st(scene):
    """(n_light, 3, 2): words 6 and 7 of every light's three vertices in wire order."""
    v = np.asarray(scene["vert"], F).reshape(-1, 15)
    l = np.asarray(scene["light"], F).reshape(-1, 4)
    return v[l[:, :3].astype(np.int64)][:, :, 6:8].astype(F)


def sample_st(st3, u):
    """st3 (n, 3, 2), u (n, 2) RAW uniforms -> (n, 2): the flip at ua0 + ub0 > 1, w0 = (1 - ua) - ub, s = (w0 * s0 + ua * s1) + ub * s2, t likewise."""
    u = np.asarray(u, F).reshape(-1, 2)
    ua0, ub0 = u[:, 0], u[:, 1]
    with np.errstate(all="ignore"):
        flip = F(1) < tm.add(ua0, ub0)
    ua = np.where(flip, tm.sub(F(1), ua0), tm.ftz(ua0)).astype(F)
    ub = np.where(flip, tm.sub(F(1), ub0), tm.ftz(ub0)).astype(F)
    w0 = tm.sub(tm.sub(F(1), ua), ub)
    out = [tm.add(tm.add(tm.mul(w0, st3[:, 0, c]), tm.mul(ua, st3[:, 1, c])), tm.mul(ub, st3[:, 2, c])) for c in (0, 1)]
    return np.stack(out, 1).astype(F)


def light_emission(scene, textures, material_emission, lid, u):
    """(n, 5) float32 {s, t, Le.rgb}: Le = emission * lookup(s, t) per channel (one rounded product) where the light's material is bound, else the emission."""
    lid = np.asarray(lid, np.int64).reshape(-1)
    m = np.asarray(scene["mat"], F).reshape(-1, 18)
    l = np.asarray(scene["light"], F).reshape(-1, 4)
    bind = np.asarray(material_emission, np.int64).reshape(-1)
    st = sample_st(light_st(scene)[lid], u)
    mid = l[lid, 3].astype(np.int64)
    le = m[mid, 3:6].copy()  # (an unbound light: the material's words as they are)
    bound = bind[mid] >= 0
    if bound.any():
        c = tm.lookup(textures, bind[mid[bound]], st[bound])
        le[bound] = tm.mul(m[mid[bound], 3:6], c)
    return np.concatenate([st, le], 1).astype(F)
