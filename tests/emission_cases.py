"""The cases tests/test_emission_host.py (CPU) and tests/test_gpu_emission.py (GPU) share for the sampled side of emission maps: a scene of random light
triangles on nine emitter materials -- one a texture in each of 3 formats x 2 filters, one on a 1 x 1 texture, one unbound, one (bound) holding a degenerate
light and lights with NaN and infinite coordinates --, and the lights and raw uniforms they are sampled at, the flip's boundary included."""
import functools

import numpy as np

import texture_cases
from glrt_amd import scenes

F = np.float32
FORMATS = ("rgba32f", "rgba8_unorm", "rgba8_srgb")
FILTERS = ("nearest", "bilinear")
PER_MATERIAL = 5  # light triangles a material


@functools.lru_cache(maxsize=None)
def case():
    """(scene, textures, material_emission, lid (n,), u (n, 2))"""
    rng = np.random.default_rng(2024)
    textures = [(texture_cases.texels(5, 4, fmt, 7 + k), fmt, ("repeat", "clamp") if k % 2 else "repeat", filt)
                for k, (fmt, filt) in enumerate((a, b) for a in FORMATS for b in FILTERS)]
    textures.append((texture_cases.texels(1, 1, "rgba32f", 99), "rgba32f", "clamp", "bilinear"))  # 1 x 1
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    b.add_mesh(*scenes.quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    bind = [-1]
    for k in range(9):
        m = b.add_material(scenes.emitter(tuple(float(x) for x in rng.uniform(0.5, 20.0, 3).astype(F))))
        pos, nrm, _ = scenes.random_triangles(PER_MATERIAL, 50 + k, 3.0, 0.5)
        uv = rng.uniform(-1.0, 2.0, (PER_MATERIAL, 3, 2)).astype(F)
        if k == 8:  # the special lights, bound to the RGBA8 bilinear texture
            pos[0, 1] = pos[0, 0]; pos[0, 2] = pos[0, 0]  # a degenerate light: a point
            uv[0] = uv[0, 0]                                # ... with one coordinate pair
            uv[1, 0, 0] = np.nan; uv[1, 2, 1] = np.nan
            uv[2, 1, 0] = np.inf; uv[2, 1, 1] = -np.inf
            uv[3] = F([[1e-40, -1e-40], [0.0, 1.0], [1.0, 0.0]])  # denormal coordinates
        b.add_mesh(pos, nrm, m, uv=uv)
        bind.append(k if k < 7 else (-1 if k == 7 else 3))
    scene = b.build("sah")
    n_light = scene["light"].reshape(-1, 4).shape[0]
    assert n_light == 9 * PER_MATERIAL
    u = rng.uniform(0.0, 1.0, (40 * n_light, 2)).astype(F)
    lid = np.tile(np.arange(n_light, dtype=np.int32), 40)
    # the flip's boundary: ua0 + ub0 exactly 1 (no flip), the smallest sum above it, 1 + 2^-23 (flip), the corners, and pt_rand's largest value
    top = np.nextafter(F(1), F(0))
    edge = F([[0.25, 0.75], [0.25, F(0.75) + F(2.0 ** -23)], [0.0, 0.0], [top, 0.0], [0.0, top], [top, top], [0.5, 0.5], [1e-40, 1e-41]])
    u = np.concatenate([u, np.repeat(edge, n_light, 0)])
    lid = np.concatenate([lid, np.tile(np.arange(n_light, dtype=np.int32), len(edge))])
    return scene, textures, np.asarray(bind, np.int32), lid, u
