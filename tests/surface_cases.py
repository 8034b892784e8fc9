"""What tests/test_oracle_surface.py (CPU) and tests/test_gpu_surface_oracle.py (GPU) share: the oracle rendered through its surface hooks (oracle/pt_oracle.c
"surface hooks", filled by glrt_amd.host.Surface), the n = 6 walls with free corner coordinates, small random textures, and the reduction of a texture to one
texel a triangle -- the texel at each triangle's centroid, which is what every pin that existed before these tests could see of it."""
import numpy as np

from glrt_amd import host
from oracle import pt_oracle

F = np.float32
N = 6
SEEDS = (host.frame_seed(0), host.frame_seed(1))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def share(a, b):
    """The share of pixels on which two accumulators differ in any bit"""
    return float((bits(a) != bits(b)).any(-1).mean())


def same(got, ref, what):
    bad = (bits(got) != bits(ref)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])].tolist()} vs {ref[tuple(np.argwhere(bad)[0])].tolist()}"


def none(scene):
    return np.full(scene["mat"].reshape(-1, 18).shape[0], -1, np.int32)


def at(scene, material, k=0):
    a = none(scene)
    a[material] = k
    return a


def oracle(scene, params, seeds=SEEDS, surface=None, **kw):
    """(accumulator, rays) of the frames `seeds`, accumulated; surface: what host.Surface.hooks() returns"""
    ref, rays = None, 0
    for sd in seeds:
        ref, n = pt_oracle.render(scene, dict(params, seed=sd), accum=ref, surface=surface, **kw)
        rays += n
    return ref, rays


def hooked(render_scene, params, bound_scene, textures, material_texture=None, cut=None, material_emission=None, seeds=SEEDS, **kw):
    """The oracle's image of render_scene with the lookups of bound_scene (the scene as it was uploaded: its coordinates are the ones that count)"""
    with host.Surface(bound_scene, textures, material_texture, cut, material_emission) as s:
        return oracle(render_scene, params, seeds, surface=s.hooks(albedo=material_texture is not None, accept=cut is not None, emission=material_emission is not None), **kw)


def free_uv(seed, n=N):
    """Free coordinates, uniform in [-1, 2], at every corner of the wall's 2 n n triangles: wrap seams, clamp regions and texel borders fall inside triangles"""
    return np.random.default_rng(seed).uniform(-1.0, 2.0, (2 * n * n, 3, 2)).astype(F)


def random_texture(width, height, fmt, wrap, filt, seed, alpha=None):
    """(array, format, wrap, filter) as host.pack_textures takes it: colours uniform in [0.05, 0.95] (float) or bytes 13 .. 242, alpha uniform in [0, 1] / 0 .. 255"""
    rng = np.random.default_rng(seed)
    if fmt == "rgba32f":
        a = rng.uniform(0.05, 0.95, (height, width, 4)).astype(F)
        a[..., 3] = rng.uniform(0.0, 1.0, (height, width)).astype(F)
    else:
        a = rng.integers(13, 243, (height, width, 4), dtype=np.uint8)
        a[..., 3] = rng.integers(0, 256, (height, width), dtype=np.uint8)
    return (a, fmt, wrap, filt)


def centroid_reduction(scene, tris, texture):
    """(uv (len(tris), 3, 2), texture'): coordinates that are each triangle's centroid at all three corners, and the texture with nearest filtering -- the
    per-triangle-constant picture of `texture` on the wire triangles `tris` (consecutive, unshared vertices)."""
    v = np.asarray(scene["vert"], F).reshape(-1, 5, 3)
    t = np.asarray(scene["tri"], F).reshape(-1, 4)
    st = np.stack([v[t[list(tris), k].astype(np.int64), 2, :2] for k in range(3)], 1)  # (n, 3, 2)
    c = st.astype(np.float64).mean(1).astype(F)
    arr, fmt, wrap, _ = texture
    return np.repeat(c[:, None, :], 3, 1), (arr, fmt, wrap, "nearest")


def with_uv(scene, wall, uv):
    """`scene` with the wall's corner coordinates replaced by uv (2 n n, 3, 2)"""
    v = np.array(scene["vert"], F).reshape(-1, 5, 3)
    v[wall["vert"].start:wall["vert"].stop, 2, :2] = np.asarray(uv, F).reshape(-1, 2)
    return dict(scene, vert=v.reshape(-1, 3))
