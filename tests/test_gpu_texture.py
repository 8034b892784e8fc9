"""Textured albedo on the GPU (csrc/texture.hip.h; include/glrtx.h "Textures").  The lookup kernel equals the CPU statement bit for bit on the CPU test's cases.
The shading is pinned THROUGH the reference: a texture whose texels are constant over each triangle must render, bit for bit and ray for ray, what the oracle
renders for the same geometry with one diffuse material a triangle -- with float, bilinear and sRGB textures, beyond the LDS material limit, next to analytic
spheres and a dielectric, and after the geometry moved.  The feature pass's plane A equals glrt_texture_albedo on the plane G of the same call, and lets the
denoiser keep a texture's edge.  Refusals leave the context rendering what it rendered."""
import functools

import numpy as np
import pytest

import texture_cases as tc
import texture_math as tm
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

N = 6
SEEDS = [host.frame_seed(0), host.frame_seed(1)]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    bad = (_bits(got) != _bits(ref)).any(-1)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} pixels differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[tuple(np.argwhere(bad)[0])].tolist()} vs {ref[tuple(np.argwhere(bad)[0])].tolist()}"


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _oracle(scene, params, seeds=SEEDS, **kw):
    ref, rays = None, 0
    for sd in seeds:
        ref, n = pt_oracle.render(scene, dict(params, seed=sd), accum=ref, **kw)
        rays += n
    return ref, rays


def _setup(d, scene, params, spheres=None, ext=0):
    d.set_variant(2); d.count_rays(True); d.set_extensions(ext)
    d.upload_scene(scene); d.upload_spheres(spheres); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _frames(d, params, seeds=SEEDS):
    d.clear(); d.reset_stats()
    for sd in seeds:
        d.render(dict(params, seed=sd))
    d.sync()
    return d.read_accum(), d.stats()


def _bind(scene, material, k=0):
    b = np.full(scene["mat"].reshape(-1, 18).shape[0], -1, np.int32)
    b[material] = k
    return b


def _cell_texture(albedo, fmt="rgba32f", filt="nearest", block=1):
    """albedo (n, n, 3): texel [j, i] of cell (column i, row j), each repeated block x block times."""
    return (np.repeat(np.repeat(albedo, block, 0), block, 1), fmt, "repeat", filt)


# ---- the two forms of the wall scene and the oracle's image of the per-cell one, computed once
@functools.lru_cache(maxsize=None)
def _wall(kind="float"):
    albedo = None
    code = None
    if kind == "srgb":
        code = np.random.default_rng(21).integers(40, 250, (N, N, 3), dtype=np.uint8)  # the bytes; the oracle scene's albedos are the table's words for them
        albedo = tm.SRGB[code.astype(np.int64)]
    tex_scene, params, wall = scenes.config_textured_wall(n=N, albedo=albedo)
    cell_scene, cell_params, cells = scenes.config_textured_wall(n=N, albedo=albedo, per_cell=True)
    # preconditions: a failure of either is a broken test
    assert np.array_equal(tex_scene["bvh"], cell_scene["bvh"]) and np.array_equal(_bits(wall["albedo"]), _bits(cells["albedo"]))
    ref, rays = _oracle(cell_scene, cell_params)
    grey, _ = _oracle(tex_scene, params)  # the one-material image: the wall's own param0
    differ = (_bits(ref) != _bits(grey)).any(-1).mean()
    assert differ >= 1.0 / 3.0, f"the per-cell image differs from the one-material image on {differ:.0%} of the pixels: the comparison would not see the albedo"
    return tex_scene, params, wall, cell_scene, ref, rays, code


# ---- 1. the lookup
def test_lookup_kernel_equals_the_host_statement(gpu_device):
    tex, which, st = tc.batch()
    got = device.debug_texture_lookup(tex, which, st)
    ref = host.texture_lookup(tex, which, st)
    bad = (_bits(got) != _bits(ref)).any(1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} lookups differ; first: texture {which[bad][0]} {tex[which[bad][0]][1:]} at {st[bad][0].tolist()}: " \
                          f"{got[bad][0].tolist()} vs {ref[bad][0].tolist()}"


# ---- 2. a constant texture is the material
def test_constant_texture_renders_the_plain_scene(dev):
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    red = b.add_material(scenes.diffuse((0.8, 0.3, 0.3)))
    cu = b.add_material(scenes.conductor(scenes.COPPER["eta"], scenes.COPPER["kappa"], 0.2))
    lamp = b.add_material(scenes.emitter((10.0, 10.0, 10.0)))
    grey2 = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))  # c1 with the grey sphere's material apart from the ground's
    b.add_mesh(*scenes.quad((-10, 0, 10), (20, 0, 0), (0, 0, -20)), grey)
    b.add_mesh(*scenes.icosphere(1, 1.0, (-2.2, 1.0, 0.0)), red)
    b.add_mesh(*scenes.icosphere(1, 1.0, (0.0, 1.0, 0.0)), cu)
    b.add_mesh(*scenes.icosphere(1, 1.0, (2.2, 1.0, 0.0)), grey2)
    b.add_mesh(*scenes.quad((-1, 5, -1), (2, 0, 0), (0, 0, 2)), lamp)
    scene = b.build()
    c1, params = scenes.config_c1(64, 64, max_depth=4, n_samples=2, subdiv=1)
    assert np.array_equal(scene["vert"], c1["vert"]) and not scene["vert"].reshape(-1, 5, 3)[:, 2].any()  # c1's geometry, all coordinates 0
    ref, rays = _oracle(scene, params)
    c = np.float32(0.7)
    tex = [(np.full((1, 1, 3), c, np.float32), "rgba32f", "clamp", "bilinear"), (np.full((4, 4, 3), c, np.float32), "rgba32f", "repeat", "bilinear")]
    bind = _bind(scene, grey, 0)
    bind[grey2] = 1
    _setup(dev, scene, params)
    dev.upload_textures(tex, bind)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and st.fallback_last == device.FALLBACK_EXTENSIONS and st.fallback_launches == 2
    _same(got, ref, "constant textures on c1")
    assert st.rays == rays


# ---- 3. a piecewise-constant texture is one material a cell
@pytest.mark.parametrize("form", ["nearest", "bilinear-blocks", "srgb"])
def test_piecewise_constant_texture_renders_the_per_cell_scene(dev, form):
    scene, params, wall, _, ref, rays, code = _wall("srgb" if form == "srgb" else "float")
    if form == "nearest":
        tex = _cell_texture(wall["albedo"])
    elif form == "bilinear-blocks":
        tex = _cell_texture(wall["albedo"], filt="bilinear", block=2)
    else:
        tex = _cell_texture(code, fmt="rgba8_srgb")
    _setup(dev, scene, params)
    dev.upload_textures([tex], _bind(scene, wall["material"]))
    got, st = _frames(dev, params)
    assert st.variant_last == 1
    _same(got, ref, form)
    assert st.rays == rays


# ---- 4. materials not staged in LDS
def test_beyond_the_lds_material_limit(dev):
    scene, params, wall, _, ref, rays, _ = _wall()
    pad = np.array([r for _ in range(300) for r in scenes._mat_rows(scenes.diffuse((0.3, 0.3, 0.3)))], np.float32)
    big = dict(scene, mat=np.concatenate([scene["mat"].reshape(-1, 3), pad], 0))
    assert big["mat"].shape[0] // 6 > 256
    _setup(dev, big, params)
    dev.upload_textures([_cell_texture(wall["albedo"], filt="bilinear", block=2)], _bind(big, wall["material"]))
    got, st = _frames(dev, params)
    _same(got, ref, "300 more materials")
    assert st.rays == rays


# ---- 5. next to the other extensions
def test_with_spheres_and_a_dielectric(dev):
    scene, params, wall, cell_scene, _, _, _ = _wall()
    glass = np.array(scenes._mat_rows(scenes.dielectric(1.5)), np.float32)

    def with_glass(s):
        return dict(s, mat=np.concatenate([s["mat"].reshape(-1, 3), glass], 0)), s["mat"].reshape(-1, 18).shape[0]

    tex_scene, g0 = with_glass(scene)
    ref_scene, g1 = with_glass(cell_scene)
    balls = lambda g: np.array([[-2.4, 0.8, 1.0, 0.8, g], [2.5, 1.0, 0.5, 1.0, 0]], np.float32)  # a glass ball and a grey one in front of the wall
    ref, rays = _oracle(ref_scene, params, spheres=balls(g1), ext_flags=device.EXT_DIELECTRIC)
    _setup(dev, tex_scene, params, spheres=balls(g0), ext=device.EXT_DIELECTRIC)
    dev.upload_textures([_cell_texture(wall["albedo"])], _bind(tex_scene, wall["material"]))
    got, st = _frames(dev, params)
    dev.set_extensions(0)
    _same(got, ref, "spheres + dielectric")
    assert st.rays == rays


# ---- 6. the feature pass
def _free_wall(bvh="sah"):
    rng = np.random.default_rng(17)
    uv = rng.uniform(-1.0, 2.0, (2 * N * N, 3, 2)).astype(np.float32)
    scene, params, wall = scenes.config_textured_wall(n=N, uv=uv, bvh=bvh)
    tex = [(tc.texels(5, 4, "rgba32f", 9), "rgba32f", "repeat", "bilinear")]
    return scene, params, wall, tex


@pytest.mark.parametrize("bvh", ["sah", "chain"])
def test_feature_plane_a_is_the_texture_albedo_of_plane_g(dev, monkeypatch, bvh):
    scene, params, wall, tex = _free_wall(bvh)
    bind = _bind(scene, wall["material"])
    _setup(dev, scene, params)
    dev.upload_textures(tex, bind)
    ref_n, ref_a, ref_g = host.render_features_geom(scene, params)
    on_wall = ref_a[..., 3].view(np.int32) == wall["material"]
    assert on_wall.mean() > 0.3
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        dev.track_motion(True)   # with G: the *_geom_tex kernels
        dev.render_features(params)
        n, a = dev.read_features()
        g = dev.read_features_geom()
        want = host.texture_albedo(scene, tex, bind, g)
        _same(a[..., :3], want, f"{bvh} compact={compact}: plane A against texture_albedo(plane G)")
        _same(g, ref_g, "plane G"); _same(n, ref_n, "plane N")
        assert np.array_equal(a[..., 3].view(np.int32), ref_a[..., 3].view(np.int32))  # the material id is unchanged
        assert not (a[on_wall][:, :3] == np.float32(0.5)).all(-1).any()                 # the texture, not param0
        dev.track_motion(False)  # without G: the *_tex kernels
        dev.render_features(params)
        _same(dev.read_features()[1][..., :3], want, f"{bvh} compact={compact}: plane A without G")
    monkeypatch.delenv("GLRTX_COMPACT_NODES")
    dev.upload_textures(None, None)
    dev.render_features(params)
    _same(dev.read_features()[1], ref_a, "unbound: plane A is the material's again")


def test_demodulation_keeps_a_texture_edge(dev):
    scene, params, wall = scenes.config_textured_wall(n=N, width=96, height=64, n_samples=4)
    ij = np.add.outer(np.arange(N), np.arange(N)) % 2
    checker = np.where(ij[..., None] == 0, np.float32(0.15), np.float32(0.85)) * np.ones(3, np.float32)
    _setup(dev, scene, params)
    dev.upload_textures([_cell_texture(checker.astype(np.float32))], _bind(scene, wall["material"]))
    clean, _ = _frames(dev, dict(params, n_samples=64), [host.frame_seed(10 + k) for k in range(4)])  # 256 spp
    clean = clean[..., :3] / clean[..., 3:]
    dev.render_features(params)
    a = dev.read_features()[1]
    on_wall = a[..., 3].view(np.int32) == wall["material"]
    step = on_wall[:, 1:] & on_wall[:, :-1] & (a[:, 1:, 0] != a[:, :-1, 0])  # a vertical edge of the checker between x and x + 1
    edge = np.zeros(on_wall.shape, bool)
    edge[:, 1:] |= step
    edge[:, :-1] |= step
    assert edge.sum() > 100
    _frames(dev, params, [host.frame_seed(3)])  # the 4-spp render
    err = {}
    for demodulate in (0, 1):
        dev.denoise(demodulate=demodulate)
        err[demodulate] = float(np.abs(dev.read_denoised()[..., :3] - clean)[edge].mean())
    print(f"mean |D - 256 spp| over {int(edge.sum())} edge pixels: demodulate=0 {err[0]:.5f}, demodulate=1 {err[1]:.5f}")
    assert err[1] < err[0], err


# ---- 7. geometry moves, the mapping stays
def test_update_vertices_moves_the_wall_and_keeps_the_mapping(dev):
    scene, params, wall, cell_scene, _, _, _ = _wall()
    moved = scene["vert"].reshape(-1, 5, 3).copy()
    moved[wall["vert"].start:wall["vert"].stop, 0, 0] += np.float32(0.5)
    moved[wall["vert"].start:wall["vert"].stop, 2, :2] = 0.0  # the update's own uv words are not read: the mapping is the upload's
    cell_moved = cell_scene["vert"].reshape(-1, 5, 3).copy()
    cell_moved[wall["vert"].start:wall["vert"].stop, 0, 0] += np.float32(0.5)
    ref_scene = dict(cell_scene, vert=cell_moved.reshape(-1, 3))
    ref_scene["bvh"] = host.refit_bvh(ref_scene["vert"], ref_scene["tri"], cell_scene["bvh"])
    ref, rays = _oracle(ref_scene, params)
    _setup(dev, scene, params)
    dev.upload_textures([_cell_texture(wall["albedo"])], _bind(scene, wall["material"]))
    dev.update_vertices(moved.reshape(-1, 15))
    got, st = _frames(dev, params)
    _same(got, ref, "after update_vertices")
    assert st.rays == rays


# ---- 8. call order and refusals
def test_call_order_and_refusals(dev):
    scene, params, wall, _, ref, rays, _ = _wall()
    tex = [_cell_texture(wall["albedo"])]
    bind = _bind(scene, wall["material"])
    n_mat = bind.size
    d = device.Device()
    try:
        with pytest.raises(device.GlrtxError, match="no scene uploaded"):
            d.upload_textures(tex, bind)
    finally:
        d.close()
    _setup(dev, scene, params)
    before, st0 = _frames(dev, params)
    assert st0.variant_last == 2
    dev.upload_textures(tex, bind)
    desc, blob = host.pack_textures(tex)

    def refused(words, textures=tex, binding=bind):
        with pytest.raises(device.GlrtxError, match=words) as e:
            dev.upload_textures(textures, binding)
        assert e.value.code == device.GLRTX_EINVAL
        got, st = _frames(dev, params)
        _same(got, ref, f"after the refusal '{words}'")
        assert st.variant_last == 1 and st.rays == rays

    def edited(**edit):
        e = desc.copy()
        for k, v in edit.items():
            e[k][0] = v
        return e, blob

    refused(f"{n_mat - 1} bindings, the scene has {n_mat} materials", binding=bind[:-1])
    refused(f"material {wall['material']} is bound to texture 1 of 1", binding=_bind(scene, wall["material"], 1))
    refused("material 0 is bound to texture -2", binding=_bind(scene, 0, -2))
    refused("material 2 is bound to texture 0 and is not diffuse", binding=_bind(scene, 2))  # the lamp
    refused("material 1 is bound to texture 0 and is not diffuse", binding=_bind(scene, 1))  # the conductor
    refused("texture 0: 0 x 6 texels", textures=edited(width=0))
    refused("texture 0: 6 x 16385 texels", textures=edited(height=16385))
    refused("texture 0: unknown format 3", textures=edited(format=3))
    refused("texture 0: unknown wrap mode", textures=edited(wrap_t=2))
    refused("texture 0: unknown filter 2", textures=edited(filter=2))
    refused("texture 0: offset 8 is not a multiple of 16", textures=edited(offset=8))
    refused("texture 0: its last texel lies past", textures=(desc, blob[:-16]))
    huge = np.zeros(9, host.TEXTURE_DTYPE)
    huge["width"], huge["height"], huge["format"] = 16384, 16384, host.TEX_RGBA8_UNORM  # nine textures over the same GiB of texels: 9 x 2^28 > 2^31 - 1
    import ctypes as C
    rc = dev.L.glrtx_upload_textures(dev.h, huge.ctypes.data, 9, blob.ctypes.data, 16384 * 16384 * 4, bind.ctypes.data_as(C.POINTER(C.c_int32)), n_mat)
    assert rc == device.GLRTX_EINVAL and b"more than 2^31 - 1 texels in total" in dev.L.glrtx_last_error(dev.h)  # (refused on the descriptors: no texel is read)
    got, st = _frames(dev, params)
    _same(got, ref, "after the refusal of 2^31 texels")
    assert st.variant_last == 1 and st.rays == rays
    # the wavefront kernel's calls refuse while a set is bound
    seeds = SEEDS
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.render_adaptive(params, seeds, 0.05)
    dev.track_moments(True)
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.render_moments(params, seeds)
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.render_adaptive_moments(params, seeds, 0.05)
    dev.track_moments(False)
    dev.track_cascades(True)
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.render_cascades(params, seeds)
    dev.track_cascades(False)
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.hit_histogram(params, scene["tri"].reshape(-1, 4).shape[0])
    got, st = _frames(dev, params)
    _same(got, ref, "after the refused calls")
    # a volume-only context with textures bound does not take the wavefront kernel's V form
    dev.set_volume_wavefront(True)
    got, st = _frames(dev, params)
    assert st.variant_last == 1
    dev.set_volume_wavefront(False)
    # n_tex = 0 unbinds
    dev.upload_textures(None, None)
    got, st = _frames(dev, params)
    assert st.variant_last == 2 and st.fallback_last == 0
    _same(got, before, "unbound")
    # upload_scene drops the set
    dev.upload_textures(tex, bind)
    dev.upload_scene(scene)
    got, st = _frames(dev, params)
    assert st.variant_last == 2
    _same(got, before, "after upload_scene")
