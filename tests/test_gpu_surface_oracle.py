"""Textures, cutouts and emission maps INSIDE triangles, pinned to the oracle (oracle/pt_oracle.c "surface hooks"; include/glrt_host.h "Surface context").
Every bit-exact render test that existed before this file uses textures that are constant over each triangle, so the render was blind to what tex_hit_st,
cut_accepts' (u, v) and emit_light_st return: u and v swapped, a wrong corner order, w0 formed in another order, an albedo that reaches only one of its two
reads, a shadow ray deciding a cutout with stale barycentrics -- all of them kept every pin green.  Here the n = 6 walls carry FREE corner coordinates
(uniform in [-1, 2]) and small random textures, so wrap seams, clamp regions, texel borders and both filters fall inside triangles, and the device's image is
compared bit for bit, and ray for ray, with the oracle rendered through its three hooks (tests/test_oracle_surface.py anchors those on the CPU).
Preconditions are asserted on the CPU oracle alone -- a failure of one is a broken test: the hooked image differs from the unhooked one on >= 1/3 of the
pixels, a cutout image from BOTH uniform decisions on >= 1/5 (and in its ray count), and every image of a varying texture from the image of the texture's
per-triangle-constant reduction (the texel at each triangle's centroid) on >= 1/5: without that the case would test nothing new.  DESIGN.md "Surface hooks of
the oracle" records the measured shares."""
import functools

import numpy as np
import pytest

import surface_cases as sc
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

F = np.float32
N = sc.N
FLAT = (np.tile(F([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear")
TEX_KERNEL = "pt_render_persistent (extensions, textures)"


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(d, scene, params, count=True, ext=0, spheres=None):
    d.set_variant(2); d.count_rays(count); d.set_extensions(ext); d.track_motion(False); d.set_texture_wavefront(False)
    d.upload_environment(None); d.upload_scene(scene); d.upload_spheres(spheres); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _frames(d, params, seeds=sc.SEEDS):
    d.clear(); d.reset_stats()
    for sd in seeds:
        d.render(dict(params, seed=sd))
    d.sync()
    return d.read_accum(), d.stats()


def _types(scene):
    return scene["mat"].reshape(-1, 18)[:, 0].astype(np.int32)


def _unshared(scene, wall):
    """precondition of with_uv / centroid_reduction: the wall's triangle t has the vertices 3t, 3t + 1, 3t + 2"""
    t = scene["tri"].reshape(-1, 4)[list(wall["tri"]), :3].astype(np.int64)
    assert np.array_equal(t.reshape(-1), np.arange(wall["vert"].start, wall["vert"].stop))


def _reduced(scene, params, wall, tex, kind, **kw):
    """The oracle's image under the per-triangle-constant reduction of `tex` on the wall"""
    uv, flat = sc.centroid_reduction(scene, wall["tri"], tex)
    red = sc.with_uv(scene, wall, uv)
    bind = sc.at(scene, wall["material"])
    if kind == "cut":
        return sc.hooked(red, params, red, [flat], cut=host.cutouts(bind.size, texture=bind, **kw))
    return sc.hooked(red, params, red, [flat], **{kind: bind})


# ============================================================ albedo inside triangles
ALBEDO_SEED = 17
ALBEDO_CASES = [(5, 4, fmt, filt, wrap) for fmt in ("rgba32f", "rgba8_unorm", "rgba8_srgb") for filt in ("nearest", "bilinear") for wrap in ("repeat", "clamp")] + \
               [(3, 7, "rgba32f", "bilinear", ("repeat", "clamp")), (3, 7, "rgba8_unorm", "nearest", ("clamp", "repeat")), (3, 7, "rgba8_srgb", "bilinear", "repeat"),
                (3, 7, "rgba32f", "nearest", "clamp"), (1, 1, "rgba32f", "bilinear", "repeat"), (1, 1, "rgba8_srgb", "nearest", "clamp")]


def _case_id(c):
    w, h, fmt, filt, wrap = c
    return f"{w}x{h}-{fmt}-{filt}-{wrap if isinstance(wrap, str) else '+'.join(wrap)}"


@functools.lru_cache(maxsize=None)
def _albedo_wall():
    scene, params, wall = scenes.config_textured_wall(n=N, uv=sc.free_uv(ALBEDO_SEED))
    assert (params["width"], params["height"], params["max_depth"], params["n_samples"]) == (64, 48, 4, 2)
    _unshared(scene, wall)
    return scene, params, wall, sc.oracle(scene, params)


@functools.lru_cache(maxsize=None)
def _albedo_ref(case):
    """(texture, oracle image, rays) of the wall under the case's texture, preconditions asserted"""
    scene, params, wall, plain = _albedo_wall()
    w, h, fmt, filt, wrap = case
    tex = sc.random_texture(w, h, fmt, wrap, filt, 100 + 10 * w + h)
    ref, rays = sc.hooked(scene, params, scene, [tex], material_texture=sc.at(scene, wall["material"]))
    unhooked = sc.share(ref, plain[0])
    assert unhooked >= 1.0 / 3.0, f"{_case_id(case)}: the hooked image differs from the unhooked one on {unhooked:.1%} of the pixels"
    inside = None
    if w * h > 1:  # (a 1 x 1 texture does not vary: it is its own reduction)
        inside = sc.share(ref, _reduced(scene, params, wall, tex, "material_texture")[0])
        assert inside >= 0.2, f"{_case_id(case)}: the image differs from the per-triangle reduction's on {inside:.1%} of the pixels"
    return tex, ref, rays, unhooked, inside


@pytest.mark.parametrize("case", ALBEDO_CASES, ids=_case_id)
def test_albedo_inside_triangles_on_the_megakernel(dev, case):
    scene, params, wall, _ = _albedo_wall()
    tex, ref, rays, _, _ = _albedo_ref(case)
    _setup(dev, scene, params)
    dev.upload_textures([tex], sc.at(scene, wall["material"]))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == TEX_KERNEL
    sc.same(got, ref, _case_id(case))
    assert st.rays == rays


@pytest.mark.parametrize("case", [ALBEDO_CASES[1], ALBEDO_CASES[6], ALBEDO_CASES[11]], ids=_case_id)
def test_albedo_inside_triangles_without_ray_counting(dev, case):
    scene, params, wall, _ = _albedo_wall()
    tex, ref, _, _, _ = _albedo_ref(case)
    _setup(dev, scene, params, count=False)
    dev.upload_textures([tex], sc.at(scene, wall["material"]))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == TEX_KERNEL
    sc.same(got, ref, _case_id(case))


@pytest.mark.parametrize("compact", ["0", "1"], ids=["nodes64", "compact"])
@pytest.mark.parametrize("case", [ALBEDO_CASES[2], ALBEDO_CASES[5], ALBEDO_CASES[11], ALBEDO_CASES[12]], ids=_case_id)
def test_albedo_inside_triangles_on_the_t_form(dev, monkeypatch, case, compact):
    monkeypatch.delenv("GLRTX_TEXTURE_WAVEFRONT", raising=False)
    monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
    scene, params, wall, _ = _albedo_wall()
    tex, ref, rays, _, _ = _albedo_ref(case)
    try:
        _setup(dev, scene, params)
        dev.upload_textures([tex], sc.at(scene, wall["material"]))
        dev.set_texture_wavefront(True)
        got, st = _frames(dev, params)
        assert st.variant_last == 2 and st.fallback_last == 0 and st.node_layout_last == int(compact), (st.variant_last, st.fallback_last, st.node_layout_last)
        sc.same(got, ref, f"T form, {_case_id(case)}, GLRTX_COMPACT_NODES={compact}")
        assert st.rays == rays
    finally:
        dev.set_texture_wavefront(False)


def test_albedo_inside_triangles_beyond_the_lds_material_limit(dev):
    scene, params, wall, _ = _albedo_wall()
    tex, ref, rays, _, _ = _albedo_ref(ALBEDO_CASES[3])
    pad = np.array([r for _ in range(300) for r in scenes._mat_rows(scenes.diffuse((0.3, 0.3, 0.3)))], F)
    big = dict(scene, mat=np.concatenate([scene["mat"].reshape(-1, 3), pad], 0))
    assert big["mat"].shape[0] // 6 > 256
    # precondition: materials nothing wears change no bit of the oracle's image
    sc.same(sc.hooked(big, params, big, [tex], material_texture=sc.at(big, wall["material"]))[0], ref, "the oracle with 300 more materials")
    _setup(dev, big, params)
    dev.upload_textures([tex], sc.at(big, wall["material"]))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == TEX_KERNEL
    sc.same(got, ref, "300 more materials")
    assert st.rays == rays


def _moved(scene, wall, dy):
    """(the scene with the wall lifted by dy and the refitted tree, the vertex records handed to update_vertices: their own uv words zeroed)"""
    v = scene["vert"].reshape(-1, 5, 3).copy()
    r = slice(wall["vert"].start, wall["vert"].stop)
    v[r, 0, 1] += F(dy)
    moved = dict(scene, vert=v.reshape(-1, 3))
    moved["bvh"] = host.refit_bvh(moved["vert"], moved["tri"], scene["bvh"])
    v = v.copy()
    v[r, 2, :2] = 0.0  # the update's own uv words are not read: the {s, t} tables are the upload's
    return moved, v.reshape(-1, 15)


def test_albedo_inside_triangles_after_a_vertex_update(dev):
    scene, params, wall, _ = _albedo_wall()
    case = ALBEDO_CASES[5]
    tex, still, _, _, _ = _albedo_ref(case)
    moved, records = _moved(scene, wall, 0.3)
    bind = sc.at(scene, wall["material"])
    ref, rays = sc.hooked(moved, params, scene, [tex], material_texture=bind)  # the moved geometry, the upload's coordinates
    assert sc.share(ref, still) >= 1.0 / 3.0 and sc.share(ref, sc.oracle(moved, params)[0]) >= 1.0 / 3.0  # preconditions: the move and the texture are seen
    _setup(dev, scene, params)
    dev.upload_textures([tex], bind)
    dev.update_vertices(records)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == TEX_KERNEL
    sc.same(got, ref, "after update_vertices, the refitted tree")
    assert st.rays == rays


def test_albedo_inside_triangles_beside_a_glass_ball(dev):
    scene, params, wall, _ = _albedo_wall()
    tex, _, _, _, _ = _albedo_ref(ALBEDO_CASES[9])
    glass = np.array(scenes._mat_rows(scenes.dielectric(1.5)), F)
    g = scene["mat"].reshape(-1, 18).shape[0]
    with_glass = dict(scene, mat=np.concatenate([scene["mat"].reshape(-1, 3), glass], 0))
    balls = np.array([[-2.4, 0.8, 1.0, 0.8, g], [2.5, 1.0, 0.5, 1.0, 0]], F)  # a glass ball and a grey one in front of the wall
    bind = sc.at(with_glass, wall["material"])
    ref, rays = sc.hooked(with_glass, params, with_glass, [tex], material_texture=bind, spheres=balls, ext_flags=device.EXT_DIELECTRIC)
    plain, _ = sc.oracle(with_glass, params, spheres=balls, ext_flags=device.EXT_DIELECTRIC)
    matte, _ = sc.hooked(with_glass, params, with_glass, [tex], material_texture=bind, spheres=balls)
    assert sc.share(ref, plain) >= 1.0 / 3.0 and sc.share(ref, matte) > 0.02  # preconditions: the texture is seen, and the glass matters
    try:
        _setup(dev, with_glass, params, ext=device.EXT_DIELECTRIC, spheres=balls)
        dev.upload_textures([tex], bind)
        got, st = _frames(dev, params)
        assert st.variant_last == 1 and dev.last_kernel() == TEX_KERNEL
        sc.same(got, ref, "spheres and EXT_DIELECTRIC")
        assert st.rays == rays
    finally:
        dev.set_extensions(0); dev.upload_spheres(None)


# ============================================================ cutouts inside triangles
CUT_SEED = 11
CUT_CASES = [("rgba32f", "nearest", 3), ("rgba32f", "bilinear", 3), ("rgba8_unorm", "bilinear", 3), ("rgba8_srgb", "nearest", 3), ("rgba32f", "bilinear", 0),
             ("rgba8_srgb", "nearest", 0)]


@functools.lru_cache(maxsize=None)
def _cut_wall():
    scene, params, wall = scenes.config_cutout_wall(n=N, uv=sc.free_uv(CUT_SEED))
    assert (params["width"], params["height"], params["max_depth"], params["n_samples"]) == (64, 48, 4, 2)
    _unshared(scene, wall)
    return scene, params, wall, sc.oracle(scene, params), sc.oracle(wall["collapsed"](list(wall["tri"])), params)


def _cut_texture(fmt, filt, channel):
    """alpha uniform in [0, 1]; for a cutout on channel 0 the red channel is made uniform in [0, 1] as well (sRGB: bytes whose decode is)"""
    arr, _, _, _ = sc.random_texture(5, 4, fmt, "repeat", filt, 300 + channel)
    if channel == 0:
        rng = np.random.default_rng(77)
        arr[..., 0] = rng.uniform(0.0, 1.0, arr.shape[:2]).astype(F) if fmt == "rgba32f" else rng.integers(120, 256, arr.shape[:2], dtype=np.uint8)
    return (arr, fmt, ("repeat", "clamp") if filt == "bilinear" else "repeat", filt)


def _cut_preconditions(what, ref, rays, plain, gone, reduced):
    a, b, c = sc.share(ref, plain[0]), sc.share(ref, gone[0]), sc.share(ref, reduced[0])
    assert min(a, b) >= 0.2, f"{what}: differs from the all-accepted image on {a:.1%} and from the all-rejected one on {b:.1%} of the pixels"
    assert rays != plain[1] and rays != gone[1], f"{what}: {rays} rays, all accepted {plain[1]}, all rejected {gone[1]}"
    assert c >= 0.2, f"{what}: differs from the per-triangle reduction's image on {c:.1%} of the pixels"
    return a, b, c


@functools.lru_cache(maxsize=None)
def _cut_ref(case):
    scene, params, wall, plain, gone = _cut_wall()
    fmt, filt, channel = case
    tex = _cut_texture(fmt, filt, channel)
    bind = sc.at(scene, wall["material"])
    cut = host.cutouts(bind.size, texture=bind, channel=channel, cutoff=0.5)
    ref, rays = sc.hooked(scene, params, scene, [tex], cut=cut)
    shares = _cut_preconditions(str(case), ref, rays, plain, gone, _reduced(scene, params, wall, tex, "cut", channel=channel, cutoff=0.5))
    return tex, cut, ref, rays, shares


@pytest.mark.parametrize("case", CUT_CASES, ids=lambda c: f"{c[0]}-{c[1]}-channel{c[2]}")
def test_holes_inside_triangles_path_rays_and_shadow_rays(dev, case):
    scene, params, wall, _, _ = _cut_wall()
    tex, cut, ref, rays, _ = _cut_ref(case)
    _setup(dev, scene, params)
    dev.upload_textures([tex], sc.none(scene))  # a set that binds no albedo at all
    dev.bind_cutouts(cut)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == "pt_render_persistent (extensions, textures, cutouts)"
    sc.same(got, ref, str(case))
    assert st.rays == rays


@pytest.mark.parametrize("env", [False, True], ids=["no-environment", "zero-environment"])
@pytest.mark.parametrize("maps", [False, True], ids=["no-maps", "flat-maps"])
def test_holes_inside_triangles_in_the_four_cut_forms(dev, maps, env):
    scene, params, wall, _, _ = _cut_wall()
    tex, cut, ref, rays, _ = _cut_ref(CUT_CASES[1])
    t, mat = _types(scene), scene["mat"].reshape(-1, 18)
    cu = int(np.flatnonzero(t == 3)[0])
    rough = (np.tile(F([mat[cu, 12], mat[cu, 13], 0.0]), (3, 3, 1)), "rgba32f", "clamp", "bilinear")  # exactly the ball's own alphas
    # the flat normal map goes on the floor and the ball, whose coordinates are all zero (det = 0 keeps the normal): the existing pins; the wall's free
    # coordinates would send a flat map through the tangent frame, which is not this file's subject
    normal = np.full(t.size, -1, np.int32)
    normal[[0, cu]] = 1
    assert t[0] == 2 and not scene["vert"].reshape(-1, 5, 3)[:wall["vert"].start, 2].any()
    _setup(dev, scene, params)
    dev.upload_textures([tex, FLAT, rough], sc.none(scene))
    try:
        if maps:
            dev.bind_material_maps(normal=normal, roughness=sc.at(scene, cu, 2))
        if env:
            dev.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape", scale=0.0))
        dev.bind_cutouts(cut)
        got, st = _frames(dev, params)
        name = "pt_render_persistent (extensions, " + ("environment, " if env else "") + "textures, " + ("maps, " if maps else "") + "cutouts)"
        assert st.variant_last == 1 and dev.last_kernel() == name
        sc.same(got, ref, name)
        assert st.rays == rays
    finally:
        dev.upload_environment(None)


def test_one_wall_textured_and_cut_with_both_hooks(dev):
    scene, params, wall, plain, gone = _cut_wall()
    albedo = sc.random_texture(3, 7, "rgba8_srgb", ("clamp", "repeat"), "bilinear", 5)
    alpha = _cut_texture("rgba32f", "bilinear", 3)
    bind = sc.at(scene, wall["material"], 0)
    cut = host.cutouts(bind.size, texture=sc.at(scene, wall["material"], 1), channel=3, cutoff=0.5)
    ref, rays = sc.hooked(scene, params, scene, [albedo, alpha], material_texture=bind, cut=cut)
    only_cut, only_cut_rays = sc.hooked(scene, params, scene, [albedo, alpha], cut=cut)
    only_albedo, _ = sc.hooked(scene, params, scene, [albedo, alpha], material_texture=bind)
    # preconditions: each hook is seen beside the other (the albedo changes no ray: its image shares the cut image's count)
    assert sc.share(ref, only_cut) >= 0.2 and sc.share(ref, only_albedo) >= 0.2 and rays == only_cut_rays and rays not in (plain[1], gone[1])
    _setup(dev, scene, params)
    dev.upload_textures([albedo, alpha], bind)
    dev.bind_cutouts(cut)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == "pt_render_persistent (extensions, textures, cutouts)"
    sc.same(got, ref, "albedo and cutout on one wall")
    assert st.rays == rays


def test_holes_inside_triangles_after_a_vertex_update(dev):
    scene, params, wall, _, _ = _cut_wall()
    tex, cut, still, _, _ = _cut_ref(CUT_CASES[2])
    moved, records = _moved(scene, wall, 0.3)
    ref, rays = sc.hooked(moved, params, scene, [tex], cut=cut)
    uncut, uncut_rays = sc.oracle(moved, params)
    assert sc.share(ref, still) >= 0.2 and sc.share(ref, uncut) >= 0.2 and rays != uncut_rays
    _setup(dev, scene, params)
    dev.upload_textures([tex], sc.none(scene))
    dev.bind_cutouts(cut)
    dev.update_vertices(records)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and "cutouts" in dev.last_kernel()
    sc.same(got, ref, "the moved wall with the refitted tree")
    assert st.rays == rays


# ============================================================ emission maps inside triangles
EMIT_SEED = 23
EMIT_KERNEL = "pt_render_persistent (extensions, textures, emission maps)"
EMIT_CASES = [(4, "rgba32f", "bilinear", "repeat"), (4, "rgba8_srgb", "nearest", "clamp"), (6, "rgba32f", "nearest", ("repeat", "clamp")), (6, "rgba8_unorm", "bilinear", "repeat")]


@functools.lru_cache(maxsize=None)
def _emit_wall(n):
    scene, params, wall = scenes.config_emissive_wall(n=n, uv=sc.free_uv(EMIT_SEED + n, n))
    assert (params["width"], params["height"], params["max_depth"], params["n_samples"]) == (64, 48, 4, 2)
    assert (scene["light"].reshape(-1, 4).shape[0] <= 64) == (n == 4)  # kMaxLdsLights: the light records in LDS, or read from global memory
    _unshared(scene, wall)
    return scene, params, wall, sc.oracle(scene, params)


@functools.lru_cache(maxsize=None)
def _emit_ref(case):
    n, fmt, filt, wrap = case
    scene, params, wall, plain = _emit_wall(n)
    tex = sc.random_texture(5, 4, fmt, wrap, filt, 500 + n)
    ref, rays = sc.hooked(scene, params, scene, [tex], material_emission=sc.at(scene, wall["material"]))
    unhooked, inside = sc.share(ref, plain[0]), sc.share(ref, _reduced(scene, params, wall, tex, "material_emission")[0])
    assert unhooked >= 1.0 / 3.0 and inside >= 0.2, f"{case}: differs from the unhooked image on {unhooked:.1%}, from the reduction's on {inside:.1%} of the pixels"
    assert rays == plain[1]  # an emission map changes no ray
    return tex, ref, rays, unhooked, inside


@pytest.mark.parametrize("case", EMIT_CASES, ids=lambda c: f"n{c[0]}-{c[1]}-{c[2]}")
def test_an_emission_map_varying_inside_the_lights_seen_and_sampled(dev, case):
    scene, params, wall, _ = _emit_wall(case[0])
    tex, ref, rays, _, _ = _emit_ref(case)
    _setup(dev, scene, params)
    dev.upload_textures([tex], sc.none(scene))
    dev.bind_emission_maps(sc.at(scene, wall["material"]))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == EMIT_KERNEL
    sc.same(got, ref, str(case))
    assert st.rays == rays


@pytest.mark.parametrize("maps, env", [(True, False), (False, True), (True, True)], ids=["flat-maps", "zero-environment", "flat-maps-zero-environment"])
def test_an_emission_map_varying_inside_the_lights_in_the_other_emit_forms(dev, maps, env):
    case = EMIT_CASES[0]
    scene, params, wall, _ = _emit_wall(case[0])
    tex, ref, rays, _, _ = _emit_ref(case)
    t, mat = _types(scene), scene["mat"].reshape(-1, 18)
    cu = int(np.flatnonzero(t == 3)[0])
    rough = (np.tile(F([mat[cu, 12], mat[cu, 13], 0.0]), (3, 3, 1)), "rgba32f", "clamp", "bilinear")  # exactly the ball's own alphas
    _setup(dev, scene, params)
    dev.upload_textures([tex, FLAT, rough], sc.none(scene))
    try:
        if maps:  # (the floor and the ball carry all-zero coordinates: a flat normal map keeps their normals, the existing pin)
            dev.bind_material_maps(normal=np.where((t == 2) | (t == 3), 1, -1), roughness=sc.at(scene, cu, 2))
        if env:
            dev.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape", scale=0.0))
        dev.bind_emission_maps(sc.at(scene, wall["material"]))
        got, st = _frames(dev, params)
        name = "pt_render_persistent (extensions, " + ("environment, " if env else "") + "textures, " + ("maps, " if maps else "") + "emission maps)"
        assert st.variant_last == 1 and dev.last_kernel() == name
        sc.same(got, ref, name)
        assert st.rays == rays
    finally:
        dev.upload_environment(None)


def test_an_emission_map_varying_inside_the_lights_after_the_lift(dev):
    case = EMIT_CASES[1]
    scene, params, wall, _ = _emit_wall(case[0])
    tex, still, _, _, _ = _emit_ref(case)
    moved, records = _moved(scene, wall, 0.3)
    bind = sc.at(scene, wall["material"])
    ref, rays = sc.hooked(moved, params, scene, [tex], material_emission=bind)
    assert sc.share(ref, still) >= 1.0 / 3.0 and sc.share(ref, sc.oracle(moved, params)[0]) >= 1.0 / 3.0
    _setup(dev, scene, params)
    dev.upload_textures([tex], sc.none(scene))
    dev.bind_emission_maps(bind)
    dev.update_vertices(records)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == EMIT_KERNEL
    sc.same(got, ref, "the lifted wall with the refitted tree")
    assert st.rays == rays


@functools.lru_cache(maxsize=None)
def _panel():
    scene, params, panel = scenes.config_emissive_panel(split=False, n_samples=2)
    assert (params["width"], params["height"], params["max_depth"], params["n_samples"]) == (64, 48, 4, 2)
    tex = (F([[[1.0, 1.0, 1.0], [0.1, 0.1, 0.1]]]), "rgba32f", "clamp", "nearest")  # 2 x 1: the left texel 1, the right 0.1
    bind = sc.at(scene, panel["material"])
    ref, rays = sc.hooked(scene, params, scene, [tex], material_emission=bind)
    plain = sc.oracle(scene, params)
    # the panel's two triangles: vertices 6 .. 11 behind the floor's six
    wall = dict(tri=range(2, 4), vert=range(6, 12), material=panel["material"])
    _unshared(scene, wall)
    unhooked, inside = sc.share(ref, plain[0]), sc.share(ref, _reduced(scene, params, wall, tex, "material_emission")[0])
    assert unhooked >= 1.0 / 3.0 and inside >= 0.2, f"the panel: differs from the unhooked image on {unhooked:.1%}, from the reduction's on {inside:.1%} of the pixels"
    return scene, params, tex, bind, ref, rays, unhooked, inside


def test_the_panel_under_its_two_texel_map_exactly(dev):
    """The scene of test_gpu_emission.py's 4 se check (a 2 x 1 map that varies inside the panel's two light triangles), here bit for bit"""
    scene, params, tex, bind, ref, rays, _, _ = _panel()
    _setup(dev, scene, params)
    dev.upload_textures([tex], sc.none(scene))
    dev.bind_emission_maps(bind)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == EMIT_KERNEL
    sc.same(got, ref, "the panel")
    assert st.rays == rays
