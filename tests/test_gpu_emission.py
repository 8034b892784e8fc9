"""Emission maps on the GPU (csrc/texture.hip.h: emit_light_st, emit_radiance; csrc/pt_kernel.hip.h: shade_core<.., EMIT>; include/glrtx.h "Emission maps").
The sampled-side statement's kernel equals the CPU statement bit for bit on the CPU test's cases.  The feature is pinned THROUGH the reference: an emission map
that is constant over each cell of the emitter wall renders, bit for bit and count for count, the oracle's image of the same triangles with one emitter material
a cell (emission = float32(e * texel)) -- with the light records in LDS (34 lights) and in global memory (74), in three texture forms, beside a zero
environment and flat maps (the four EMIT forms of the megakernel), after a vertex update, and behind a glass ball (the emission a specular path meets).
Bindings of -1 and unbinding change nothing; plane A carries the emitter's picture; refusals leave the context rendering what it rendered; and a texture that
varies INSIDE a light triangle lights the floor as the same panel split into two constant emitters does, within the split scene's own noise."""
import functools

import numpy as np
import pytest

import emission_cases
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

F = np.float32
SEEDS = [host.frame_seed(0), host.frame_seed(1)]
FLAT = (np.tile(F([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear")
EMIT = "pt_render_persistent (extensions, textures, emission maps)"


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


def _oracle(scene, params, seeds=SEEDS, ext_flags=0):
    ref, rays = None, 0
    for sd in seeds:
        ref, n = pt_oracle.render(scene, dict(params, seed=sd), accum=ref, ext_flags=ext_flags)
        rays += n
    return ref, rays


def _setup(d, scene, params, ext=0):
    d.set_variant(2); d.count_rays(True); d.set_extensions(ext); d.track_motion(False); d.set_texture_wavefront(False)
    d.upload_environment(None); d.upload_scene(scene); d.upload_spheres(None); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _frames(d, params, seeds=SEEDS):
    d.clear(); d.reset_stats()
    for sd in seeds:
        d.render(dict(params, seed=sd))
    d.sync()
    return d.read_accum(), d.stats()


def _types(scene):
    return scene["mat"].reshape(-1, 18)[:, 0].astype(np.int32)


def _none(scene):
    return np.full(_types(scene).size, -1, np.int32)


def _at(scene, material, k):
    a = _none(scene)
    a[material] = k
    return a


# ---- 1. the sampled-side statement's kernel
def test_debug_light_emission_equals_the_host_statement(dev):
    scene, tex, bind, lid, u = emission_cases.case()
    ref = host.light_emission(scene, tex, bind, lid, u)
    dev.upload_environment(None); dev.upload_scene(scene); dev.upload_textures(tex, _none(scene))
    with pytest.raises(device.GlrtxError, match="no emission maps are bound"):
        dev.debug_light_emission(lid, u)
    dev.bind_emission_maps(bind)
    got = device.debug_light_emission(dev, lid, u)
    bad = ((_bits(got) != _bits(ref)) & ~(np.isnan(got) & np.isnan(ref))).any(-1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} samples differ; first {np.flatnonzero(bad)[0]}: {got[bad][0].tolist()} vs {ref[bad][0].tolist()}"
    with pytest.raises(device.GlrtxError, match=f"names light {scene['light'].reshape(-1, 4).shape[0]} of"):
        dev.debug_light_emission([scene["light"].reshape(-1, 4).shape[0]], [[0.5, 0.25]])


# ---- 2. the pin through the reference
def _texture(form, n, seed=3):
    """The emission map of an n x n wall in one of the three forms: constant over each cell at the cell's centre."""
    rng = np.random.default_rng(seed)
    if form == "rgba32f-nearest":
        return (rng.uniform(0.1, 0.9, (n, n, 3)).astype(F), "rgba32f", "repeat", "nearest")
    b = rng.integers(26, 231, (n, n, 3), dtype=np.uint8)
    if form == "rgba8-bilinear-blocks":  # 2 x 2 equal texels a cell, looked up at the block's centre: four equal texels give the texel exactly
        return (np.repeat(np.repeat(b, 2, 0), 2, 1), "rgba8_unorm", "clamp", "bilinear")
    assert form == "rgba8-srgb"
    return (b, "rgba8_srgb", "repeat", "nearest")


@functools.lru_cache(maxsize=None)
def _pin(n, form, ball="conductor", ext=0):
    """(scene, params, wall, texture, oracle image and rays of the per-cell scene)"""
    tex = _texture(form, n)
    centres = np.array([[(i + 0.5) / n, (j + 0.5) / n] for j in range(n) for i in range(n)], F)
    texel = host.texture_lookup([tex], np.zeros(n * n, np.int32), centres).reshape(n, n, 3)  # the CPU statement's value of every cell
    scene, params, wall = scenes.config_emissive_wall(n=n, texel=texel, ball=ball)
    cells, _, _ = scenes.config_emissive_wall(n=n, texel=texel, ball=ball, per_cell=True)
    # preconditions: a failure of any is a broken test
    assert scene["light"].reshape(-1, 4).shape[0] == 2 + 2 * n * n
    assert np.array_equal(scene["bvh"], cells["bvh"]) and np.array_equal(scene["light"][:, :3], cells["light"][:, :3])
    assert np.array_equal(scene["vert"].reshape(-1, 5, 3)[:, :2], cells["vert"].reshape(-1, 5, 3)[:, :2])
    ref, rays = _oracle(cells, params, ext_flags=ext)
    plain, _ = _oracle(scene, params, ext_flags=ext)  # the wall with its plain emission: what a missing lookup would render
    differ = (_bits(ref) != _bits(plain)).any(-1).mean()
    assert differ >= 0.5, f"the per-cell image differs from the plain emitter's on {differ:.1%} of the pixels: the comparison would not see the map"
    return scene, params, wall, tex, cells, ref, rays


def _counts_of(dev, cells, params, ext=0):
    """rays_untraced and paths of the per-cell scene on the device's own untextured kernels"""
    _setup(dev, cells, params, ext)
    _, st = _frames(dev, params)
    return st.rays, st.rays_untraced, st.paths


@pytest.mark.parametrize("n, form", [(4, "rgba32f-nearest"), (4, "rgba8-bilinear-blocks"), (4, "rgba8-srgb"), (6, "rgba32f-nearest"), (6, "rgba8-srgb")])
def test_a_map_constant_over_each_cell_renders_the_per_cell_scene(dev, n, form):
    scene, params, wall, tex, cells, ref, rays = _pin(n, form)
    counts = _counts_of(dev, cells, params)
    assert counts[0] == rays
    _setup(dev, scene, params)
    assert (scene["light"].reshape(-1, 4).shape[0] <= 64) == (n == 4)  # kMaxLdsLights: the light records in LDS, or read from global memory
    dev.upload_textures([tex], _none(scene))  # a set that binds no albedo at all
    dev.bind_emission_maps(_at(scene, wall["material"], 0))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == EMIT
    _same(got, ref, f"n={n}, {form}")
    assert (st.rays, st.rays_untraced, st.paths) == counts


@pytest.mark.parametrize("maps, env", [(True, False), (False, True), (True, True)], ids=["flat-maps", "zero-environment", "flat-maps-zero-environment"])
def test_beside_flat_maps_and_a_zero_environment(dev, maps, env):
    scene, params, wall, tex, cells, ref, rays = _pin(4, "rgba32f-nearest")
    counts = _counts_of(dev, cells, params)
    t, mat = _types(scene), scene["mat"].reshape(-1, 18)
    cu = int(np.flatnonzero(t == 3)[0])
    rough = (np.tile(F([mat[cu, 12], mat[cu, 13], 0.0]), (3, 3, 1)), "rgba32f", "clamp", "bilinear")  # exactly the ball's own alphas
    _setup(dev, scene, params)
    dev.upload_textures([tex, FLAT, rough], _none(scene))
    try:
        if maps:  # the existing pins: a flat normal map and a roughness map of the material's own alphas change no bit
            dev.bind_material_maps(normal=np.where((t == 2) | (t == 3), 1, -1), roughness=_at(scene, cu, 2))
        if env:  # ... and neither does an environment of scale 0 in escape mode
            dev.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape", scale=0.0))
        dev.bind_emission_maps(_at(scene, wall["material"], 0))
        got, st = _frames(dev, params)
        name = "pt_render_persistent (extensions, " + ("environment, " if env else "") + "textures, " + ("maps, " if maps else "") + "emission maps)"
        assert st.variant_last == 1 and dev.last_kernel() == name
        _same(got, ref, name)
        assert (st.rays, st.rays_untraced, st.paths) == counts
    finally:
        dev.upload_environment(None)


def test_the_bindings_survive_a_vertex_update(dev):
    scene, params, wall, tex, cells, _, _ = _pin(4, "rgba32f-nearest")
    r = slice(wall["vert"].start, wall["vert"].stop)

    def lifted(s, zero_uv):
        v = s["vert"].reshape(-1, 5, 3).copy()
        v[r, 0, 1] += F(0.3)  # the wall lifted by 0.3
        if zero_uv:
            v[r, 2, :2] = 0.0  # the update's own uv words are not read: light_st and the {s, t} table are the upload's
        m = dict(s, vert=v.reshape(-1, 3))
        m["bvh"] = host.refit_bvh(m["vert"], m["tri"], s["bvh"])
        return m, v

    moved_cells, _ = lifted(cells, False)
    moved_scene, moved = lifted(scene, True)
    assert np.array_equal(moved_cells["bvh"], moved_scene["bvh"])
    ref, rays = _oracle(moved_cells, params)
    _setup(dev, scene, params)
    dev.upload_textures([tex], _none(scene))
    dev.bind_emission_maps(_at(scene, wall["material"], 0))
    dev.update_vertices(moved.reshape(-1, 15))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == EMIT
    _same(got, ref, "the moved wall with the refitted tree")
    assert st.rays == rays


def test_behind_glass_the_specular_path_meets_the_map(dev):
    ext = device.EXT_DIELECTRIC
    scene, params, wall, tex, cells, ref, rays = _pin(4, "rgba8-srgb", "glass", ext)
    matte, _ = _oracle(cells, params)  # without the extension the ball is black: the glass must matter
    assert (_bits(ref) != _bits(matte)).any(-1).mean() > 0.02
    counts = _counts_of(dev, cells, params, ext)
    assert counts[0] == rays
    _setup(dev, scene, params, ext)
    dev.upload_textures([tex], _none(scene))
    dev.bind_emission_maps(_at(scene, wall["material"], 0))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == EMIT
    _same(got, ref, "EXT_DIELECTRIC, a glass ball in front of the panel")
    assert (st.rays, st.rays_untraced, st.paths) == counts
    dev.set_extensions(0)


# ---- 3. bindings of -1, and unbinding
def test_nothing_bound_and_unbinding_change_nothing(dev):
    scene, params, wall, tex, _, _, _ = _pin(4, "rgba32f-nearest")
    alb = _at(scene, 0, 0)  # the floor textured, so that the TEX form has something to do
    _setup(dev, scene, params)
    dev.upload_textures([tex], alb)
    before, st0 = _frames(dev, params)
    old = dev.last_kernel()
    assert st0.variant_last == 1 and old == "pt_render_persistent (extensions, textures)"
    dev.bind_emission_maps(_none(scene))
    got, st = _frames(dev, params)
    assert dev.last_kernel() == EMIT and st.variant_last == 1
    _same(got, before, "every material bound to -1")
    assert (st.rays, st.rays_untraced, st.paths) == (st0.rays, st0.rays_untraced, st0.paths)
    dev.bind_emission_maps(_at(scene, wall["material"], 0))
    lit, _ = _frames(dev, params)
    assert (_bits(lit) != _bits(before)).any(-1).mean() > 0.5  # the binding matters
    dev.bind_emission_maps()
    got, st = _frames(dev, params)
    assert dev.last_kernel() == old and st.variant_last == 1
    _same(got, before, "after unbinding")
    assert (st.rays, st.rays_untraced, st.paths) == (st0.rays, st0.rays_untraced, st0.paths)


# ---- 4. the feature pass
def test_plane_a_carries_the_emitters_picture(dev, monkeypatch):
    scene, params, wall = scenes.config_emissive_wall(n=4, uv="corner")
    rng = np.random.default_rng(17)
    tex = [(rng.uniform(0.0, 1.0, (5, 7, 4)).astype(F), "rgba32f", "clamp", "bilinear"), (rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear")]
    alb, emi = _at(scene, 0, 1), _at(scene, wall["material"], 0)
    emi[0] = 0  # the diffuse floor bound as well: it keeps its albedo rule
    ref_n, un_a, ref_g = host.render_features_geom(scene, params)
    ref_a = un_a.copy()
    ref_a[..., :3] = host.emission_albedo(scene, tex, alb, emi, ref_g)
    tex_a = un_a.copy()
    tex_a[..., :3] = host.texture_albedo(scene, tex, alb, ref_g)
    on_wall = np.isin(ref_g[..., 0].view(np.int32), np.asarray(list(wall["tri"])))
    assert on_wall.sum() > 300 and len(np.unique(_bits(ref_a[on_wall][:, :3]), axis=0)) > 100  # the picture varies inside the triangles
    _setup(dev, scene, params)
    dev.upload_textures(tex, alb)
    dev.bind_emission_maps(emi)
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        dev.track_motion(True)
        dev.render_features(params)
        n, a = dev.read_features()
        _same(dev.read_features_geom(), ref_g, f"compact={compact}: plane G"); _same(a, ref_a, f"compact={compact}: plane A"); _same(n, ref_n, f"compact={compact}: plane N")
        dev.track_motion(False)
        dev.render_features(params)
        n, a = dev.read_features()
        _same(a, ref_a, f"compact={compact}: plane A without G"); _same(n, ref_n, f"compact={compact}: plane N without G")
    monkeypatch.delenv("GLRTX_COMPACT_NODES")
    dev.bind_emission_maps()  # unbound: the kernels the pass ran before
    dev.render_features(params)
    n, a = dev.read_features()
    _same(a, tex_a, "unbound: plane A")


# ---- 5. routing and refusals
def test_routing_and_refusals(dev):
    scene, params, wall, tex, cells, ref, rays = _pin(4, "rgba32f-nearest")
    n_mat = _types(scene).size
    w = wall["material"]
    good = _at(scene, w, 0)
    d = device.Device()
    try:
        with pytest.raises(device.GlrtxError, match="glrtx_bind_emission_maps: no scene uploaded"):
            d.bind_emission_maps(good)
        d.upload_scene(scene)
        with pytest.raises(device.GlrtxError, match="no texture set is bound"):
            d.bind_emission_maps(good)
        b = scenes.SceneBuilder()
        b.add_mesh(*scenes.quad((-1, 0, 1), (2, 0, 0), (0, 0, -2)), b.add_material(scenes.emitter((1.0, 1.0, 1.0))))
        b.add_mesh(*scenes.box((-1, 0, -1), (1, 2, 1)), b.add_material(scenes.media()))
        d.upload_scene(b.build())
        d.upload_textures([tex], [-1, -1])
        with pytest.raises(device.GlrtxError, match="material 1 has an emission map and is a medium"):
            d.bind_emission_maps([0, 0])
        d.bind_emission_maps([0, -1])
    finally:
        d.close()
    _setup(dev, scene, params)
    dev.upload_textures([tex], _none(scene))
    dev.set_texture_wavefront(True)
    before, st0 = _frames(dev, params)  # the T form, before the bind
    assert st0.variant_last == 2
    dev.bind_emission_maps(good)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and st.fallback_last & device.FALLBACK_EXTENSIONS and dev.last_kernel() == EMIT  # the switch does not take emission maps
    _same(got, ref, "bound, with the texture wavefront switch on")
    assert st.rays == rays

    def still_lit(what):
        got, st = _frames(dev, params)
        _same(got, ref, f"after the refusal '{what}'")
        assert st.variant_last == 1 and st.rays == rays

    with pytest.raises(device.GlrtxError, match="textures are bound.*emission maps are bound"):
        dev.render_adaptive(params, SEEDS, 0.05)
    still_lit("render_adaptive")
    with pytest.raises(device.GlrtxError, match="textures are bound.*emission maps are bound"):
        dev.hit_histogram(params, scene["tri"].reshape(-1, 4).shape[0])
    still_lit("hit_histogram")
    for track, call in ((dev.track_moments, dev.render_moments), (dev.track_cascades, dev.render_cascades)):
        track(True)
        with pytest.raises(device.GlrtxError, match="textures are bound.*emission maps are bound"):
            call(params, SEEDS)
        track(False)
        still_lit(call.__name__)

    def refused(words, bind):
        with pytest.raises(device.GlrtxError, match=words) as e:
            dev.bind_emission_maps(bind)
        assert e.value.code == device.GLRTX_EINVAL
        still_lit(words)

    refused(f"{n_mat - 1} bindings, the scene has {n_mat} materials", good[:-1])
    refused(f"material {w}: emission map 1 of 1 textures", _at(scene, w, 1))
    refused(f"material {w}: emission map -2 of 1 textures", _at(scene, w, -2))
    with pytest.raises(device.GlrtxError, match="emission maps are bound") as e:
        dev.bind_cutouts(texture=_at(scene, 0, 0))
    assert e.value.code == device.GLRTX_EINVAL
    still_lit("bind_cutouts")
    # beside the volume: refused at render time, and nothing has changed afterwards
    dens, temp = scenes.fire_grids()
    dev.upload_volume(dens, temp, (-1.0, 0.0, -1.0), (1.0, 2.0, 1.0))
    dev.set_extensions(device.EXT_VOLUME)
    with pytest.raises(device.GlrtxError, match="GLRTX_EXT_VOLUME is set and emission maps are bound"):
        dev.render(dict(params, seed=SEEDS[0]))
    dev.set_extensions(0)
    dev.upload_volume(None, None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    still_lit("the volume")
    # cutouts first: the binding call names them
    dev.bind_emission_maps()
    dev.bind_cutouts(texture=_at(scene, 0, 0))
    with pytest.raises(device.GlrtxError, match="glrtx_bind_emission_maps: cutouts are bound"):
        dev.bind_emission_maps(good)
    dev.bind_cutouts()
    # after unbinding the T form runs again and equals its image from before the bind
    got, st = _frames(dev, params)
    assert st.variant_last == 2 and st.fallback_last == 0
    _same(got, before, "unbound: the T form's image from before the bind")
    # upload_textures drops the bindings, and so does upload_scene
    dev.bind_emission_maps(good)
    dev.upload_textures([tex], _none(scene))
    got, st = _frames(dev, params)
    assert st.variant_last == 2
    _same(got, before, "after upload_textures")
    dev.bind_emission_maps(good)
    dev.upload_scene(scene)
    got, st = _frames(dev, params)
    assert st.variant_last == 2
    with pytest.raises(device.GlrtxError, match="no texture set is bound"):
        dev.bind_emission_maps(good)
    dev.set_texture_wavefront(False)


# ---- 6. a texture that varies inside a light triangle
S, FRAMES = 8, 32


def _floor_block(scene, params, panel):
    """A block of floor pixels on the image's left half (the bright half's side: a mirrored lookup would show), all of which see the floor"""
    _, a, _ = host.render_features_geom(scene, params)
    floor = a[..., 3].view(np.int32) == panel["floor"]
    cols = slice(params["width"] // 8, params["width"] // 2 - 2)
    rows = np.flatnonzero(floor[:, cols].all(1))
    assert rows.size >= 8, rows
    return rows, cols


def _block_mean(img, rows, cols):
    return float((img[rows][:, cols, :3] / img[rows][:, cols, 3:4]).mean())


def within_four_standard_errors(value, others):
    """|value - mean(others)| <= 4 se, se = std(others, ddof 1) * sqrt(1 + 1 / len(others)): the standard error of the difference between ONE render's block
    mean and the mean of len(others) independent renders of the same expectation, estimated from those renders alone."""
    others = np.asarray(others, np.float64)
    se = others.std(ddof=1) * np.sqrt(1.0 + 1.0 / others.size)
    return abs(value - others.mean()) <= 4.0 * se, (value - others.mean()) / se


def test_a_texture_varying_inside_a_light_triangle_lights_the_floor_as_the_split_panel_does(dev):
    """Measured on the MI355X (DESIGN.md "Emission maps"): see the figures recorded there."""
    split, params, panel_s = scenes.config_emissive_panel(split=True)
    one, _, panel = scenes.config_emissive_panel(split=False)
    rows, cols = _floor_block(split, params, panel_s)
    rows1, cols1 = _floor_block(one, params, panel)
    assert np.array_equal(rows, rows1) and cols == cols1
    _setup(dev, split, params)
    means = []
    for s in range(S):
        img, _ = _frames(dev, params, [host.frame_seed(FRAMES * s + f) for f in range(FRAMES)])
        means.append(_block_mean(img, rows, cols))
    _setup(dev, one, params)
    tex = (F([[[1.0, 1.0, 1.0], [0.1, 0.1, 0.1]]]), "rgba32f", "clamp", "nearest")  # 2 x 1: the left texel 1, the right 0.1
    dev.upload_textures([tex], _none(one))
    seeds = [host.frame_seed(FRAMES * S + f) for f in range(FRAMES)]
    plain, _ = _frames(dev, params, seeds)  # the panel at its full emission everywhere: what a missing lookup would give
    dev.bind_emission_maps(_at(one, panel["material"], 0))
    img, st = _frames(dev, params, seeds)
    assert dev.last_kernel() == EMIT
    got = _block_mean(img, rows, cols)
    ok, z = within_four_standard_errors(got, means)
    ok_plain, z_plain = within_four_standard_errors(_block_mean(plain, rows, cols), means)
    print(f"split panel: block mean {np.mean(means):.6f}, std of {S} renders {np.std(means, ddof=1):.6f}; textured {got:.6f} ({z:+.2f} se); untextured {z_plain:+.2f} se")
    assert not ok_plain, "the untextured panel passes the criterion: the comparison would not see the map"
    assert ok, f"the textured panel's floor block mean {got} lies {z:+.2f} standard errors from the split panel's {np.mean(means)}"
