"""Alpha cutouts on the GPU (csrc/texture.hip.h: tex_lookup_channel, cut_accepts; csrc/pt_kernel.hip.h: trav_step<.., CUT>; include/glrtx.h "Cutouts").  The
one-channel lookup's kernel equals the CPU statement bit for bit on the CPU test's batch.  The alpha test is pinned THROUGH the reference: a rejected candidate
leaves the traversal as if that piece of surface did not exist, so a cutout texture that is constant over each wall triangle renders, bit for bit and ray for
ray, the oracle's image of the same five buffers -- the same `bvh` array included -- with the rejected triangles collapsed to a point (det = 0: never hit).
All accepted is the plain scene, all rejected the scene without its wall; flat maps and a zero environment beside the cutouts change nothing, in each of the
four CUT forms of the megakernel; the feature planes follow the holes inside triangles, as the CPU statement does; the records survive a vertex update;
refusals leave the context rendering what it rendered, and after unbinding everything routes as before."""
import functools

import numpy as np
import pytest

import texture_cases
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

N = 6
F = np.float32
SEEDS = [host.frame_seed(0), host.frame_seed(1)]
FLAT = (np.tile(F([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear")
_J, _I = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
CUT_CELLS = (_I + _J) % 2 == 0  # [row j, column i]: the cells the checkerboard removes -- 18 cells, 36 triangles
CHECKER = np.where(CUT_CELLS, 0.0, 1.0).astype(F)  # the texel of cell (i, j): 0 where (i + j) % 2 == 0, 1 elsewhere


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


def _oracle(scene, params, seeds=SEEDS):
    ref, rays = None, 0
    for sd in seeds:
        ref, n = pt_oracle.render(scene, dict(params, seed=sd), accum=ref)
        rays += n
    return ref, rays


def _setup(d, scene, params, count=True):
    d.set_variant(2); d.count_rays(count); d.set_extensions(0); d.track_motion(False); d.set_texture_wavefront(False)
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


# ---- 1. the lookup kernel
@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_channel_kernel_equals_the_host_statement(gpu_device, channel):
    tex, which, st = texture_cases.batch()
    got, ref = device.debug_texture_channel(tex, which, channel, st), host.texture_channel(tex, which, channel, st)
    bad = (_bits(got) != _bits(ref)) & ~(np.isnan(got) & np.isnan(ref))
    assert not bad.any(), f"channel {channel}: {int(bad.sum())} of {bad.size} lookups differ; first {np.flatnonzero(bad)[0]}: {got[bad][0]!r} vs {ref[bad][0]!r}"


# ---- 2. the pin through the reference
@functools.lru_cache(maxsize=None)
def _checker_wall():
    scene, params, wall = scenes.config_cutout_wall(n=N)
    cut_tris = wall["cell_tris"](CUT_CELLS)
    collapsed = wall["collapsed"](cut_tris)
    # preconditions: a failure of either is a broken test
    assert len(cut_tris) == 36 and np.array_equal(scene["bvh"], collapsed["bvh"])
    for k in ("tri", "mat", "light"):
        assert np.array_equal(scene[k], collapsed[k])
    ref, rays = _oracle(collapsed, params)
    full, full_rays = _oracle(scene, params)
    differ = (_bits(ref) != _bits(full)).any(-1).mean()
    assert differ >= 1.0 / 3.0, f"the collapsed image differs from the full wall's on {differ:.1%} of the pixels: the comparison would not see the cutouts"
    assert rays != full_rays
    return scene, params, wall, ref, rays, full, full_rays


def _checker_texture(form):
    """(texture, channel): the checkerboard in the form's format and channel; every other channel says the opposite or nothing."""
    rgba = np.zeros((N, N, 4), F)
    if form == "rgba32f-alpha-nearest":
        rgba[..., :3] = 1.0 - CHECKER[..., None]; rgba[..., 3] = CHECKER
        return (rgba, "rgba32f", "repeat", "nearest"), 3
    if form == "rgba8-alpha":
        b = np.zeros((N, N, 4), np.uint8)
        b[..., :3] = 255 - (CHECKER[..., None] * 255).astype(np.uint8); b[..., 3] = (CHECKER * 255).astype(np.uint8)
        return (b, "rgba8_unorm", "clamp", "nearest"), 3
    if form == "rgba8-srgb-alpha":  # a kept cell's alpha byte 160: 160 / 255 = 0.627 is kept, its sRGB decode 0.352 would be cut
        b = np.full((N, N, 4), 160, np.uint8)
        b[..., 3] = np.where(CUT_CELLS, 0, 160)
        return (b, "rgba8_srgb", "repeat", "nearest"), 3
    if form == "rgba32f-red":
        rgba[..., 0] = CHECKER; rgba[..., 1:] = 1.0 - CHECKER[..., None]
        return (rgba, "rgba32f", "clamp", "nearest"), 0
    assert form == "bilinear-blocks"  # 2 x 2 equal texels a cell, looked up at the block's centre: four equal texels give the texel exactly
    rgba[..., 3] = CHECKER
    return (np.repeat(np.repeat(rgba, 2, 0), 2, 1), "rgba32f", "repeat", "bilinear"), 3


FORMS = ["rgba32f-alpha-nearest", "rgba8-alpha", "rgba8-srgb-alpha", "rgba32f-red", "bilinear-blocks"]


@pytest.mark.parametrize("count", [True, False], ids=["rays-counted", "rays-not-counted"])
@pytest.mark.parametrize("form", FORMS)
def test_a_checkerboard_cutout_renders_the_collapsed_scene(dev, form, count):
    scene, params, wall, ref, rays, _, _ = _checker_wall()
    tex, channel = _checker_texture(form)
    _setup(dev, scene, params, count)
    dev.upload_textures([tex], _none(scene))  # a set that binds no albedo at all
    dev.bind_cutouts(texture=_at(scene, wall["material"], 0), channel=channel, cutoff=0.5)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and dev.last_kernel() == "pt_render_persistent (extensions, textures, cutouts)"
    _same(got, ref, form)
    if count:
        assert st.rays == rays


# ---- 3. / 4. all accepted, all rejected
@functools.lru_cache(maxsize=None)
def _free_wall(seed=11):
    """The wall with free random coordinates in [-1, 2] at every corner, and a 5 x 4 RGBA32F texture with alpha uniform in [0.5, 1]"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.0, 2.0, (2 * N * N, 3, 2)).astype(F)
    scene, params, wall = scenes.config_cutout_wall(n=N, uv=uv)
    rgba = rng.uniform(0.0, 1.0, (4, 5, 4)).astype(F)
    rgba[..., 3] = rng.uniform(0.5, 1.0, (4, 5)).astype(F)
    return scene, params, wall, (rgba, "rgba32f", "repeat", "bilinear")


@pytest.mark.parametrize("cutoff, what", [(0.5, "all accepted"), (2.0, "all rejected")])
def test_uniform_decisions_render_the_plain_and_the_wall_less_scene(dev, cutoff, what):
    scene, params, wall, tex = _free_wall()
    plain, plain_rays = _oracle(scene, params)
    gone, gone_rays = _oracle(wall["collapsed"](list(wall["tri"])), params)
    assert (_bits(plain) != _bits(gone)).any(-1).mean() >= 1.0 / 3.0  # precondition: the wall is seen
    ref, rays = (plain, plain_rays) if cutoff == 0.5 else (gone, gone_rays)
    _setup(dev, scene, params)
    dev.upload_textures([tex], _none(scene))
    dev.bind_cutouts(texture=_at(scene, wall["material"], 0), channel=3, cutoff=cutoff)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and "cutouts" in dev.last_kernel()
    _same(got, ref, what)
    assert st.rays == rays


# ---- 5. beside maps and the environment: the four CUT forms
@functools.lru_cache(maxsize=None)
def _mapped_checker_wall():
    scene, params, wall = scenes.config_mapped_wall(n=N)  # a conductor wall, alpha 0.2, the cell's centre as coordinates
    first = wall["tri"][0]
    cut_tris = [first + 2 * (j * N + i) + k for j in range(N) for i in range(N) if CUT_CELLS[j, i] for k in (0, 1)]
    collapsed = scenes.collapse_triangles(scene, cut_tris)
    assert np.array_equal(scene["bvh"], collapsed["bvh"])
    ref, rays = _oracle(collapsed, params)
    full, _ = _oracle(scene, params)
    assert (_bits(ref) != _bits(full)).any(-1).mean() >= 1.0 / 3.0
    return scene, params, wall, ref, rays


@pytest.mark.parametrize("env", [False, True], ids=["no-environment", "zero-environment"])
@pytest.mark.parametrize("maps", [False, True], ids=["no-maps", "flat-maps"])
def test_cutouts_beside_flat_maps_and_a_zero_environment(dev, maps, env):
    scene, params, wall, ref, rays = _mapped_checker_wall()
    t, mat = _types(scene), scene["mat"].reshape(-1, 18)
    w = wall["material"]
    assert t[w] == 3 and mat[w, 12] == mat[w, 13]
    rgba = np.zeros((N, N, 4), F)
    rgba[..., 3] = CHECKER
    rough = (np.tile(F([mat[w, 12], mat[w, 13], 0.0]), (3, 3, 1)), "rgba32f", "clamp", "bilinear")  # exactly the wall's own alphas
    _setup(dev, scene, params)
    dev.upload_textures([(rgba, "rgba32f", "repeat", "nearest"), FLAT, rough], _none(scene))
    try:
        if maps:  # the existing pins: a flat normal map and a roughness map of the material's own alphas change no bit
            dev.bind_material_maps(normal=np.where((t == 2) | (t == 3), 1, -1), roughness=_at(scene, w, 2))
        if env:  # ... and neither does an environment of scale 0 in escape mode
            dev.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape", scale=0.0))
        dev.bind_cutouts(texture=_at(scene, w, 0))  # channel 3, cutoff 0.5: the defaults
        got, st = _frames(dev, params)
        name = "pt_render_persistent (extensions, " + ("environment, " if env else "") + "textures, " + ("maps, " if maps else "") + "cutouts)"
        assert st.variant_last == 1 and dev.last_kernel() == name
        _same(got, ref, name)
        assert st.rays == rays
    finally:
        dev.upload_environment(None)


# ---- 6. the feature pass: alpha inside triangles
FEATURE_SEED = 11  # (_free_wall's) measured on the CPU statement: the primary triangle changes on 38.8 % of the wall's 1579 pixels


def test_feature_planes_follow_the_holes(dev, monkeypatch):
    scene, params, wall, _ = _free_wall(FEATURE_SEED)
    rng = np.random.default_rng(FEATURE_SEED + 1)
    rgba = rng.uniform(0.0, 1.0, (4, 5, 4)).astype(F)
    tex = [(rgba, "rgba32f", "repeat", "bilinear")]
    bind = _none(scene)
    cut = host.cutouts(_types(scene).size, texture=_at(scene, wall["material"], 0), channel=3, cutoff=0.5)
    ref_n, ref_a, ref_g = host.render_features_geom_cutout(scene, params, tex, bind, cut)
    un_n, un_a, un_g = host.render_features_geom(scene, params)
    # precondition, on the CPU statements: between 20 % and 80 % of the wall's pixels change their primary triangle
    t0, t1 = un_g[..., 0].view(np.int32), ref_g[..., 0].view(np.int32)
    on_wall = np.isin(t0, np.asarray(list(wall["tri"])))
    share = (t0 != t1)[on_wall].mean()
    print(f"wall pixels {int(on_wall.sum())}, primary triangle changed on {share:.1%}")
    assert on_wall.sum() > 500 and 0.2 <= share <= 0.8, share
    _setup(dev, scene, params)
    dev.upload_textures(tex, bind)
    dev.bind_cutouts(cut)
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        dev.track_motion(True)
        dev.render_features(params)
        n, a = dev.read_features()
        _same(dev.read_features_geom(), ref_g, f"compact={compact}: plane G"); _same(a, ref_a, f"compact={compact}: plane A"); _same(n, ref_n, f"compact={compact}: plane N")
        dev.track_motion(False)  # without G: the kernels on CutArgs<TexArgs>
        dev.render_features(params)
        n, a = dev.read_features()
        _same(a, ref_a, f"compact={compact}: plane A without G"); _same(n, ref_n, f"compact={compact}: plane N without G")
    monkeypatch.delenv("GLRTX_COMPACT_NODES")
    dev.bind_cutouts()  # unbound: the kernels the pass ran before
    dev.render_features(params)
    n, a = dev.read_features()
    _same(n, un_n, "unbound: plane N"); _same(a, un_a, "unbound: plane A")


# ---- 7. after a move
def test_the_records_survive_a_vertex_update(dev):
    scene, params, wall, _, _, _, _ = _checker_wall()
    moved = scene["vert"].reshape(-1, 5, 3).copy()
    r = slice(wall["vert"].start, wall["vert"].stop)
    moved[r, 0, 1] += F(0.3)  # the wall lifted by 0.3
    moved[r, 2, :2] = 0.0  # the update's own uv words are not read: the {s, t} table is the upload's
    moved_scene = dict(scene, vert=moved.reshape(-1, 3))
    moved_scene["bvh"] = host.refit_bvh(moved_scene["vert"], moved_scene["tri"], scene["bvh"])
    ref_scene = wall["collapsed"](wall["cell_tris"](CUT_CELLS), moved_scene)
    assert np.array_equal(ref_scene["bvh"], moved_scene["bvh"])
    ref, rays = _oracle(ref_scene, params)
    uncut, _ = _oracle(moved_scene, params)
    assert (_bits(ref) != _bits(uncut)).any(-1).mean() >= 1.0 / 3.0
    tex, channel = _checker_texture("rgba32f-alpha-nearest")
    _setup(dev, scene, params)
    dev.upload_textures([tex], _none(scene))
    dev.bind_cutouts(texture=_at(scene, wall["material"], 0), channel=channel, cutoff=0.5)
    dev.update_vertices(moved.reshape(-1, 15))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and "cutouts" in dev.last_kernel()
    _same(got, ref, "the moved, collapsed scene with the refitted tree")
    assert st.rays == rays


# ---- 8. routing and refusals
def test_routing_and_refusals(dev):
    scene, params, wall, ref, rays, full, full_rays = _checker_wall()
    tex, channel = _checker_texture("rgba32f-alpha-nearest")
    n_mat = _types(scene).size
    w, t = wall["material"], _types(scene)
    grey, lamp, cu = int(np.flatnonzero(t == 2)[0]), int(np.flatnonzero(t == 1)[0]), int(np.flatnonzero(t == 3)[0])
    d = device.Device()
    try:
        with pytest.raises(device.GlrtxError, match="no texture set is bound"):
            d.bind_cutouts(texture=_at(scene, w, 0))
        d.upload_scene(scene)
        with pytest.raises(device.GlrtxError, match="no texture set is bound"):
            d.bind_cutouts(texture=_at(scene, w, 0))
        d.upload_scene(scenes.rebuild_bvh(scene, "chain"))  # a vine tree: the list scan has no cutout form
        d.upload_textures([tex], _none(scene))
        with pytest.raises(device.GlrtxError, match="the tree is a vine"):
            d.bind_cutouts(texture=_at(scene, w, 0))
    finally:
        d.close()
    _setup(dev, scene, params)
    dev.upload_textures([tex], _none(scene))
    dev.set_texture_wavefront(True)
    before, st0 = _frames(dev, params)  # the T form, before the bind
    assert st0.variant_last == 2 and st0.rays == full_rays
    _same(before, full, "the T form renders the plain scene")
    dev.bind_cutouts(texture=_at(scene, w, 0), channel=channel, cutoff=0.5)
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and st.fallback_last & device.FALLBACK_EXTENSIONS  # the switch does not take cutouts
    _same(got, ref, "bound, with the texture wavefront switch on")
    assert st.rays == rays

    def still_cut(what):
        got, st = _frames(dev, params)
        _same(got, ref, f"after the refusal '{what}'")
        assert st.variant_last == 1 and st.rays == rays

    with pytest.raises(device.GlrtxError, match="textures are bound.*cutouts are bound"):
        dev.render_adaptive(params, SEEDS, 0.05)
    still_cut("render_adaptive")
    with pytest.raises(device.GlrtxError, match="textures are bound.*cutouts are bound"):
        dev.hit_histogram(params, scene["tri"].reshape(-1, 4).shape[0])
    still_cut("hit_histogram")

    def refused(words, *a, **kw):
        with pytest.raises(device.GlrtxError, match=words) as e:
            dev.bind_cutouts(*a, **kw)
        assert e.value.code == device.GLRTX_EINVAL
        still_cut(words)

    good = _at(scene, w, 0)
    refused(f"{n_mat - 1} records, the scene has {n_mat} materials", texture=good[:-1])
    refused(f"material {w}: cutout texture 1 of 1 textures", texture=_at(scene, w, 1))
    refused(f"material {w}: cutout texture -2 of 1 textures", texture=_at(scene, w, -2))
    refused(f"material {w}: channel 4 is not 0 .. 3", texture=good, channel=np.where(np.arange(n_mat) == w, 4, 3))
    refused(f"material {grey}: channel -1 is not 0 .. 3", texture=good, channel=np.where(np.arange(n_mat) == grey, -1, 3))
    for bad in (np.inf, -np.inf, np.nan):
        refused(f"material {w}: cutoff is not finite", texture=good, cutoff=np.where(np.arange(n_mat) == w, bad, 0.5))
    refused(f"material {lamp} has a cutout and is neither diffuse nor conductor", texture=_at(scene, lamp, 0))
    rec = host.cutouts(n_mat, texture=good)
    rec["reserved"][cu] = 7
    refused(f"material {cu}: reserved is 7", rec)
    both = good.copy()
    both[cu] = 0
    dev.bind_cutouts(texture=both)  # a conductor may be cut as well (here: the sphere, by the same texture)
    # beside the volume: refused at render time, and nothing has changed afterwards
    dens, temp = scenes.fire_grids()
    dev.upload_volume(dens, temp, (-1.0, 0.0, -1.0), (1.0, 2.0, 1.0))
    dev.set_extensions(device.EXT_VOLUME)
    with pytest.raises(device.GlrtxError, match="GLRTX_EXT_VOLUME is set and cutouts are bound"):
        dev.render(dict(params, seed=SEEDS[0]))
    dev.set_extensions(0)
    dev.upload_volume(None, None, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    dev.bind_cutouts(texture=good, channel=channel, cutoff=0.5)
    still_cut("binding again")
    # after unbinding the T form runs again and equals its image from before the bind
    dev.bind_cutouts()
    got, st = _frames(dev, params)
    assert st.variant_last == 2 and st.fallback_last == 0 and st.rays == full_rays
    _same(got, before, "unbound: the T form's image from before the bind")
    # upload_textures drops the records, and so does upload_scene
    dev.bind_cutouts(texture=good)
    dev.upload_textures([tex], _none(scene))
    got, st = _frames(dev, params)
    assert st.variant_last == 2
    _same(got, before, "after upload_textures")
    dev.bind_cutouts(texture=good)
    dev.upload_scene(scene)
    got, st = _frames(dev, params)
    assert st.variant_last == 2 and st.rays == full_rays
    with pytest.raises(device.GlrtxError, match="no texture set is bound"):
        dev.bind_cutouts(texture=good)
    dev.set_texture_wavefront(False)
