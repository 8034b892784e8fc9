"""Textures and material maps on the wavefront kernel (glrtx_set_texture_wavefront: pt_render_wgwf's T and TM forms, csrc/pt_kernel.hip.h:
wf_shade_textured).  Pinned through the reference -- a texture constant over each cell renders, on the T form, the image the per-cell scene renders on the plain
wavefront kernel, which tests/test_gpu_texture.py ties to the oracle -- and held bit for bit, images and ray counts, to the textured megakernel through every
way a launch is made: frames in flight, fed single calls, adaptive calls, the moments and cascade folds, the present ring, a group; and the routing back to the
megakernel where the forms do not apply."""
import functools
import subprocess

import numpy as np
import pytest

import adaptive_math as am
import adaptive_moments_math as amm
import texture_cases as tc
import texture_math as tm
from conftest import PKG, assert_bit_equal
from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

F = np.float32
N = 6
BIG = dict(width=203, height=131)  # partial 8 x 8 tiles at both edges, several workgroups; 64 x 48 (the wall scenes' own size): one workgroup holds every path
TRAVERSALS = {  # environment -> (node_fetch_last, node_layout_last)
    "compact": ({"GLRTX_COMPACT_NODES": "1"}, 0, 1),
    "fetch0": ({"GLRTX_COMPACT_NODES": "0", "GLRTX_PAIR_FETCH": "0"}, 0, 0),
    "pair": ({"GLRTX_COMPACT_NODES": "0", "GLRTX_PAIR_FETCH": "1"}, 1, 0),
}


@pytest.fixture(autouse=True)
def _no_env_switch(monkeypatch):
    monkeypatch.delenv("GLRTX_TEXTURE_WAVEFRONT", raising=False)


@pytest.fixture(scope="module")
def devices(gpu_device):
    """Two contexts of this module's own (gpu_device first: torch's runtime is set up before libglrtx's)."""
    ds = (device.Device(), device.Device())
    yield ds
    for d in ds:
        d.close()


def _seeds(n, f0=0):
    return [host.frame_seed(f0 + i) for i in range(n)]


def _setup(d, scene, params, tex=None, bind=None, maps=None, wavefront=False, count=True):
    d.set_variant(2); d.count_rays(count); d.set_extensions(0); d.upload_environment(None)
    d.upload_scene(scene); d.upload_spheres(None)
    if tex is not None:
        d.upload_textures(tex, bind)
        if maps:
            d.bind_material_maps(**maps)
    d.set_texture_wavefront(wavefront)
    d.set_partition(0, 1, 16); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _teardown(*ds):
    for d in ds:
        d.set_texture_wavefront(False)
        d.upload_textures(None, None)
        d.set_extensions(0); d.upload_spheres(None); d.upload_environment(None)
        d.count_rays(False); d.track_moments(False); d.track_cascades(False)


def _frames(d, params, seeds):
    d.render_frames(params, seeds)
    d.sync()
    return d.read_accum(), d.stats()


def _singles(d, params, seeds):
    for sd in seeds:
        d.render(dict(params, seed=sd))
    d.sync()
    return d.read_accum(), d.stats()


def _on_t_form(st):
    assert st.variant_last == 2 and st.fallback_last == 0 and st.fallback_launches == 0 and st.device_error_pending == 0, \
        (st.variant_last, st.fallback_last, st.fallback_launches, st.device_error_pending)


def _same_rays(st, ref):
    assert st.rays == ref.rays > 0 and st.rays_untraced == ref.rays_untraced and st.paths == ref.paths, (st.rays, ref.rays, st.rays_untraced, ref.rays_untraced)


def _none(scene):
    return np.full(scene["mat"].reshape(-1, 18).shape[0], -1, np.int32)


def _at(scene, material, k=0):
    b = _none(scene)
    b[material] = k
    return b


def _cell_texture(albedo, fmt="rgba32f", filt="nearest", block=1):
    """albedo (n, n, 3): texel [j, i] of cell (column i, row j), each repeated block x block times."""
    return (np.repeat(np.repeat(albedo, block, 0), block, 1), fmt, "repeat", filt)


def _corner_uv(n, scale=1.0, shift=0.0):
    """The wall's own parametrisation (s across, t up, [0, 1]) at the corners of quad()'s triangles (a, b, c), (a, c, d), scaled and shifted."""
    st = []
    for j in range(n):
        for i in range(n):
            c = np.array([[i, j], [i + 1, j], [i + 1, j + 1], [i, j + 1]], F) / F(n)
            st.append(np.stack([c[[0, 1, 2]], c[[0, 2, 3]]]))
    return (np.concatenate(st, 0) * F(scale) + F(shift)).astype(F)


@functools.lru_cache(maxsize=None)
def _wall(kind="float", n_samples=2):
    """The textured wall and its per-cell form (the same triangles, the same tree), and for `srgb` the texture's bytes."""
    albedo = code = None
    if kind == "srgb":
        code = np.random.default_rng(21).integers(40, 250, (N, N, 3), dtype=np.uint8)
        albedo = tm.SRGB[code.astype(np.int64)]
    tex_scene, params, wall = scenes.config_textured_wall(n=N, albedo=albedo, n_samples=n_samples)
    cell_scene, cell_params, cells = scenes.config_textured_wall(n=N, albedo=albedo, per_cell=True, n_samples=n_samples)
    assert np.array_equal(tex_scene["bvh"], cell_scene["bvh"])  # precondition: the same tree
    return tex_scene, params, wall, cell_scene, code


def _constant_per_cell(form):
    scene, params, wall, cell_scene, code = _wall("srgb" if form == "srgb" else "float")
    if form == "nearest":
        tex = _cell_texture(wall["albedo"])
    elif form == "bilinear-blocks":
        tex = _cell_texture(wall["albedo"], filt="bilinear", block=2)
    else:
        tex = _cell_texture(code, fmt="rgba8_srgb")
    return scene, params, wall, cell_scene, tex


_CELL_REF = {}


def _cell_reference(d2, kind):
    """The per-cell scene on the plain wavefront kernel, 3 frames in flight, counting: computed once a texel kind (every traversal form renders the same bits)."""
    if kind not in _CELL_REF:
        _, params, _, cell_scene, _ = _wall(kind)
        _setup(d2, cell_scene, params)
        acc, st = _frames(d2, params, _seeds(3))
        assert st.variant_last == 2 and st.fallback_last == 0
        _CELL_REF[kind] = (acc, st.rays, st.rays_untraced)
    return _CELL_REF[kind]


# ---- 1. pinned through the reference: a texture constant over each cell is one material a cell on the plain kernel
@pytest.mark.parametrize("count_rays", [True, False], ids=["counting", "timed"])
@pytest.mark.parametrize("traversal", list(TRAVERSALS))
@pytest.mark.parametrize("form", ["nearest", "bilinear-blocks", "srgb"])
def test_constant_per_cell_texture_equals_the_per_cell_scene_on_the_plain_kernel(devices, monkeypatch, form, traversal, count_rays):
    d, d2 = devices
    env, fetch, layout = TRAVERSALS[traversal]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    scene, params, wall, _, tex = _constant_per_cell(form)
    try:
        ref, rays, untraced = _cell_reference(d2, "srgb" if form == "srgb" else "float")
        _setup(d, scene, params, [tex], _at(scene, wall["material"]), wavefront=True, count=count_rays)
        acc, st = _frames(d, params, _seeds(3))
        _on_t_form(st)
        assert (st.node_fetch_last, st.node_layout_last) == (fetch, layout), (st.node_fetch_last, st.node_layout_last)
        assert_bit_equal(acc, ref, f"{form}, {traversal}: T form vs the per-cell scene on the plain kernel")
        if count_rays:
            assert st.rays == rays > 0 and st.rays_untraced == untraced
    finally:
        _teardown(d, d2)


def test_forced_alternating_fetch_is_served_as_one_record_per_lane(devices, monkeypatch):
    d, d2 = devices
    monkeypatch.setenv("GLRTX_COMPACT_NODES", "0")
    monkeypatch.setenv("GLRTX_PAIR_FETCH", "2")
    scene, params, wall, _, tex = _constant_per_cell("nearest")
    try:
        ref, rays, untraced = _cell_reference(d2, "float")
        _setup(d, scene, params, [tex], _at(scene, wall["material"]), wavefront=True)
        acc, st = _frames(d, params, _seeds(3))
        _on_t_form(st)
        assert st.node_fetch_last == 0 and st.node_layout_last == 0
        assert_bit_equal(acc, ref, "GLRTX_PAIR_FETCH=2")
        assert st.rays == rays
    finally:
        _teardown(d, d2)


# ---- 2. general textures against the megakernel: frames in flight and fed single calls
@pytest.mark.parametrize("fmt", tc.FORMATS)
@pytest.mark.parametrize("size", [(5, 3), (16, 16)], ids=["5x3", "16x16"])
def test_general_textures_equal_the_megakernel(devices, size, fmt):
    d, d2 = devices
    uv = _corner_uv(N, 2.5, -0.75)  # beyond [0, 1] on every side: repeat and clamp both act
    scene, params, wall = scenes.config_textured_wall(n=N, uv=uv, max_depth=8, **BIG)
    texels = tc.texels(size[0], size[1], fmt, 31 + size[0])
    bind = _at(scene, wall["material"])
    seeds = _seeds(24)
    try:
        for filt in tc.FILTERS:
            for wrap in ("repeat", "clamp"):
                what = f"{size} {fmt} {filt} {wrap}"
                tex = [(texels, fmt, wrap, filt)]
                _setup(d2, scene, params, tex, bind)
                ref12, st12 = _singles(d2, params, seeds[:12])
                assert st12.variant_last == 1 and st12.fallback_last == device.FALLBACK_EXTENSIONS
                _setup(d, scene, params, tex, bind, wavefront=True)
                acc, st = _frames(d, params, seeds[:12])
                _on_t_form(st)
                assert_bit_equal(acc, ref12, f"{what}: 12-frame render_frames vs 12 megakernel launches")
                _same_rays(st, st12)
                ref24, st24 = _singles(d2, params, seeds[12:])  # (on top of the 12: 24 megakernel launches)
                _setup(d, scene, params, tex, bind, wavefront=True)
                acc, st = _singles(d, params, seeds)
                _on_t_form(st)
                assert st.feed_appended > 0
                assert_bit_equal(acc, ref24, f"{what}: 24 single calls vs 24 megakernel launches")
                _same_rays(st, st24)
    finally:
        _teardown(d, d2)


# ---- 3. material maps: the TM form
def _normal_map(seed=5):
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.uniform(-0.6, 0.6, (8, 8, 2)), np.ones((8, 8, 1))], -1)
    m /= np.linalg.norm(m, axis=-1, keepdims=True)
    return (((m + 1.0) / 2.0).astype(F), "rgba32f", "repeat", "bilinear")


def _roughness_map(seed=6):
    rng = np.random.default_rng(seed)
    a = np.concatenate([rng.uniform(0.02, 0.6, (8, 8, 2)), np.zeros((8, 8, 1))], -1).astype(F)
    return (a, "rgba32f", "repeat", "bilinear")


@pytest.mark.parametrize("case", ["normal-on-diffuse", "normal-on-conductor", "roughness-on-conductor", "both-on-conductor"])
def test_maps_equal_the_megakernels_maps_kernels(devices, case):
    d, d2 = devices
    big = case == "both-on-conductor"
    shape = dict(max_depth=8, **BIG) if big else {}
    scene, params, wall = scenes.config_mapped_wall(n=N, wall="diffuse" if case == "normal-on-diffuse" else "conductor", uv="corner", **shape)
    w = wall["material"]
    maps = dict(normal_scale=0.7)
    if case != "roughness-on-conductor":
        maps["normal"] = _at(scene, w, 0)
    if case in ("roughness-on-conductor", "both-on-conductor"):
        maps["roughness"] = _at(scene, w, 1)
    tex = [_normal_map(), _roughness_map()]
    seeds = _seeds(8 if big else 3)
    try:
        _setup(d2, scene, params, tex, _none(scene), maps)
        ref, st2 = _singles(d2, params, seeds)
        assert st2.variant_last == 1
        _setup(d2, scene, params, tex, _none(scene))
        unmapped, _ = _singles(d2, params, seeds)
        assert (unmapped.view(np.uint32) != ref.view(np.uint32)).any(-1).mean() > 0.05  # the maps are seen
        _setup(d, scene, params, tex, _none(scene), maps, wavefront=True)
        acc, st = _frames(d, params, seeds)
        _on_t_form(st)
        assert_bit_equal(acc, ref, f"{case}: TM form vs the megakernel's MAPS kernel")
        _same_rays(st, st2)
    finally:
        _teardown(d, d2)


def test_flat_maps_equal_the_unmapped_scene_on_the_plain_kernel(devices):
    d, d2 = devices
    scene, params, wall = scenes.config_mapped_wall(n=N, uv="corner")
    t = scene["mat"].reshape(-1, 18)[:, 0].astype(np.int32)
    mat = scene["mat"].reshape(-1, 18)
    flat = (np.tile(F([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear")
    w = wall["material"]
    assert t[w] == 3
    own = (np.tile(F([mat[w, 12], mat[w, 13], 0.0]), (3, 3, 1)), "rgba32f", "clamp", "bilinear")  # exactly the conductor's alphas
    try:
        _setup(d2, scene, params)
        ref, st2 = _frames(d2, params, _seeds(3))
        assert st2.variant_last == 2
        _setup(d, scene, params, [flat, own], _none(scene), dict(normal=np.where((t == 2) | (t == 3), 0, -1).astype(np.int32), roughness=_at(scene, w, 1)), wavefront=True)
        acc, st = _frames(d, params, _seeds(3))
        _on_t_form(st)
        assert_bit_equal(acc, ref, "flat maps vs the unmapped scene")
        _same_rays(st, st2)
    finally:
        _teardown(d, d2)


def test_per_cell_roughness_map_equals_the_per_cell_scene_on_the_plain_kernel(devices):
    d, d2 = devices
    scene, params, wall = scenes.config_mapped_wall(n=N)
    cell_scene, _, cells = scenes.config_mapped_wall(n=N, per_cell=True)
    assert np.array_equal(scene["bvh"], cell_scene["bvh"])
    a = np.concatenate([wall["alpha"], np.zeros(wall["alpha"].shape[:2] + (1,), F)], -1).astype(F)
    tex = (np.repeat(np.repeat(a, 2, 0), 2, 1), "rgba32f", "repeat", "bilinear")
    try:
        _setup(d2, cell_scene, params)
        ref, st2 = _frames(d2, params, _seeds(3))
        assert st2.variant_last == 2
        _setup(d, scene, params, [tex], _none(scene), dict(roughness=_at(scene, wall["material"])), wavefront=True)
        acc, st = _frames(d, params, _seeds(3))
        _on_t_form(st)
        assert_bit_equal(acc, ref, "per-cell roughness map vs one conductor a cell")
        _same_rays(st, st2)
    finally:
        _teardown(d, d2)


# ---- 4. materials past the LDS staging limit
def test_beyond_the_lds_material_limit(devices):
    d, d2 = devices
    scene, params, wall, _, tex = _constant_per_cell("nearest")
    pad = np.array([r for _ in range(300) for r in scenes._mat_rows(scenes.diffuse((0.3, 0.3, 0.3)))], np.float32)
    big = dict(scene, mat=np.concatenate([scene["mat"].reshape(-1, 3), pad], 0))
    assert big["mat"].shape[0] // 6 > 256
    try:
        ref, rays, untraced = _cell_reference(d2, "float")
        _setup(d, big, params, [tex], _at(big, wall["material"]), wavefront=True)
        acc, st = _frames(d, params, _seeds(3))
        _on_t_form(st)
        assert_bit_equal(acc, ref, "300 more materials")
        assert st.rays == rays and st.rays_untraced == untraced
    finally:
        _teardown(d, d2)


# ---- 5. after a move: the mapping stays, the map frame follows the refitted edges
@pytest.mark.parametrize("form", ["T", "TM"])
def test_after_update_vertices(devices, form):
    d, d2 = devices
    if form == "T":
        scene, params, wall = scenes.config_textured_wall(n=N, uv=_corner_uv(N))
        tex, bind, maps = [(tc.texels(16, 16, "rgba32f", 3), "rgba32f", "repeat", "bilinear")], _at(scene, wall["material"]), None
    else:
        scene, params, wall = scenes.config_mapped_wall(n=N, wall="diffuse", uv="corner")
        tex, bind, maps = [_normal_map()], _none(scene), dict(normal=_at(scene, wall["material"]), normal_scale=0.7)
    moved = scene["vert"].reshape(-1, 5, 3).copy()
    r = slice(wall["vert"].start, wall["vert"].stop)
    moved[r, 0, 0] += F(0.5)                          # shifted
    moved[r, 0, 2] += F(0.3) * moved[r, 0, 1]         # and sheared: z grows with y
    moved[r, 2, :2] = 0.0                             # the update's own uv words are not read
    seeds = _seeds(3)
    try:
        _setup(d2, scene, params, tex, bind, maps)
        before, _ = _singles(d2, params, seeds)
        d2.update_vertices(moved.reshape(-1, 15))
        d2.clear(); d2.reset_stats()
        ref, st2 = _singles(d2, params, seeds)
        assert st2.variant_last == 1
        assert (before.view(np.uint32) != ref.view(np.uint32)).any(-1).mean() > 0.05  # the move is seen
        _setup(d, scene, params, tex, bind, maps, wavefront=True)
        d.update_vertices(moved.reshape(-1, 15))
        acc, st = _frames(d, params, seeds)
        _on_t_form(st)
        assert_bit_equal(acc, ref, f"{form} form after update_vertices")
        _same_rays(st, st2)
    finally:
        _teardown(d, d2)


# ---- 6. adaptive calls
def test_adaptive_nothing_retires_equals_render_frames(devices):
    d, d2 = devices
    scene, params, wall = scenes.config_textured_wall(n=N, uv=_corner_uv(N, 2.5, -0.75), max_depth=8, **BIG)
    tex, bind = [(tc.texels(16, 16, "rgba8_srgb", 4), "rgba8_srgb", "repeat", "bilinear")], _at(scene, wall["material"])
    try:
        _setup(d, scene, params, tex, bind, wavefront=True)
        _setup(d2, scene, params, tex, bind)
        f0 = 0
        for n in (1, 4, 2):
            d.render_adaptive(params, _seeds(n, f0), -1.0, 2)
            d2.render_frames(params, _seeds(n, f0))
            f0 += n
        active, total = d.adaptive_active_tiles()
        assert active == total == ((BIG["height"] + 7) // 8) * ((BIG["width"] + 7) // 8)
        d2.sync()
        _on_t_form(d.stats())
        assert d2.stats().variant_last == 1
        assert_bit_equal(d.read_accum(), d2.read_accum(), "adaptive (threshold -1) vs the megakernel's frames")
        _same_rays(d.stats(), d2.stats())
    finally:
        _teardown(d, d2)


def _adaptive_pair(devices):
    """The textured wall on the T form and its per-cell form on the plain kernel, one sample a frame (the half buffer takes every second FRAME's sample then)."""
    d, d2 = devices
    scene, params, wall, cell_scene, _ = _wall("float", n_samples=1)
    _setup(d, scene, params, [_cell_texture(wall["albedo"], filt="bilinear", block=2)], _at(scene, wall["material"]), wavefront=True)
    _setup(d2, cell_scene, params)
    return d, d2, params


def test_adaptive_median_threshold_equals_the_per_cell_scene_call_by_call(devices):
    """The scene and the threshold rule (the median tile error after 6 frames) were checked on the CPU oracle for the per-cell scene: 24 of 48 tiles stay active."""
    try:
        d, d2, params = _adaptive_pair(devices)
        thr, f0 = -1.0, 0
        for k, n in enumerate([2, 4, 3, 3]):
            if k == 2:
                thr = float(np.median(am.tile_error(d2.read_accum(), d2.read_adaptive_half())))
                want, _, _ = am.select(d2.read_accum(), d2.read_adaptive_half(), thr, 2)
            for x in (d, d2):
                x.render_adaptive(params, _seeds(n, f0), thr, 2)
            f0 += n
            (active, total), (active2, total2) = d.adaptive_active_tiles(), d2.adaptive_active_tiles()
            assert (active, total) == (active2, total2), (k, active, total, active2, total2)
            if k >= 2:
                assert 0 < active < total, (k, active, total)
            if k == 2:
                assert np.array_equal(d2.tile_mask(), want)  # the plain kernel's selection is the numpy statement's
            assert np.array_equal(d.tile_mask(), d2.tile_mask()), k
            assert_bit_equal(d.read_accum(), d2.read_accum(), f"accumulator after call {k}")
            assert_bit_equal(d.read_adaptive_half(), d2.read_adaptive_half(), f"half buffer after call {k}")
        _on_t_form(d.stats())
        assert d2.stats().variant_last == 2
        _same_rays(d.stats(), d2.stats())
    finally:
        _teardown(*devices)


def test_adaptive_moments_equals_the_per_cell_scene(devices):
    try:
        d, d2, params = _adaptive_pair(devices)
        for x in (d, d2):
            x.track_moments(True)
            x.render_adaptive_moments(params, _seeds(6), -1.0, 2)
        thr = float(np.median(amm.tile_error(d2.read_moments())))
        for x in (d, d2):
            x.render_adaptive_moments(params, _seeds(3, 6), thr, 2)
        active, total = d.adaptive_active_tiles()
        assert (active, total) == d2.adaptive_active_tiles() and 0 < active < total, (active, total)
        assert np.array_equal(d.tile_mask(), d2.tile_mask())
        assert_bit_equal(d.read_accum(), d2.read_accum(), "accumulator")
        assert_bit_equal(d.read_moments(), d2.read_moments(), "moments plane")
        _on_t_form(d.stats())
    finally:
        _teardown(*devices)


# ---- 7. the moments and cascade folds
def test_moments_and_cascades_equal_the_per_cell_scene(devices):
    d, d2 = devices
    scene, params, wall, cell_scene, _ = _wall("float")
    try:
        _setup(d, scene, params, [_cell_texture(wall["albedo"])], _at(scene, wall["material"]), wavefront=True)
        _setup(d2, cell_scene, params)
        for x in (d, d2):
            x.track_moments(True)
            x.render_moments(params, _seeds(4))
        assert_bit_equal(d.read_accum(), d2.read_accum(), "render_moments: accumulator")
        assert_bit_equal(d.read_moments(), d2.read_moments(), "render_moments: moments plane")
        assert d.read_moments()[..., 3].min() == 8  # 4 frames of 2 samples
        _on_t_form(d.stats())
        for x in (d, d2):
            x.track_moments(False)
            x.clear()
            x.track_cascades(True)
            x.render_cascades(params, _seeds(4, 4))
        assert_bit_equal(d.read_accum(), d2.read_accum(), "render_cascades: accumulator")
        c, c2 = d.read_cascades(), d2.read_cascades()
        assert c.shape[0] == 6 and c[..., 3].sum() > 0
        assert_bit_equal(c, c2, "render_cascades: the six cascade planes")
        _on_t_form(d.stats())
    finally:
        _teardown(d, d2)


# ---- 8. the present ring
def test_present_ring_images_equal_the_resolve(devices):
    d, _ = devices
    scene, params, wall, _, tex = _constant_per_cell("bilinear-blocks")
    try:
        _setup(d, scene, params, [tex], _at(scene, wall["material"]), wavefront=True, count=False)
        d.present_enable(4)
        try:
            for f in range(3):
                d.render(dict(params, seed=host.frame_seed(f)))
                img = d.present_acquire(True)
                ref = d.resolve_rgba8(2.2, True)
                assert np.array_equal(img.rgba, ref), f
                d.present_release(img)
            d.render_frames(params, _seeds(3, 3))
            imgs = [d.present_acquire(True) for _ in range(3)]
            ref = d.resolve_rgba8(2.2, True)
            assert np.array_equal(imgs[-1].rgba, ref)
            for img in imgs:
                d.present_release(img)
            _on_t_form(d.stats())
        finally:
            d.present_enable(0)
    finally:
        _teardown(d)


# ---- 9. a group of two on one device
def test_group_of_two_on_one_device_equals_one_context(devices):
    import ctypes as C
    d, _ = devices
    scene, params, wall = scenes.config_textured_wall(n=N, uv=_corner_uv(N, 2.5, -0.75), **BIG)
    tex, bind = [(tc.texels(5, 3, "rgba8_unorm", 9), "rgba8_unorm", "clamp", "bilinear")], _at(scene, wall["material"])
    seeds = _seeds(3)
    try:
        _setup(d, scene, params, tex, bind, wavefront=True, count=False)
        one, st = _frames(d, params, seeds)
        _on_t_form(st)
    finally:
        _teardown(d)
    g = device.Group([0, 0])
    try:
        g.upload_scene(scene)
        desc, blob = host.pack_textures(tex)
        g.member_call(g.L.glrtx_upload_textures, desc.ctypes.data, desc.size, blob.ctypes.data, blob.size, bind.ctypes.data_as(C.POINTER(C.c_int32)), bind.size)
        g.member_call(g.L.glrtx_set_texture_wavefront, 1)
        g.resize(params["width"], params["height"])
        g.render_frames(params, seeds)
        g.sync()
        two = g.read_accum()
        assert g.stats().fallback_launches == 0
    finally:
        g.close()
    assert_bit_equal(two, one, "group vs context")


# ---- 10. routing: where the forms do not apply
@pytest.mark.parametrize("other", ["sphere", "dielectric", "environment", "vine", "depth256"])
def test_anything_else_still_runs_on_the_megakernel(devices, other):
    d, d2 = devices
    scene, params, wall = scenes.config_textured_wall(n=8 if other == "vine" else N, bvh="chain" if other == "vine" else "sah")
    if other == "vine":
        assert scene["tri"].reshape(-1, 4).shape[0] > 200
    if other == "depth256":
        params = dict(params, max_depth=256)
    tex, bind = [(tc.texels(5, 3, "rgba32f", 2), "rgba32f", "repeat", "bilinear")], _at(scene, wall["material"])

    def rest(x):
        if other == "sphere":
            x.upload_spheres([[2.5, 1.0, 0.5, 1.0, 0.0]])
        elif other == "dielectric":
            x.set_extensions(device.EXT_DIELECTRIC)
        elif other == "environment":
            x.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape"))

    try:
        _setup(d2, scene, params, tex, bind)
        rest(d2)
        ref, st2 = _singles(d2, params, _seeds(2))
        _setup(d, scene, params, tex, bind, wavefront=True)
        rest(d)
        acc, st = _singles(d, params, _seeds(2))
        assert st.variant_last == 1 and st.fallback_last & device.FALLBACK_EXTENSIONS and st.fallback_launches == 2, (st.variant_last, st.fallback_last)
        assert st.fallback_last == st2.fallback_last
        if other == "depth256":
            assert st.fallback_last & device.FALLBACK_DEPTH
        assert_bit_equal(acc, ref, f"{other}: the switch changes nothing")
        _same_rays(st, st2)
        with pytest.raises(device.GlrtxError, match="textures are bound") as e:
            d.render_adaptive(params, _seeds(1), -1.0, 2)
        assert e.value.code == device.GLRTX_EINVAL
        d.track_moments(True)
        with pytest.raises(device.GlrtxError, match="textures are bound"):
            d.render_moments(params, _seeds(1))
    finally:
        _teardown(d, d2)


def test_switch_off_and_unbinding(devices):
    d, d2 = devices
    scene, params, wall, _, tex = _constant_per_cell("nearest")
    bind = _at(scene, wall["material"])
    seeds = _seeds(2)
    try:
        _setup(d2, scene, params)
        plain, _ = _singles(d2, params, seeds)  # the untextured scene
        _setup(d, scene, params, [tex], bind, wavefront=True)
        on, st = _singles(d, params, seeds)
        _on_t_form(st)
        # switch off again: the megakernel and the old refusals
        d.set_texture_wavefront(False)
        d.clear(); d.reset_stats()
        off, st = _singles(d, params, seeds)
        assert st.variant_last == 1 and st.fallback_last == device.FALLBACK_EXTENSIONS and st.fallback_launches == 2
        assert_bit_equal(off, on, "switch off vs on")
        with pytest.raises(device.GlrtxError, match="textures are bound"):
            d.render_adaptive(params, seeds, 0.05)
        d.track_moments(True)
        with pytest.raises(device.GlrtxError, match="textures are bound"):
            d.render_moments(params, seeds)
        with pytest.raises(device.GlrtxError, match="textures are bound"):
            d.render_adaptive_moments(params, seeds, 0.05)
        d.track_moments(False)
        d.track_cascades(True)
        with pytest.raises(device.GlrtxError, match="textures are bound"):
            d.render_cascades(params, seeds)
        d.track_cascades(False)
        # the environment switch overrides the context's, at every launch
        d.set_texture_wavefront(True)
        import os
        os.environ["GLRTX_TEXTURE_WAVEFRONT"] = "0"
        try:
            d.clear(); d.reset_stats()
            assert _singles(d, params, seeds)[1].variant_last == 1
        finally:
            del os.environ["GLRTX_TEXTURE_WAVEFRONT"]
        # the histogram refuses while a set is bound, switch or no switch
        with pytest.raises(device.GlrtxError, match="textures are bound"):
            d.hit_histogram(params, scene["tri"].reshape(-1, 4).shape[0])
        # unbound with the switch still on: the plain kernel, the untextured image
        d.upload_textures(None, None)
        d.clear(); d.reset_stats()
        got, st = _singles(d, params, seeds)
        assert st.variant_last == 2 and st.fallback_last == 0
        assert_bit_equal(got, plain, "unbound")
        assert (plain.view(np.uint32) != on.view(np.uint32)).any(-1).mean() > 0.2
    finally:
        _teardown(d, d2)


# ---- 11. the façade
def test_glrt_main_texture_wavefront_writes_the_same_png(tmp_path, gpu_device):
    from PIL import Image
    rng = np.random.default_rng(8)
    tex = rng.integers(20, 250, (6, 7, 3), dtype=np.uint8)
    scenes.write_ppm(tmp_path / "wall.ppm", tex)
    _, _, wall = scenes.config_textured_wall(n=4, uv=rng.uniform(-1.0, 2.0, (32, 3, 2)).astype(np.float32), texture={"file": "wall.ppm"})
    js = scenes.export_json_obj(wall["builder"], tmp_path, 96, 64, *wall["camera"])

    def glrt_main(extra, name):
        out = tmp_path / name
        r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", "4", "--frames", "6", "--frames-in-flight", "3", "--out", str(out),
                            "--extensions"] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "textures: 1," in r.stdout
        return np.asarray(Image.open(out)), r.stdout

    plain, log = glrt_main([], "plain.png")
    assert "texture wavefront" not in log
    twf, log = glrt_main(["--texture-wavefront"], "twf.png")
    assert "texture wavefront" in log
    assert plain.shape == (64, 96, 4) and np.array_equal(plain, twf), int((plain != twf).any(-1).sum())
