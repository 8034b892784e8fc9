"""Material maps on the GPU (csrc/maps.hip.h; include/glrtx.h "Material maps").  The rule's kernel equals the CPU statement bit for bit on the CPU test's batch.
The shading is pinned THROUGH the reference: flat normal maps and a roughness map of the conductor's own alphas render c1 as the oracle does, bit for bit and
ray for ray; a roughness map constant over each cell renders the oracle's image of one conductor a cell; a constant tilted map lights a quad as the oracle lights
the same quad with tilted vertex normals.  The feature pass's plane N carries n' of the primary hit, also after the geometry moved; flat maps combine with
albedo textures, an environment, a sphere and a dielectric without changing a bit; refusals leave the context rendering what it rendered."""
import functools

import numpy as np
import pytest

import maps_cases
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

N = 6
F = np.float32
SEEDS = [host.frame_seed(0), host.frame_seed(1)]
FLAT = (np.tile(F([0.5, 0.5, 1.0]), (2, 2, 1)), "rgba32f", "repeat", "bilinear")


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
    d.set_variant(2); d.count_rays(True); d.set_extensions(ext); d.track_motion(False)
    d.upload_environment(None); d.upload_scene(scene); d.upload_spheres(spheres); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


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


def _flat_everywhere(scene, k=0):
    """texture k as the normal map of every diffuse and conductor material"""
    t = _types(scene)
    return np.where((t == 2) | (t == 3), k, -1).astype(np.int32)


# ---- 1. the rule
@pytest.mark.parametrize("scale", maps_cases.SCALES)
def test_map_normal_kernel_equals_the_host_statement(gpu_device, scale):
    rec = maps_cases.batch()
    got, ref = device.debug_map_normal(rec, scale), host.map_normal(rec, scale)
    bad = (_bits(got) != _bits(ref)).any(1)
    assert not bad.any(), f"scale {scale}: {int(bad.sum())} of {bad.size} records differ; first {np.flatnonzero(bad)[0]}: {got[bad][0].tolist()} vs {ref[bad][0].tolist()}"


# ---- 2. flat maps = the reference
def test_flat_maps_render_the_reference_image(dev):
    scene, params = scenes.config_c1(64, 64, max_depth=4, n_samples=2, subdiv=1)
    ref, rays = _oracle(scene, params)
    t = _types(scene)
    mat = scene["mat"].reshape(-1, 18)
    cu = int(np.flatnonzero(t == 3)[0])
    assert (t == 3).sum() == 1 and mat[cu, 12] == mat[cu, 13]
    rough = (np.tile(F([mat[cu, 12], mat[cu, 13], 0.0]), (3, 3, 1)), "rgba32f", "clamp", "bilinear")  # exactly the conductor's alphas
    _setup(dev, scene, params)
    dev.upload_textures([FLAT, rough], _none(scene))  # a set that binds no albedo at all
    dev.bind_material_maps(normal=_flat_everywhere(scene), roughness=np.where(t == 3, 1, -1))
    got, st = _frames(dev, params)
    assert st.variant_last == 1
    _same(got, ref, "flat normal maps and the conductor's own roughness on c1")
    assert st.rays == rays


# ---- 3. per-cell roughness = one conductor per cell
@functools.lru_cache(maxsize=None)
def _rough_wall():
    map_scene, params, wall = scenes.config_mapped_wall(n=N)
    cell_scene, cell_params, cells = scenes.config_mapped_wall(n=N, per_cell=True)
    # preconditions: a failure of either is a broken test
    assert np.array_equal(map_scene["bvh"], cell_scene["bvh"]) and np.array_equal(_bits(wall["alpha"]), _bits(cells["alpha"]))
    assert wall["alpha"].min() >= 0.05 and wall["alpha"].max() <= 0.5
    ref, rays = _oracle(cell_scene, cell_params)
    one, _ = _oracle(map_scene, params)  # the one-material image: alpha 0.2 everywhere
    differ = (_bits(ref) != _bits(one)).any(-1).mean()
    assert differ >= 1.0 / 3.0, f"the per-cell image differs from the one-material image on {differ:.0%} of the pixels: the comparison would not see the roughness"
    return map_scene, params, wall, ref, rays


def _alpha_texture(alpha, filt="nearest", block=1):
    """alpha (n, n, 2): texel [j, i] = (ax, ay, 0) of cell (column i, row j), each repeated block x block times."""
    a = np.concatenate([alpha, np.zeros(alpha.shape[:2] + (1,), F)], -1).astype(F)
    return (np.repeat(np.repeat(a, block, 0), block, 1), "rgba32f", "repeat", filt)


@pytest.mark.parametrize("form", ["nearest", "bilinear-blocks"])
def test_per_cell_roughness_renders_one_conductor_per_cell(dev, form):
    scene, params, wall, ref, rays = _rough_wall()
    tex = _alpha_texture(wall["alpha"]) if form == "nearest" else _alpha_texture(wall["alpha"], "bilinear", 2)
    rough = _none(scene)
    rough[wall["material"]] = 0
    _setup(dev, scene, params)
    dev.upload_textures([tex], _none(scene))
    dev.bind_material_maps(roughness=rough)
    got, st = _frames(dev, params)
    assert st.variant_last == 1
    _same(got, ref, form)
    assert st.rays == rays


# ---- 4. a tilted map is a tilted normal
TILT = np.deg2rad(30.0)
TILT_SEEDS = [host.frame_seed(20 + k) for k in range(8)]


@functools.lru_cache(maxsize=None)
def _tilt_scene(n_samples=16):
    """A diffuse quad y = 0 with s along +x and t along -z, and a small emitter 45 degrees towards +s from the quad's centre, facing it.  (The tilted image is
    DARKER than the untilted one, not brighter, and black on the emitter's side.  That is the reference's spawn rule meeting a shading normal that leaves the
    geometric one: the shadow ray starts at the hit pushed EPS along the ray and then n' * EPS along the normal, which with a tilted n' can stay under the surface,
    or shorten the ray by nearly EPS where n' points at the emitter -- and the acceptance test |dist - t| < EPS then rejects the sample.  The oracle
    with tilted vertex normals does exactly the same, which is what the comparison is about.)"""
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    lamp = b.add_material(scenes.emitter((40.0, 40.0, 40.0)))
    pos, nrm = scenes.quad((-2, 0, 2), (4, 0, 0), (0, 0, -4))
    st = np.array([[[0, 0], [1, 0], [1, 1]], [[0, 0], [1, 1], [0, 1]]], F)
    b.add_mesh(pos, nrm, grey, uv=st)
    b.add_mesh(*scenes.quad((3.0, 3.25, -0.25), (0.35, -0.35, 0), (0, 0, 0.5)), lamp)  # normal towards (-1, -1, 0)
    scene = b.build()
    w, h = 32, 24
    c2w, s2c = scenes.camera((0, 5, 3), (0, 0, 0), (0, 1, 0), 40.0, w, h)
    params = scenes.make_params(c2w, s2c, w, h, 2, n_samples)
    a = host.render_features(scene, params)[1]
    on_quad = a[..., 3].view(np.int32) == grey
    assert on_quad.mean() > 0.3
    # the oracle's quad: vertex normals set to the host statement's result for the constant texel
    m = host.map_decode(((F([np.sin(TILT), 0.0, np.cos(TILT)]) + F(1)) / F(2))[None])
    v = scene["vert"].reshape(-1, 5, 3)
    rec = host.map_records(v[0:6, 1], np.repeat(v[[1, 4], 0] - v[[0, 3], 0], 3, 0), np.repeat(v[[2, 5], 0] - v[[0, 3], 0], 3, 0), np.repeat(v[[0, 3], 2, :2], 3, 0),
                           np.repeat(v[[1, 4], 2, :2], 3, 0), np.repeat(v[[2, 5], 2, :2], 3, 0), np.repeat(m, 6, 0))
    tilted = v.copy()
    tilted[0:6, 1] = host.map_normal(rec, 1.0)
    assert np.abs(tilted[0:6, 1] - [np.sin(TILT), np.cos(TILT), 0.0]).max() < 1e-6
    return scene, params, grey, on_quad, dict(scene, vert=tilted.reshape(-1, 3))


def _seed_means(render_one, on_quad):
    """mean radiance over the quad's pixels, one value a seed"""
    out = []
    for sd in TILT_SEEDS:
        acc = render_one(sd)
        out.append(float((acc[..., :3] / acc[..., 3:])[on_quad].mean()))
    return np.array(out)


def test_a_tilted_map_is_a_tilted_normal(dev):
    scene, params, grey, on_quad, tilted_scene = _tilt_scene()
    ref = _seed_means(lambda sd: pt_oracle.render(tilted_scene, dict(params, seed=sd))[0], on_quad)
    flat = _seed_means(lambda sd: pt_oracle.render(scene, dict(params, seed=sd))[0], on_quad)
    se = ref.std(ddof=1) / np.sqrt(len(ref))
    assert abs(flat.mean() - ref.mean()) > 10 * se, f"precondition: untilted {flat.mean():.5f} vs tilted {ref.mean():.5f}, standard error {se:.5f}: raise the sample count"
    texel = (F([np.sin(TILT), 0.0, np.cos(TILT)]) + F(1)) / F(2)
    normal = _none(scene)
    normal[grey] = 0
    _setup(dev, scene, params)
    dev.upload_textures([(np.tile(texel, (4, 4, 1)), "rgba32f", "repeat", "bilinear")], _none(scene))
    dev.bind_material_maps(normal=normal)

    def gpu(sd):
        dev.clear()
        dev.render(dict(params, seed=sd))
        dev.sync()
        return dev.read_accum()

    got = _seed_means(gpu, on_quad)
    diff = abs(got.mean() - ref.mean())
    print(f"mean radiance over the quad: GPU {got.mean():.6f}, oracle (tilted vertex normals) {ref.mean():.6f}, untilted {flat.mean():.6f}; "
          f"difference {diff:.3e}, standard error {se:.3e}")
    assert diff <= 3 * se, f"difference {diff:.3e} exceeds 3 standard errors ({3 * se:.3e}) of the oracle's mean {ref.mean():.6f} (GPU {got.mean():.6f})"


# ---- 5. / 6. the feature plane carries n'
def _bump_map(seed=5):
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.uniform(-0.6, 0.6, (8, 8, 2)), np.ones((8, 8, 1))], -1)
    m /= np.linalg.norm(m, axis=-1, keepdims=True)
    return ((m + 1.0) / 2.0).astype(F)


def _expected_plane_n(scene, st_scene, tex, k, scale, mapped_materials, ref_n, g):
    """ref_n with the normal of every pixel whose plane G names a triangle of a mapped material replaced by host.map_normal of that triangle's record (edges
    and normals from `scene`, coordinates from `st_scene`: the table is frozen) and the map's texel at the hit."""
    v, vs = scene["vert"].reshape(-1, 5, 3), st_scene["vert"].reshape(-1, 5, 3)
    tri = scene["tri"].reshape(-1, 4)
    t = g[..., 0].view(np.int32)
    hit = t >= 0
    mapped = np.zeros(t.shape, bool)
    mapped[hit] = np.isin(tri[t[hit], 3].astype(np.int32), mapped_materials)
    i = tri[t[mapped], 0:3].astype(np.int64)
    u, w = g[mapped][:, 1], g[mapped][:, 2]
    st = [vs[i[:, c], 2, :2] for c in range(3)]
    w0 = (F(1) - u) - w
    s = (w0 * st[0][:, 0] + u * st[1][:, 0]) + w * st[2][:, 0]
    q = (w0 * st[0][:, 1] + u * st[1][:, 1]) + w * st[2][:, 1]
    c = host.texture_lookup(tex, np.full(s.size, k, np.int32), np.stack([s, q], 1))
    rec = host.map_records(ref_n[mapped][:, :3], v[i[:, 1], 0] - v[i[:, 0], 0], v[i[:, 2], 0] - v[i[:, 0], 0], st[0], st[1], st[2], host.map_decode(c))
    want = ref_n.copy()
    want[mapped, :3] = host.map_normal(rec, scale)
    return want, mapped


def _feature_case(dev, scene, params, wall, ref_scene, what):
    tex = [(_bump_map(), "rgba32f", "repeat", "bilinear")]
    ref_n, ref_a, ref_g = host.render_features_geom(ref_scene, params)
    dev.track_motion(True)
    dev.render_features(params)
    n, a = dev.read_features()
    g = dev.read_features_geom()
    _same(g, ref_g, f"{what}: plane G"); _same(a, ref_a, f"{what}: plane A")
    want, mapped = _expected_plane_n(ref_scene, scene, tex, 0, 0.75, [wall["material"]], ref_n, g)
    assert mapped.mean() > 0.1, mapped.mean()
    changed = (_bits(want[mapped][:, :3]) != _bits(ref_n[mapped][:, :3])).any(-1)
    assert changed.mean() > 0.9  # the map is not flat: the comparison sees n'
    _same(n, want, f"{what}: plane N against host.map_normal(plane G)")
    dev.track_motion(False)  # without G: the *_maps kernels
    dev.render_features(params)
    _same(dev.read_features()[0], want, f"{what}: plane N without G")
    return ref_n


@pytest.mark.parametrize("kind", ["diffuse", "conductor"])
def test_feature_plane_n_carries_the_mapped_normal(dev, monkeypatch, kind):
    scene, params, wall = scenes.config_mapped_wall(n=N, wall=kind, uv="corner")
    normal = _none(scene)
    normal[wall["material"]] = 0
    _setup(dev, scene, params)
    dev.upload_textures([(_bump_map(), "rgba32f", "repeat", "bilinear")], _none(scene))
    dev.bind_material_maps(normal=normal, normal_scale=0.75)
    for compact in ("0", "1"):
        monkeypatch.setenv("GLRTX_COMPACT_NODES", compact)
        ref_n = _feature_case(dev, scene, params, wall, scene, f"{kind} compact={compact}")
    monkeypatch.delenv("GLRTX_COMPACT_NODES")
    dev.bind_material_maps()
    dev.render_features(params)
    _same(dev.read_features()[0], ref_n, "unbound: plane N is surf_tri's again")


def test_the_frame_follows_a_move(dev):
    scene, params, wall = scenes.config_mapped_wall(n=N, wall="diffuse", uv="corner")
    normal = _none(scene)
    normal[wall["material"]] = 0
    moved = scene["vert"].reshape(-1, 5, 3).copy()
    r = slice(wall["vert"].start, wall["vert"].stop)
    for row in (0, 1):  # the wall turned by 90 degrees about y: (x, y, z) -> (z, y, -x), positions and normals; exact
        moved[r, row] = np.stack([moved[r, row, 2], moved[r, row, 1], -moved[r, row, 0]], -1)
    moved[r, 2, :2] = 0.0  # the update's own uv words are not read: the {s, t} table is the upload's
    ref_scene = dict(scene, vert=moved.reshape(-1, 3))
    ref_scene["bvh"] = host.refit_bvh(ref_scene["vert"], ref_scene["tri"], scene["bvh"])
    _setup(dev, scene, params)
    dev.upload_textures([(_bump_map(), "rgba32f", "repeat", "bilinear")], _none(scene))
    dev.bind_material_maps(normal=normal, normal_scale=0.75)
    dev.update_vertices(moved.reshape(-1, 15))
    _feature_case(dev, scene, params, wall, ref_scene, "after update_vertices")


# ---- 7. combinations, against the existing kernels
@pytest.mark.parametrize("extras", [False, True])
def test_flat_maps_change_nothing_next_to_the_other_extensions(dev, extras):
    scene, params, wall = scenes.config_textured_wall(n=N)
    spheres, ext = None, 0
    if extras:
        glass = np.array(scenes._mat_rows(scenes.dielectric(1.5)), F)
        g = scene["mat"].reshape(-1, 18).shape[0]
        scene = dict(scene, mat=np.concatenate([scene["mat"].reshape(-1, 3), glass], 0))
        spheres, ext = np.array([[-2.4, 0.8, 1.0, 0.8, g]], F), device.EXT_DIELECTRIC
    albedo = _none(scene)
    albedo[wall["material"]] = 1
    tex = [FLAT, (np.repeat(np.repeat(wall["albedo"], 2, 0), 2, 1), "rgba32f", "repeat", "bilinear")]
    _setup(dev, scene, params, spheres=spheres, ext=ext)
    dev.upload_textures(tex, albedo)
    dev.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape"))
    try:
        ref, st0 = _frames(dev, params)
        dev.bind_material_maps(normal=_flat_everywhere(scene))
        got, st = _frames(dev, params)
        assert st.variant_last == 1
        _same(got, ref, f"albedo + environment + flat maps (extras={extras})")
        assert st.rays == st0.rays
        # without the environment: pt_render_persistent's TEX + MAPS form against its TEX form
        dev.upload_environment(None)
        got, st = _frames(dev, params)
        dev.bind_material_maps()
        ref, st0 = _frames(dev, params)
        _same(got, ref, f"albedo + flat maps (extras={extras})")
        assert st.rays == st0.rays
    finally:
        dev.upload_environment(None)
        dev.set_extensions(0)


# ---- 8. call order and refusals
def test_call_order_and_refusals(dev):
    scene, params, wall, ref, rays = _rough_wall()
    n_mat = _types(scene).size
    srgb = (np.full((2, 2, 4), 128, np.uint8), "rgba8_srgb", "repeat", "nearest")
    tex = [_alpha_texture(wall["alpha"]), srgb]
    rough = _none(scene)
    rough[wall["material"]] = 0
    d = device.Device()
    try:
        with pytest.raises(device.GlrtxError, match="no texture set is bound"):
            d.bind_material_maps(roughness=rough)
        d.upload_scene(scene)
        with pytest.raises(device.GlrtxError, match="no texture set is bound"):
            d.bind_material_maps(roughness=rough)
    finally:
        d.close()
    _setup(dev, scene, params)
    dev.upload_textures(tex, _none(scene))
    unmapped, st0 = _frames(dev, params)
    assert st0.variant_last == 1
    dev.bind_material_maps(roughness=rough)

    def refused(words, **kw):
        with pytest.raises(device.GlrtxError, match=words) as e:
            dev.bind_material_maps(**kw)
        assert e.value.code == device.GLRTX_EINVAL
        got, st = _frames(dev, params)
        _same(got, ref, f"after the refusal '{words}'")
        assert st.variant_last == 1 and st.rays == rays

    def at(material, k):
        a = _none(scene)
        a[material] = k
        return a

    w, t = wall["material"], _types(scene)
    grey, lamp = int(np.flatnonzero(t == 2)[0]), int(np.flatnonzero(t == 1)[0])
    refused(f"{n_mat - 1} records, the scene has {n_mat} materials", roughness=rough[:-1])
    refused(f"material {w}: roughness map 2 of 2 textures", roughness=at(w, 2))
    refused(f"material {w}: normal map -2 of 2 textures", normal=at(w, -2))
    refused(f"material {lamp} has a normal map and is neither diffuse nor conductor", normal=at(lamp, 0))
    refused(f"material {grey} has a roughness map and is not a conductor", roughness=at(grey, 0))
    refused(f"material {lamp} has a roughness map and is not a conductor", roughness=at(lamp, 0))
    refused(f"material {w}: roughness map 1 has format GLRTX_TEX_RGBA8_SRGB", roughness=at(w, 1))
    refused(f"material {grey}: normal map 1 has format GLRTX_TEX_RGBA8_SRGB", normal=at(grey, 1))
    for bad in (np.inf, -np.inf, np.nan):
        refused(f"material {w}: normal_scale is not finite", roughness=rough, normal_scale=np.where(np.arange(n_mat) == w, bad, 1.0))
    rec = host.material_maps(n_mat, roughness=rough)
    rec["reserved"][grey] = 7
    refused(f"material {grey}: reserved is 7", normal=rec)
    # the wavefront kernel's calls still say "textures are bound"
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.render_adaptive(params, SEEDS, 0.05)
    with pytest.raises(device.GlrtxError, match="textures are bound"):
        dev.hit_histogram(params, scene["tri"].reshape(-1, 4).shape[0])
    got, st = _frames(dev, params)
    _same(got, ref, "after the refused calls")
    # maps == NULL unbinds, and binding again maps again
    dev.bind_material_maps()
    _same(_frames(dev, params)[0], unmapped, "unbound")
    dev.bind_material_maps(roughness=rough)
    _same(_frames(dev, params)[0], ref, "bound again")
    # upload_textures drops the maps: the next image is the unmapped one
    dev.upload_textures(tex, _none(scene))
    _same(_frames(dev, params)[0], unmapped, "after upload_textures")
    # ... and so does unbinding the set, and upload_scene
    dev.bind_material_maps(roughness=rough)
    dev.upload_textures(None, None)
    with pytest.raises(device.GlrtxError, match="no texture set is bound"):
        dev.bind_material_maps(roughness=rough)
    dev.upload_textures(tex, _none(scene))
    dev.bind_material_maps(roughness=rough)
    dev.upload_scene(scene)
    got, st = _frames(dev, params)
    assert st.variant_last == 2
    with pytest.raises(device.GlrtxError, match="no texture set is bound"):
        dev.bind_material_maps(roughness=rough)
