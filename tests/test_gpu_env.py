"""Environment lighting on the GPU (csrc/environment.hip.h; include/glrtx.h "Environment").  The three debug hooks equal the host statements bit for bit on the
CPU test's cases.  A black environment is pinned THROUGH the reference: with a map of zeros, with scale 0, and in sampled mode with light_pick 0 in a closed
room, image and ray count are the oracle's.  The orientation is checked texel by texel, a constant environment against the furnace value, and both estimators
against the analytic irradiance of a map with a bright spot, within a tolerance derived from each estimator's own variance.  Refusals leave the context
rendering what it rendered."""
import functools

import numpy as np
import pytest

import env_cases as ec
import query_rays
from glrt_amd import device, host, scenes
from oracle import pt_oracle

pytestmark = pytest.mark.gpu

F = np.float32
SEEDS = [host.frame_seed(0), host.frame_seed(1)]


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


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
    d.upload_environment(None); d.upload_scene(scene); d.upload_spheres(spheres); d.resize(params["width"], params["height"]); d.clear(); d.reset_stats()


def _frames(d, params, seeds=SEEDS):
    d.clear(); d.reset_stats()
    for sd in seeds:
        d.render(dict(params, seed=sd))
    d.sync()
    return d.read_accum(), d.stats()


def _bright(n=16, seed=11):
    return (np.random.default_rng(seed).uniform(0.5, 8.0, (n, n, 4)).astype(F), "rgba32f", "bilinear")


ZERO = (np.zeros((8, 8, 4), F), "rgba32f", "bilinear")


@functools.lru_cache(maxsize=None)
def _c1():
    """c1 (64 x 64, depth 4, two frames of 2 spp), the oracle's image of it, and the share of its primary centre rays that miss."""
    scene, params = scenes.config_c1(64, 64, max_depth=4, n_samples=2, subdiv=1)
    ref, rays = _oracle(scene, params)
    _, tri, _, _ = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], query_rays.camera_rays(params))
    return scene, params, ref, rays, float((tri < 0).mean())


# ---- 1. the statements agree
@pytest.mark.parametrize("k", range(len(ec.maps())))
def test_debug_hooks_equal_the_host_statements(gpu_device, k):
    name, env_map, kw = ec.maps()[k]
    cfg = host.env_cfg(**kw)
    gw, hw = device.debug_env_weights(env_map, cfg), host.env_weights(env_map, cfg)
    assert gw.shape == hw.shape and np.array_equal(_bits(gw), _bits(hw)), f"{name}: {int((_bits(gw) != _bits(hw)).sum())} of {hw.size} cell weights differ"
    u, d = ec.uniforms(), ec.directions()
    gs, hs = device.debug_env_sample(env_map, cfg, u), host.env_sample(env_map, cfg, u)
    bad = (_bits(gs) != _bits(hs)).any(1)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} samples differ; first at {u[bad][0].tolist()}: {gs[bad][0].tolist()} vs {hs[bad][0].tolist()}"
    ge, he = device.debug_env_eval(env_map, cfg, d), host.env_eval(env_map, cfg, d)
    bad = (_bits(ge) != _bits(he)).any(1)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} evaluations differ; first at {d[bad][0].tolist()}: {ge[bad][0].tolist()} vs {he[bad][0].tolist()}"


# ---- 2. black is the reference
@pytest.mark.parametrize("form", ["zero map", "scale 0"])
def test_black_escape_environment_renders_the_oracle_image(dev, form):
    scene, params, ref, rays, missing = _c1()
    assert missing >= 1.0 / 3.0, f"only {missing:.0%} of c1's primary rays miss: the comparison would not see the miss path"
    _setup(dev, scene, params)
    if form == "zero map":
        dev.upload_environment(ZERO, host.env_cfg("escape"))
    else:
        dev.upload_environment(_bright(), host.env_cfg("escape", scale=0.0))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and st.fallback_last == device.FALLBACK_EXTENSIONS
    _same(got, ref, form)
    assert st.rays == rays


def test_black_environment_beside_spheres_and_a_dielectric(dev):
    scene, params, spheres = scenes.config_spheres(64, 64, max_depth=4, n_samples=2, glass=True)
    ref, rays = _oracle(scene, params, spheres=spheres, ext_flags=device.EXT_DIELECTRIC)
    _setup(dev, scene, params, spheres=spheres, ext=device.EXT_DIELECTRIC)
    dev.upload_environment(ZERO, host.env_cfg("escape"))
    got, st = _frames(dev, params)
    dev.set_extensions(0)
    assert st.variant_last == 1
    _same(got, ref, "spheres + dielectric + a zero map")
    assert st.rays == rays


# ---- 3. sampled mode with light_pick 0 is the reference
def test_sampled_mode_without_a_pick_is_the_oracle_in_a_closed_room(dev):
    scene, params = scenes.config_env_box()
    _, tri, _, _ = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], query_rays.camera_rays(params))
    assert (tri >= 0).all(), "the room is closed: no primary ray leaves it"
    ref, rays = _oracle(scene, params)
    _setup(dev, scene, params)
    dev.upload_environment(_bright(), host.env_cfg("sampled", light_pick=0.0, scale=50.0))
    got, st = _frames(dev, params)
    assert st.variant_last == 1
    _same(got, ref, "a bright map, sampled, light_pick 0, closed room")
    assert st.rays == rays


def test_sampled_mode_without_a_pick_and_a_zero_map_is_the_oracle_on_c1(dev):
    scene, params, ref, rays, _ = _c1()
    _setup(dev, scene, params)
    dev.upload_environment(ZERO, host.env_cfg("sampled", light_pick=0.0))
    got, st = _frames(dev, params)
    _same(got, ref, "a zero map, sampled, light_pick 0")
    assert st.rays == rays


# ---- 4. orientation
def _texel_of(d, R=np.eye(3)):
    """The texel [y, x] of a 4 x 4 map a direction reads, in float64 from the header's rule (an independent statement for this test)."""
    e = np.asarray(d, np.float64) @ np.asarray(R, np.float64).reshape(3, 3).T
    p = e / np.abs(e).sum(-1, keepdims=True)
    px, pz = p[..., 0], p[..., 2]
    lower = e[..., 1] < 0
    fx = (1 - np.abs(pz)) * np.where(px < 0, -1, 1)
    fz = (1 - np.abs(px)) * np.where(pz < 0, -1, 1)
    px, pz = np.where(lower, fx, px), np.where(lower, fz, pz)
    ix = np.clip(np.floor((px * 0.5 + 0.5) * 4), 0, 3).astype(int)
    iy = np.clip(np.floor((pz * 0.5 + 0.5) * 4), 0, 3).astype(int)
    return iy, ix


VIEWS = [tuple(float(v) for v in a) for a in ec.axes()] + [tuple(float(v) for v in f) for f in ec.face_centres()]


@pytest.mark.parametrize("turned", [False, True])
def test_every_pixel_shows_its_octants_texel(dev, turned):
    tex = scenes.env_octant_map()
    R = ec.QUARTER_TURN if turned else (1, 0, 0, 0, 1, 0, 0, 0, 1)
    seen = set()
    for view in VIEWS:
        scene, params = scenes.config_env_sky(view)
        _setup(dev, scene, params)
        dev.upload_environment((tex, "rgba32f", "nearest"), host.env_cfg("escape", rotation=R))
        got, st = _frames(dev, params, SEEDS[:1])
        assert st.variant_last == 1 and (got[..., 3] == 1).all()
        h, w = params["height"], params["width"]
        # the texel at the middle and at the four corners of the pixel's footprint: where they agree the pixel must show exactly that texel, elsewhere one of them
        c2w = np.asarray(params["c2w"], np.float64).reshape(4, 4).T
        s2c = np.asarray(params["s2c"], np.float64).reshape(4, 4).T
        cand = []
        # (a sample of pixel x goes through x + 0.5 + r, r in [0, 1): the reference adds its jitter to gl_FragCoord, the pixel's centre -- main() :577)
        for ox, oy in ((1.0, 1.0), (0.52, 0.52), (1.48, 0.52), (0.52, 1.48), (1.48, 1.48)):
            y, x = np.mgrid[0:h, 0:w]
            ndc = np.stack([(x + ox) / w * 2 - 1, (y + oy) / h * 2 - 1, np.ones((h, w)), np.ones((h, w))], -1)
            p = ndc @ s2c.T
            d = (p[..., :3] / p[..., 3:4]) @ c2w[:3, :3].T
            iy, ix = _texel_of(d, R)
            cand.append(tex[iy, ix])
        centre, corners = cand[0], cand[1:]
        sure = np.all([(_bits(c) == _bits(centre)).all(-1) for c in corners], 0)
        assert sure.mean() > 0.9, view
        bad = sure & (_bits(got[..., :3]) != _bits(centre)).any(-1)
        assert not bad.any(), f"view {view}, turned {turned}: {int(bad.sum())} pixels show another texel; first {np.argwhere(bad)[0].tolist()}"
        loose = ~sure & ~np.any([(_bits(got[..., :3]) == _bits(c)).all(-1) for c in cand], 0)
        assert not loose.any(), f"view {view}: a pixel on a texel boundary shows neither neighbour"
        if all(abs(v) == 1.0 for v in view):  # a diagonal: the whole view lies in one octant, one texel
            assert sure.all() and len({tuple(r) for r in _bits(got[..., :3]).reshape(-1, 3).tolist()}) == 1, view
            seen.add(tuple(_bits(got[0, 0, :3]).tolist()))
    assert len(seen) == 8, "the eight octants show eight different texels"
    if turned:  # the colours move as stated: what the map holds along +z is seen along world +x
        scene, params = scenes.config_env_sky((1.0, 0.3, 0.3))
        _setup(dev, scene, params)
        dev.upload_environment((tex, "rgba32f", "nearest"), host.env_cfg("escape", rotation=R))
        a, _ = _frames(dev, params, SEEDS[:1])
        iy, ix = _texel_of(np.array([-0.3, 0.3, 1.0]))
        _same(a[..., :3], np.broadcast_to(tex[iy, ix], a[..., :3].shape), "a quarter turn about y")


# ---- 5. the furnace
def test_furnace_in_escape_mode(dev):
    """beta = f cw / pdf = rho (n . w) / wlz with wlz >= 2^-12 and a rotated cosine that carries an absolute error of a few 2^-24: every sample is rho E to 1e-3."""
    scene, params = scenes.config_env_quad(max_depth=2, n_samples=4)
    _, tri, _, _ = host.trace_rays(scene["vert"], scene["tri"], scene["bvh"], query_rays.camera_rays(params))
    assert (tri >= 0).all(), "the quad fills the view"
    _setup(dev, scene, params)
    dev.upload_environment((np.ones((8, 8, 4), F), "rgba32f", "bilinear"), host.env_cfg("escape"))
    got, st = _frames(dev, params)
    mean = got[..., :3] / got[..., 3:4]
    rho = np.asarray(scenes.ENV_QUAD_ALBEDO, F)
    err = np.abs(mean / rho - 1).max()
    print(f"furnace: max relative error {err:.3e}")
    assert (got[..., 3] == 8).all() and err <= 1e-3, err


# ---- 6. both modes meet the analytic value
N_MAP, SUB = 32, 64
SPOT = (slice(18, 20), slice(18, 20))  # a 2 x 2 block of the upper half (u = v = 0.16 .. 0.25)


def _spot_map():
    a = np.full((N_MAP, N_MAP, 4), 0.25, F)
    a[SPOT] = 64.0
    return a


@functools.lru_cache(maxsize=None)
def _analytic():
    """From the texel data alone, in float64: a 64 x 64 midpoint quadrature a texel of the quad's irradiance integrals.  Returns (mu (3,), var_escape (3,),
    var_sampled (3,), bound (3,)): the expected pixel value, each estimator's per-sample variance and the largest sample sampled mode can produce."""
    le = _spot_map()[..., 0].astype(np.float64)
    n, m = N_MAP, N_MAP * SUB
    c = (np.arange(m) + 0.5) / m
    s, t = np.meshgrid(c, c)
    u, v = 2 * s - 1, 2 * t - 1
    y = 1 - np.abs(u) - np.abs(v)
    x = np.where(y < 0, (1 - np.abs(v)) * np.where(u < 0, -1, 1), u)
    z = np.where(y < 0, (1 - np.abs(u)) * np.where(v < 0, -1, 1), v)
    r = 1 / np.sqrt(x * x + y * y + z * z)
    jac = 4 * ((np.abs(x) + np.abs(y) + np.abs(z)) * r) ** 3
    cos = np.maximum(y * r, 0.0)
    L = np.repeat(np.repeat(le, SUB, 0), SUB, 1)
    dA = 1.0 / m ** 2
    # the grid's pdf: one cell a texel (G = min(N, 256) = N), weights over the texel block widened by one, luminance of a grey texel = its value
    cc = (np.arange(n) + 0.5) / n
    cs, ct = np.meshgrid(cc, cc)
    cu, cv = 2 * cs - 1, 2 * ct - 1
    cy = 1 - np.abs(cu) - np.abs(cv)
    cx = np.where(cy < 0, (1 - np.abs(cv)) * np.where(cu < 0, -1, 1), cu)
    cz = np.where(cy < 0, (1 - np.abs(cu)) * np.where(cv < 0, -1, 1), cv)
    w_texel = le * (0.2126 + 0.7152 + 0.0722) * 4 * ((np.abs(cx) + np.abs(cy) + np.abs(cz)) / np.sqrt(cx * cx + cy * cy + cz * cz)) ** 3
    pad = np.pad(w_texel, 1)
    w_cell = sum(pad[1 + dy:1 + dy + n, 1 + dx:1 + dx + n] for dy in (-1, 0, 1) for dx in (-1, 0, 1))
    p_cell = w_cell / w_cell.sum()
    pdf = np.repeat(np.repeat(p_cell * n * n, SUB, 0), SUB, 1) / jac
    rho = np.asarray(scenes.ENV_QUAD_ALBEDO, np.float64)
    irr = (L * cos * jac).sum() * dA
    mu = rho / np.pi * irr
    second_escape = (L ** 2 * cos * jac).sum() * dA / np.pi          # integral of (f Le cos)^2 / (cos / pi), without rho^2
    second_sampled = ((L * cos) ** 2 / pdf * jac).sum() * dA / np.pi ** 2
    bound = (rho / np.pi) * (L * cos / pdf).max()
    return mu, rho ** 2 * second_escape - mu ** 2, rho ** 2 * second_sampled - mu ** 2, bound


@functools.lru_cache(maxsize=None)
def _spot_images():
    """{mode: mean image (48, 64, 3)} of the quad under the spot map, kept by the test below for the variance ratio it prints."""
    return {}


@pytest.mark.parametrize("mode", ["escape", "sampled"])
def test_both_modes_meet_the_analytic_irradiance(dev, mode):
    """The image mean of each mode within 6 standard errors, sigma / sqrt(pixels * samples), plus 0.5 % of the expected value (quadrature, the tables' rounding).
    Measured on the MI355X with these two frames: escape 1.117 mu (5.6 SE), sampled 1.025 mu (5.5 SE).  Other frames give -5.4, -3.9, +0.7, -1.8 SE (escape) and
    -3.0, -3.4, +3.9, +1.3 SE (sampled), and 128 frames of sampled mode 0.9996 mu: the sign changes and the mean converges, so there is no bias -- but the
    pixels' sin-hash streams (the reference's rand()) are not independent of each other, and the spread is wider than one SE.  The per-pixel image variance is
    what the quadrature predicts (0.507 against 14.49 / 32 for escape, 0.0215 against 0.681 / 32 for sampled)."""
    mu, var_e, var_s, bound = _analytic()
    scene, params = scenes.config_env_quad(max_depth=2, n_samples=16)
    assert 0.75 * 64 < 100 and bound.max() < 100, "every sample stays under the accumulation clamp"
    _setup(dev, scene, params)
    dev.upload_environment((_spot_map(), "rgba32f", "nearest"), host.env_cfg(mode))
    got, st = _frames(dev, params)
    assert st.variant_last == 1 and (got[..., 3] == 32).all()
    img = (got[..., :3] / got[..., 3:4]).astype(np.float64)
    _spot_images()[mode] = img
    n = img.shape[0] * img.shape[1] * 32
    var = var_e if mode == "escape" else var_s
    tol = 6 * np.sqrt(var / n) + 0.005 * mu
    mean = img.reshape(-1, 3).mean(0)
    print(f"{mode}: image mean {mean.tolist()}, expected {mu.tolist()}, tolerance {tol.tolist()}, per-sample sigma {np.sqrt(var).tolist()}, "
          f"image variance {img.reshape(-1, 3).var(0).tolist()}")
    assert (np.abs(mean - mu) <= tol).all(), (mode, mean, mu, tol)
    if mode == "sampled":
        print(f"sampled: largest pixel {img.reshape(-1, 3).max(0).tolist()}, per-sample bound {bound.tolist()}")
        assert (img.reshape(-1, 3).max(0) <= bound * (1 + 1e-3)).all(), "a pixel above the per-sample bound: a wrong pdf shows as a firefly"
        if "escape" in _spot_images():
            ratio = _spot_images()["escape"].reshape(-1, 3).var(0) / img.reshape(-1, 3).var(0)
            print(f"image variance, escape / sampled: {ratio.tolist()}")


# ---- 7. combinations and refusals
def test_black_environment_beside_a_texture_set(dev):
    n = 6
    tex_scene, params, wall = scenes.config_textured_wall(n=n)
    cell_scene, cell_params, _ = scenes.config_textured_wall(n=n, per_cell=True)
    ref, rays = _oracle(cell_scene, cell_params)
    bind = np.full(tex_scene["mat"].reshape(-1, 18).shape[0], -1, np.int32)
    bind[wall["material"]] = 0
    _setup(dev, tex_scene, params)
    dev.upload_textures([(wall["albedo"], "rgba32f", "repeat", "nearest")], bind)
    dev.upload_environment(ZERO, host.env_cfg("escape"))
    got, st = _frames(dev, params)
    assert st.variant_last == 1
    _same(got, ref, "textures + a zero map")
    assert st.rays == rays
    dev.upload_environment(_bright(), host.env_cfg("sampled", light_pick=0.0, scale=0.0))
    got, st = _frames(dev, params)
    _same(got, ref, "textures + sampled mode, light_pick 0, scale 0")
    dev.upload_textures(None, None)


def test_refusals_and_unbinding(dev):
    scene, params, ref, rays, _ = _c1()
    _setup(dev, scene, params)
    plain, st = _frames(dev, params)
    assert st.variant_last == 2
    _same(plain, ref, "c1 without an environment")
    dev.render_features(params)
    planes = dev.read_features()
    env_map, cfg = _bright(), host.env_cfg("sampled", light_pick=0.5)
    dev.upload_environment(env_map, cfg)
    lit, st = _frames(dev, params)
    assert st.variant_last == 1 and (_bits(lit) != _bits(ref)).any(-1).mean() > 1.0 / 3.0
    # the feature pass is unchanged
    dev.render_features(params)
    for a, b in zip(planes, dev.read_features()):
        assert np.array_equal(_bits(a), _bits(b)), "the feature planes do not depend on the environment"

    def refused(text, call):
        with pytest.raises(device.GlrtxError, match=text) as e:
            call()
        assert e.value.code == device.GLRTX_EINVAL

    # configurations and maps that are refused name their offender and change nothing
    arr = env_map[0]
    refused("mode 2", lambda: dev.set_environment_cfg(host.env_cfg(2)))
    refused("grid 1025", lambda: dev.set_environment_cfg(host.env_cfg(grid=1025)))
    refused("grid -1", lambda: dev.set_environment_cfg(host.env_cfg(grid=-1)))
    refused("light_pick 1.5", lambda: dev.set_environment_cfg(host.env_cfg(light_pick=1.5)))
    refused("light_pick nan", lambda: dev.set_environment_cfg(host.env_cfg(light_pick=float("nan"))))
    refused(r"scale\[1\] = -1", lambda: dev.set_environment_cfg(host.env_cfg(scale=(1, -1, 1))))
    refused(r"scale\[2\] = inf", lambda: dev.set_environment_cfg(host.env_cfg(scale=(1, 1, np.inf))))
    refused(r"rotation\[4\] = nan", lambda: dev.set_environment_cfg(host.env_cfg(rotation=(1, 0, 0, 0, np.nan, 0, 0, 0, 1))))
    refused("NULL configuration", lambda: dev.set_environment_cfg(None))
    refused("16 x 8 texels", lambda: dev.upload_environment((arr[:8], "rgba32f", "bilinear"), cfg))
    refused("1 x 1 texels", lambda: dev.upload_environment((arr[:1, :1], "rgba32f", "bilinear"), cfg))
    desc, blob = host.pack_environment(env_map)
    for field, value, text in (("wrap_s", 0, "wrap mode 0 / 1"), ("wrap_t", 0, "wrap mode 1 / 0"), ("filter", 2, "unknown filter 2"), ("format", 3, "unknown format 3"),
                               ("offset", 8, "offset 8 is not a multiple of 16")):
        e = desc.copy()
        e[field] = value
        refused(text, lambda e=e: dev.upload_environment((e, blob), cfg))
    refused("its last texel lies past", lambda: dev.upload_environment((desc, blob[:-16]), cfg))
    again, st = _frames(dev, params)
    _same(again, lit, "after the refused configurations and maps")

    # the volume and the wavefront kernel's calls refuse while an environment is bound
    dens, temp = scenes.fire_grids((4, 4, 4))
    dev.upload_volume(dens, temp, (0, 0, 0), (1, 1, 1))
    dev.set_extensions(device.EXT_VOLUME)
    refused("an environment is bound", lambda: dev.render(dict(params, seed=SEEDS[0])))
    dev.set_extensions(0)
    dev.upload_volume(None, None, (0, 0, 0), (1, 1, 1))
    refused("an environment is bound", lambda: dev.render_adaptive(params, SEEDS, 0.05))
    dev.track_moments(True)
    refused("an environment is bound", lambda: dev.render_moments(params, SEEDS))
    refused("an environment is bound", lambda: dev.render_adaptive_moments(params, SEEDS, 0.05))
    dev.track_moments(False)
    dev.track_cascades(True)
    refused("an environment is bound", lambda: dev.render_cascades(params, SEEDS))
    dev.track_cascades(False)
    refused("an environment is bound", lambda: dev.hit_histogram(params, scene["tri"].reshape(-1, 4).shape[0]))
    again, st = _frames(dev, params)
    _same(again, lit, "after the refused calls")
    assert st.variant_last == 1

    # the configuration can change without the map; the map is kept across an upload of the scene
    dev.set_environment_cfg(host.env_cfg("escape", scale=0.0))
    black, st = _frames(dev, params)
    _same(black, ref, "scale 0 through set_environment_cfg")
    assert st.rays == rays
    dev.set_environment_cfg(cfg)
    dev.upload_scene(scene)
    again, st = _frames(dev, params)
    _same(again, lit, "after upload_scene and the first configuration again")

    # unbinding restores the untouched image
    dev.upload_environment(None)
    got, st = _frames(dev, params)
    assert st.variant_last == 2 and st.fallback_last == 0
    _same(got, plain, "after unbinding")
    refused("no environment is bound", lambda: dev.set_environment_cfg(cfg))
