"""Emission maps without a GPU (include/glrtx.h "Emission maps"; include/glrt_host.h): glrt_light_emission equals tests/emission_math.py bit for bit on random
lights and uniforms over 3 formats x 2 filters, the flip's boundary, a degenerate light, NaN, infinite and denormal coordinates and a 1 x 1 texture; Le is the
one rounded product emission * lookup; glrt_light_st is the vertices' uv words in wire order; glrt_emission_albedo is glrt_texture_albedo plus the texel at
a bound, non-diffuse hit; and the validator the device's binding call uses refuses what the header lists, with its messages."""
import numpy as np
import pytest

import emission_cases
import emission_math
import texture_math
from glrt_amd import host, scenes

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, ref, what):
    bad = (_bits(got) != _bits(ref)) & ~(np.isnan(got) & np.isnan(ref))
    assert not bad.any(), f"{what}: {int(bad.any(-1).sum())} of {bad.shape[0]} rows differ; first {np.argwhere(bad)[0].tolist()}: " \
                          f"{got[np.argwhere(bad)[0][0]].tolist()} vs {ref[np.argwhere(bad)[0][0]].tolist()}"


def test_light_emission_equals_the_numpy_statement():
    scene, tex, bind, lid, u = emission_cases.case()
    got, ref = host.light_emission(scene, tex, bind, lid, u), emission_math.light_emission(scene, tex, bind, lid, u)
    assert got.shape == (lid.size, 5)
    _same(got, ref, "glrt_light_emission")
    flipped = u[:, 0] + u[:, 1] > 1
    assert 0.3 < flipped.mean() < 0.7  # both sides of the flip are there
    assert np.isnan(got[:, :2]).any() and np.isfinite(got[:, 2:]).all()  # a NaN coordinate is looked up at 0: Le stays finite


def test_le_is_one_rounded_product_and_an_unbound_light_is_plain():
    scene, tex, bind, lid, u = emission_cases.case()
    got = host.light_emission(scene, tex, bind, lid, u)
    mat = scene["mat"].reshape(-1, 18)
    mid = scene["light"].reshape(-1, 4)[lid, 3].astype(np.int64)
    bound = bind[mid] >= 0
    assert bound.any() and (~bound).any()
    _same(got[~bound, 2:], mat[mid[~bound], 3:6], "an unbound light")
    c = host.texture_lookup(tex, bind[mid[bound]], got[bound, :2])
    _same(got[bound, 2:], (mat[mid[bound], 3:6] * c).astype(F), "Le = emission * lookup(s, t)")
    one = bind[mid] == 6  # the 1 x 1 texture: one texel whatever the coordinates
    assert one.any()
    texel = np.asarray(tex[6][0], F)[0, 0, :3]
    _same(got[one, 2:], (mat[mid[one], 3:6] * texel).astype(F), "the 1 x 1 texture")


def test_the_degenerate_light_and_the_flip_boundary():
    scene, tex, bind, lid, u = emission_cases.case()
    st = host.light_st(scene)
    _same(st.reshape(-1, 6), emission_math.light_st(scene).reshape(-1, 6), "glrt_light_st")
    point = int(np.flatnonzero((st == st[:, :1]).all((1, 2)))[0])  # the light whose three coordinate pairs are one
    sel = lid == point
    got = host.light_emission(scene, tex, bind, lid[sel], u[sel])
    # w0 s + ua s + ub s is s only up to rounding: the statement is the arithmetic, and it stays within a few ulps of the corner
    assert np.abs(got[:, :2] - st[point, 0]).max() <= 4 * np.spacing(np.abs(st[point, 0]).max())
    above = F(0.75) + F(2.0 ** -23)  # 0.25 + above = 1 + 2^-23 exactly: the smallest sum that flips
    on = host.light_emission(scene, tex, bind, [3, 3], [[0.25, 0.75], [0.25, above]])
    s3 = st[3]
    _same(on[0, :2], emission_math.sample_st(s3[None], [[0.25, 0.75]])[0], "ua0 + ub0 == 1 does not flip")
    w0 = F(F(1) - F(0.25)) - F(0.75)
    assert w0 == 0 and np.array_equal(on[0, :2], (F(0.25) * s3[1] + F(0.75) * s3[2]).astype(F))
    flipped = emission_math.sample_st(s3[None], [[F(1) - F(0.25), F(1) - above]])[0]  # the flipped pair (1 - ua0, 1 - ub0), itself below the boundary
    assert F(0.25) + above > 1
    _same(on[1, :2], flipped, "one float above the boundary flips")


def test_emission_albedo_is_the_albedo_rule_plus_the_texel_at_a_bound_emitter():
    scene, params, wall = scenes.config_emissive_wall(n=4, uv="corner")
    rng = np.random.default_rng(5)
    tex = [(rng.uniform(0, 1, (3, 5, 4)).astype(F), "rgba32f", "clamp", "bilinear"), (rng.integers(0, 256, (4, 4, 4), dtype=np.uint8), "rgba8_srgb", "repeat", "bilinear")]
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    alb = np.full(n_mat, -1, np.int32); alb[0] = 1  # the grey floor: an albedo texture
    emi = np.full(n_mat, -1, np.int32); emi[wall["material"]] = 0; emi[0] = 0  # ... and an emission map on it as well, which plane A does not show
    _, _, g = host.render_features_geom(scene, params)
    got = host.emission_albedo(scene, tex, alb, emi, g)
    base = host.texture_albedo(scene, tex, alb, g)
    tri = g[..., 0].view(np.int32)
    on_wall = np.isin(tri, np.asarray(list(wall["tri"])))
    assert on_wall.sum() > 300
    _same(got[~on_wall], base[~on_wall], "off the panel: glrt_texture_albedo")
    st, ok, _ = texture_math.hit_st(scene["vert"], scene["tri"], g.reshape(-1, 4))
    ref = texture_math.lookup(tex, np.zeros(int(on_wall.sum()), np.int64), st[on_wall.reshape(-1)])
    _same(got[on_wall], ref, "on the panel: the texel, without the emission")
    assert len(np.unique(_bits(got[on_wall]), axis=0)) > 100  # ... which varies inside the triangles
    none = host.emission_albedo(scene, tex, alb, np.full(n_mat, -1, np.int32), g)
    _same(none.reshape(-1, 3), base.reshape(-1, 3), "nothing bound")


def test_the_validator_refuses_what_the_header_lists():
    scene, _, wall = scenes.config_emissive_wall(n=4)
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    w = wall["material"]
    good = np.full(n_mat, -1, np.int32); good[w] = 0
    assert host.emission_bind_check(scene, 2, good) == ""
    every = np.zeros(n_mat, np.int32)  # diffuse, conductor, emitter: any type but media
    assert host.emission_bind_check(scene, 1, every) == ""
    assert host.emission_bind_check(scene, 0, good) == "no texture set is bound (call glrtx_upload_textures first)"
    assert host.emission_bind_check(scene, 2, good[:-1]) == f"{n_mat - 1} bindings, the scene has {n_mat} materials"
    bad = good.copy(); bad[w] = 2
    assert host.emission_bind_check(scene, 2, bad) == f"material {w}: emission map 2 of 2 textures"
    bad[w] = -2
    assert host.emission_bind_check(scene, 2, bad) == f"material {w}: emission map -2 of 2 textures"
    assert "cutouts are bound" in host.emission_bind_check(scene, 2, good, cutouts_bound=True)
    b = scenes.SceneBuilder()
    b.add_mesh(*scenes.quad((-1, 0, 1), (2, 0, 0), (0, 0, -2)), b.add_material(scenes.emitter((1.0, 1.0, 1.0))))
    b.add_mesh(*scenes.box((-1, 0, -1), (1, 2, 1)), b.add_material(scenes.media()))
    fog = b.build()
    assert host.emission_bind_check(fog, 1, [0, -1]) == ""
    assert host.emission_bind_check(fog, 1, [0, 0]) == "material 1 has an emission map and is a medium (type 5)"
    with pytest.raises(RuntimeError):
        host.light_emission(fog, [(np.zeros((1, 1, 4), F), "rgba32f", "repeat", "nearest")], [0, 0], [0], [[0.1, 0.1]])  # GLRT_HOST_EINDEX: a bound medium
    with pytest.raises(RuntimeError):
        host.light_emission(fog, [(np.zeros((1, 1, 4), F), "rgba32f", "repeat", "nearest")], [0, -1], [2], [[0.1, 0.1]])  # a light out of range


# ---- sanitizers: the statements in a stand-alone program of their own
def test_statements_run_clean_under_sanitizers(tmp_path):
    import pathlib
    import shutil
    import subprocess
    from conftest import PKG, ROOT
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "the host library's compiler is needed"
    host_dir = PKG / "host"
    exe = tmp_path / "emission_sanitize"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT / 'include'}",
           f"-I{host_dir}", "-o", str(exe), str(pathlib.Path(__file__).with_name("emission_sanitize.cpp")), str(host_dir / "texture.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "emission_sanitize ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
