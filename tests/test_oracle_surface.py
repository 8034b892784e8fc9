"""The oracle's surface hooks (oracle/pt_oracle.c: pt_oracle_set_surface; include/glrt_host.h "Surface context"), anchored without a GPU to the equivalences the
suite already trusts.  The hooks add no shading statement: a material constant is replaced by the host library's lookup at the hit.  So, bit for bit and ray
for ray: the albedo hook under a texture constant over each cell is the per-cell scene; the accept hook under the checkerboard is the collapsed scene, under a
cutoff nothing reaches the wall-less scene, under one everything reaches the plain scene; the emission hook under per-cell texels is the per-cell emitters;
hooks that are NULL or bind nothing are the plain oracle.  The per-hit calls equal the batch statements they are built on, and run clean under sanitizers
in a stand-alone program of their own."""
import ctypes as C
import pathlib
import re
import shutil
import subprocess

import numpy as np
import pytest

import emission_cases
import surface_cases as sc
import texture_cases
import texture_math as tm
from conftest import PKG, ROOT
from glrt_amd import host, scenes

F = np.float32
N = sc.N


def _both(got, ref, what):
    sc.same(got[0], ref[0], what)
    assert got[1] == ref[1], f"{what}: {got[1]} rays, {ref[1]} in the reference"


# ---- albedo: a texture constant over each cell is one diffuse material a cell
@pytest.mark.parametrize("form", ["float-nearest", "srgb", "bilinear-blocks"])
def test_albedo_hook_under_a_per_cell_texture_is_the_per_cell_scene(form):
    albedo = code = None
    if form == "srgb":
        code = np.random.default_rng(21).integers(40, 250, (N, N, 3), dtype=np.uint8)
        albedo = tm.SRGB[code.astype(np.int64)]
    scene, params, wall = scenes.config_textured_wall(n=N, albedo=albedo)
    cells, _, _ = scenes.config_textured_wall(n=N, albedo=albedo, per_cell=True)
    assert (params["width"], params["height"], params["max_depth"]) == (64, 48, 4) and np.array_equal(scene["bvh"], cells["bvh"])
    if form == "float-nearest":
        tex = (wall["albedo"], "rgba32f", "repeat", "nearest")
    elif form == "srgb":
        tex = (code, "rgba8_srgb", "repeat", "nearest")
    else:  # 2 x 2 equal texels a cell, looked up at the block's centre
        tex = (np.repeat(np.repeat(wall["albedo"], 2, 0), 2, 1), "rgba32f", "repeat", "bilinear")
    ref = sc.oracle(cells, params)
    plain = sc.oracle(scene, params)
    assert sc.share(ref[0], plain[0]) >= 1.0 / 3.0  # precondition: the albedo is seen
    _both(sc.hooked(scene, params, scene, [tex], material_texture=sc.at(scene, wall["material"])), ref, form)


# ---- cutouts: a rejected candidate is a triangle that is not there
def test_accept_hook_under_the_checkerboard_is_the_collapsed_scene():
    scene, params, wall = scenes.config_cutout_wall(n=N)
    j, i = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    cells = (i + j) % 2 == 0
    rgba = np.zeros((N, N, 4), F)
    rgba[..., 3] = np.where(cells, 0.0, 1.0)
    tex = [(rgba, "rgba32f", "repeat", "nearest")]
    n_mat = sc.none(scene).size
    cut = lambda cutoff: host.cutouts(n_mat, texture=sc.at(scene, wall["material"]), channel=3, cutoff=cutoff)
    collapsed = sc.oracle(wall["collapsed"](wall["cell_tris"](cells)), params)
    plain = sc.oracle(scene, params)
    gone = sc.oracle(wall["collapsed"](list(wall["tri"])), params)
    # preconditions: the three images are three images
    assert min(sc.share(collapsed[0], plain[0]), sc.share(collapsed[0], gone[0]), sc.share(plain[0], gone[0])) >= 0.2
    assert len({collapsed[1], plain[1], gone[1]}) == 3
    _both(sc.hooked(scene, params, scene, tex, cut=cut(0.5)), collapsed, "the checkerboard")
    _both(sc.hooked(scene, params, scene, tex, cut=cut(2.0)), gone, "a cutoff of 2: the wall-less scene")
    _both(sc.hooked(scene, params, scene, tex, cut=cut(-1.0)), plain, "a cutoff below every texel: the plain scene")


# ---- emission: a map constant over each cell is one emitter material a cell
@pytest.mark.parametrize("n", [4, 6])
def test_emission_hook_under_per_cell_texels_is_the_per_cell_emitters(n):
    texel = np.random.default_rng(3).uniform(0.1, 0.9, (n, n, 3)).astype(F)
    scene, params, wall = scenes.config_emissive_wall(n=n, texel=texel)
    cells, _, _ = scenes.config_emissive_wall(n=n, texel=texel, per_cell=True)
    assert np.array_equal(scene["bvh"], cells["bvh"]) and np.array_equal(scene["light"][:, :3], cells["light"][:, :3])
    ref = sc.oracle(cells, params)
    plain = sc.oracle(scene, params)
    assert sc.share(ref[0], plain[0]) >= 0.5  # precondition: the map is seen
    _both(sc.hooked(scene, params, scene, [(texel, "rgba32f", "repeat", "nearest")], material_emission=sc.at(scene, wall["material"])), ref, f"n = {n}")


# ---- hooks that are NULL or bind nothing
def test_null_hooks_and_empty_bindings_are_the_plain_oracle():
    scene, params, wall = scenes.config_textured_wall(n=N, uv=sc.free_uv(5))
    plain = sc.oracle(scene, params)
    tex = [sc.random_texture(5, 4, "rgba32f", "repeat", "bilinear", 1)]
    n_mat = sc.none(scene).size
    with host.Surface(scene, tex, sc.at(scene, wall["material"])) as s:
        user = s.hooks()[0]
        _both(sc.oracle(scene, params, surface=(user, None, None, None)), plain, "three NULL hooks")
        _both(sc.oracle(scene, params, surface=(None, None, None, None)), plain, "a NULL record")
        assert sc.share(sc.oracle(scene, params, surface=s.hooks())[0], plain[0]) >= 1.0 / 3.0  # the same context, hooked: another image
        _both(sc.oracle(scene, params), plain, "the hooks are cleared after a render")
    _both(sc.hooked(scene, params, scene, tex, sc.none(scene), host.cutouts(n_mat), sc.none(scene)), plain, "three hooks that bind nothing")
    _both(sc.hooked(scene, params, scene, [], None, None, None), plain, "an empty set")


# ---- the per-hit calls against the batch statements
def _flat_scene(textures, seed):
    """One diffuse material and three triangles a texture, free corner coordinates; (scene, hits (n, 4): wire triangle bits, u, v, 0)"""
    rng = np.random.default_rng(seed)
    b = scenes.SceneBuilder()
    for k in range(len(textures)):
        pos, nrm, _ = scenes.random_triangles(3, 100 + k, 3.0, 0.5)
        b.add_mesh(pos, nrm, b.add_material(scenes.diffuse((0.5, 0.5, 0.5))), uv=rng.uniform(-1.0, 2.0, (3, 3, 2)).astype(F))
    scene = b.build("sah")
    n_tri = scene["tri"].reshape(-1, 4).shape[0]
    tri = np.tile(np.arange(n_tri, dtype=np.int32), 24)
    u = rng.uniform(0.0, 1.0, tri.size).astype(F)
    v = (rng.uniform(0.0, 1.0, tri.size).astype(F) * (F(1) - u)).astype(F)
    u[:n_tri], v[:n_tri] = 0.0, 0.0  # the corners and an edge
    u[n_tri:2 * n_tri], v[n_tri:2 * n_tri] = 1.0, 0.0
    u[2 * n_tri:3 * n_tri], v[2 * n_tri:3 * n_tri] = 0.0, 1.0
    v[3 * n_tri:4 * n_tri] = 0.0
    hits = np.zeros((tri.size, 4), F)
    hits[:, 0] = tri.view(F); hits[:, 1] = u; hits[:, 2] = v
    return scene, tri, u, v, hits


def _equal_or_both_nan(a, b):
    return (sc.bits(a) == sc.bits(b)) | (np.isnan(a) & np.isnan(b))


def test_per_hit_albedo_and_accept_equal_the_batch_statements():
    textures = texture_cases.textures()[:96]  # every format, filter and wrap pair at 1 x 1, 1 x 7, 2 x 3 and 5 x 4 texels
    scene, tri, u, v, hits = _flat_scene(textures, 41)
    n_mat = len(textures)
    mat_of = scene["tri"].reshape(-1, 4)[:, 3].astype(np.int64)
    bind = np.arange(n_mat, dtype=np.int32)
    bind[::7] = -1  # some materials unbound
    channel = (np.arange(n_mat) % 4).astype(np.int32)
    cutoff = np.random.default_rng(5).uniform(0.2, 0.8, n_mat).astype(F)
    cut = host.cutouts(n_mat, texture=bind, channel=channel, cutoff=cutoff)
    want_rgb = host.texture_albedo(scene, textures, bind, hits)
    # the coordinates, mixed as the statements mix them (the operands are far from the denormals: numpy's fp32 operations are the statements')
    vert, wire = scene["vert"].reshape(-1, 5, 3), scene["tri"].reshape(-1, 4)
    a, b, c = (vert[wire[tri, k].astype(np.int64), 2, :2] for k in range(3))
    w0 = (F(1) - u) - v
    st = ((w0[:, None] * a + u[:, None] * b) + v[:, None] * c).astype(F)
    m = mat_of[tri]
    bound = bind[m] >= 0
    value = np.zeros(tri.size, F)
    value[bound] = host.texture_channel(textures, bind[m][bound], channel[m][bound], st[bound])
    want_accept = ~bound | (value >= cutoff[m])
    assert 0.2 < want_accept[bound].mean() < 0.8
    with host.Surface(scene, textures, bind, cut) as s:
        for i in range(tri.size):
            got_bound, rgb = s.albedo(tri[i], u[i], v[i])
            assert got_bound == bool(bound[i])
            if got_bound:
                assert _equal_or_both_nan(rgb, want_rgb[i]).all(), (i, rgb, want_rgb[i])
            assert s.accept(tri[i], u[i], v[i]) == bool(want_accept[i]), (i, value[i], cutoff[m[i]])
        n_tri = wire.shape[0]
        for bad in (-1, n_tri, 2 ** 31 - 1, -2 ** 31):  # outside the scene: unbound
            assert s.albedo(bad, 0.25, 0.25)[0] is False and s.accept(bad, 0.25, 0.25) is True and s.emission(bad, 0, 0.25, 0.25)[0] is False


def test_per_hit_emission_equals_the_batch_statement():
    scene, textures, bind, lid, u = emission_cases.case()
    step = 7  # every seventh sample, and every sample of the flip's boundary (the last 8 a light)
    n_light = scene["light"].reshape(-1, 4).shape[0]
    keep = np.concatenate([np.arange(0, 40 * n_light, step), np.arange(40 * n_light, lid.size)])
    lid, u = lid[keep], u[keep]
    want = host.light_emission(scene, textures, bind, lid, u)
    flip = F(1) < u[:, 0] + u[:, 1]  # sampleDirect's flip, taken by the caller of the per-hit call
    ua = np.where(flip, F(1) - u[:, 0], u[:, 0]).astype(F)
    ub = np.where(flip, F(1) - u[:, 1], u[:, 1]).astype(F)
    mat = scene["mat"].reshape(-1, 18)
    light_mat = scene["light"].reshape(-1, 4)[:, 3].astype(np.int64)
    seen = 0
    with host.Surface(scene, textures, material_emission=bind) as s:
        for i in range(lid.size):
            m = light_mat[lid[i]]
            bound, c = s.emission(lid[i], 1, ua[i], ub[i])
            assert bound == bool(bind[m] >= 0)
            le = (mat[m, 3:6] * c).astype(F) if bound else mat[m, 3:6]  # Le = emission * c: one rounded product a channel
            assert _equal_or_both_nan(le, want[i, 2:]).all(), (i, int(lid[i]), u[i].tolist(), le, want[i])
            seen += bound
        # the seen side: a light's triangle at the same barycentrics reads the same texel (the wall's lights are its triangles)
        wire = scene["tri"].reshape(-1, 4)
        light = scene["light"].reshape(-1, 4)
        for l in range(0, n_light, 3):
            t = int(np.flatnonzero((wire[:, :3] == light[l, :3]).all(1))[0])
            assert np.array_equal(sc.bits(s.emission(t, 0, 0.3, 0.45)[1]), sc.bits(s.emission(l, 1, 0.3, 0.45)[1]))
    assert seen > 500


def test_create_refuses_what_the_binds_refuse():
    scene, params, wall = scenes.config_cutout_wall(n=N)
    tex = [sc.random_texture(5, 4, "rgba32f", "repeat", "nearest", 2)]
    t = scene["mat"].reshape(-1, 18)[:, 0].astype(np.int32)
    lamp, cu = int(np.flatnonzero(t == 1)[0]), int(np.flatnonzero(t == 3)[0])
    n_mat = t.size
    for kw in (dict(material_texture=sc.at(scene, wall["material"], 1)), dict(material_texture=sc.at(scene, cu, 0)), dict(material_emission=sc.at(scene, lamp, 1)),
               dict(cut=host.cutouts(n_mat, texture=sc.at(scene, lamp, 0))), dict(cut=host.cutouts(n_mat, texture=sc.at(scene, cu, 0), channel=4)),
               dict(cut=host.cutouts(n_mat, texture=sc.at(scene, cu, 0), cutoff=np.nan))):
        with pytest.raises(RuntimeError, match="glrt_surface_create failed"):
            host.Surface(scene, tex, **kw)
    host.Surface(scene, tex, sc.at(scene, wall["material"]), host.cutouts(n_mat, texture=sc.at(scene, cu, 0)), sc.at(scene, lamp, 0)).close()


# ---- ABI
def test_header_library_and_bindings_carry_the_calls():
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in ("glrt_surface_create", "glrt_surface_free", "glrt_surface_albedo", "glrt_surface_accept", "glrt_surface_emission"):
        assert re.search(rf"\b(int|void) {name}\(", host_h), name
        assert hasattr(H, name), name
    assert "int glrt_surface_albedo(void *surface, int tri, float u, float v, float rgb[3]);" in host_h
    assert "int glrt_surface_accept(void *surface, int tri, float u, float v);" in host_h
    from oracle import pt_oracle
    assert hasattr(pt_oracle.lib(), "pt_oracle_set_surface") and C.sizeof(pt_oracle._Surface) == 4 * C.sizeof(C.c_void_p)


# ---- the library is this source's, whatever the time stamps say
def test_a_library_built_from_another_source_is_not_taken_for_this_one(tmp_path, monkeypatch):
    """oracle/_ref/ is outside git and can outlive a checkout: a newer library built from another commit's pt_oracle.c must be rebuilt, not loaded"""
    from oracle import pt_oracle
    pt_oracle.lib()
    real = pt_oracle._LIB.read_bytes()
    own = b"pt_oracle_src_id=" + pt_oracle._src_id().encode() + b"\0"
    assert pt_oracle._fresh() and own in real
    other = tmp_path / "libpt_oracle.so"
    monkeypatch.setattr(pt_oracle, "_LIB", other)
    assert not pt_oracle._fresh()  # missing
    other.write_bytes(real.replace(own, b"pt_oracle_src_id=" + b"0" * 16 + b"\0"))
    assert not pt_oracle._fresh()  # another source's id
    other.write_bytes(real.replace(own, b""))
    assert not pt_oracle._fresh()  # no id at all: a library from before the id existed
    other.write_bytes(real.replace(own, b"pt_oracle_src_id=unstamped\0"))
    assert pt_oracle._fresh()      # compiled by hand
    other.write_bytes(real)
    assert pt_oracle._fresh()
    makefile = (ROOT / "oracle" / "Makefile").read_text()
    assert 'grep -qa "pt_oracle_src_id=$(SRC_ID)"' in makefile and "-DPT_SRC_ID=" in makefile  # make itself rebuilds by content


# ---- sanitizers: the per-hit calls in a stand-alone program of their own
def test_per_hit_calls_run_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "the host library's compiler is needed"
    host_dir = PKG / "host"
    exe = tmp_path / "surface_sanitize"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT / 'include'}",
           f"-I{host_dir}", "-o", str(exe), str(pathlib.Path(__file__).with_name("surface_sanitize.cpp")), str(host_dir / "texture.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "surface_sanitize ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
