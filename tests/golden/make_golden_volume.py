#!/usr/bin/env python3
"""Volume fixtures for tests/golden/: the reference's fragment shader with its volume branch switched on, on Mesa llvmpipe.

Run where the reference checkout (oracle/glref.py: GLRT_REFERENCE) and Mesa's swrast_dri.so exist:

    make -C oracle && make -C opengl-raytracer_amd host && python tests/golden/make_golden_volume.py

The reference compiles the branch out (`#define ENABLE_VOLUME 0`, raytrace.frag:4).  Its shader text is read at run time by
oracle/glref.py's conventions and edited IN MEMORY only -- nothing of it is written here, a fixture is data:
  * class "switch": the define set to 1, nothing else.  Used with CONSTANT grids only, where the nearest and the linear filter
    return the stored value exactly (a lerp of equal values is that value), so the filter GL picks from the implicit derivatives
    of the 2x2 pixel quad cannot matter;
  * class "lod": the define set to 1 and densityLookup / temperatureLookup reading textureLod(tex, uvw, 0.0) instead of
    texture(tex, uvw) -- the magnification filter (trilinear, GL_REPEAT) everywhere.  This is the one edit of the pinned contract
    ("Volumes").
The grids are uploaded the way the reference does (scene.cpp:183-188: glTexStorage3D with one level, GL_R32F, glTexSubImage3D with
GL_RED, no sampler state) and bound the way Window::render does (window.cpp:271-286: units 7 and 8, u_hasVolume, u_bboxMin,
u_bboxMax, u_densityMax).  oracle/glref has no 3D-texture entry points; they are taken from libglapi in the same process, after
glref has made its context current.

Fixtures go to tests/golden/volume/.  Also writes math_volume.npz: llvmpipe's own exp / log / acos on a dense sweep, blackBody (the reference's two functions, taken
from its shader text at run time) on a temperature sweep, and a textureLod(..., 0.0) lookup sweep of a probe shader of this file.
"""
from __future__ import annotations

import ctypes as C
import pathlib
import re
import sys

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "opengl-raytracer_amd" / "python"))

from glrt_amd import host, scenes  # noqa: E402
from glrt_amd.scenes import SceneBuilder, camera, conductor, diffuse, emitter, make_params, media, quad  # noqa: E402
from oracle.glref import REFERENCE_SHADERS, GLRef  # noqa: E402

OUT = pathlib.Path(__file__).resolve().parent / "volume"  # (a directory of its own: tests/conftest.py:golden_names() takes every *.npz of tests/golden as a shader-only fixture)
g = GLRef()
OUT.mkdir(exist_ok=True)

GL_TEXTURE_3D, GL_R32F, GL_RED, GL_FLOAT, GL_TEXTURE0 = 0x806F, 0x822E, 0x1903, 0x1406, 0x84C0
_api = C.CDLL("libglapi.so.0", mode=C.RTLD_GLOBAL)
_getproc = _api._glapi_get_proc_address
_getproc.restype, _getproc.argtypes = C.c_void_p, [C.c_char_p]


def _gl(name, *args):
    return C.CFUNCTYPE(None, *args)(_getproc(name.encode()))


glGenTextures = _gl("glGenTextures", C.c_int, C.POINTER(C.c_uint))
glDeleteTextures = _gl("glDeleteTextures", C.c_int, C.POINTER(C.c_uint))
glBindTexture = _gl("glBindTexture", C.c_uint, C.c_uint)
glActiveTexture = _gl("glActiveTexture", C.c_uint)
glTexStorage3D = _gl("glTexStorage3D", C.c_uint, C.c_int, C.c_uint, C.c_int, C.c_int, C.c_int)
glTexSubImage3D = _gl("glTexSubImage3D", C.c_uint, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_uint, C.c_void_p)


def tex3d(unit, grid):
    """GL_R32F 3D texture of grid (nz, ny, nx), x fastest, bound on `unit` (the reference's upload: one immutable level, default sampler state)."""
    a = np.ascontiguousarray(grid, np.float32)
    nz, ny, nx = a.shape
    t = C.c_uint(0)
    glGenTextures(1, C.byref(t))
    glActiveTexture(GL_TEXTURE0 + unit)
    glBindTexture(GL_TEXTURE_3D, t.value)
    glTexStorage3D(GL_TEXTURE_3D, 1, GL_R32F, nx, ny, nz)
    glTexSubImage3D(GL_TEXTURE_3D, 0, 0, 0, 0, nx, ny, nz, GL_RED, GL_FLOAT, a.ctypes.data)
    glActiveTexture(GL_TEXTURE0)
    return t


def shader(cls):
    fs = (REFERENCE_SHADERS / "raytrace.frag").read_text()
    fs, n = re.subn(r"#define ENABLE_VOLUME 0", "#define ENABLE_VOLUME 1", fs)
    assert n == 1, "the reference's volume switch was not found"
    if cls == "lod":
        for tex in ("u_densityTex", "u_temperatureTex"):
            fs, n = re.subn(rf"texture\({tex}, vec3\(uvw\)\)", f"textureLod({tex}, vec3(uvw), 0.0)", fs)
            assert n == 1, f"the lookup of {tex} was not found"
    return fs


def render_volume(scene, params, vol, cls, frames=None):
    """oracle.glref.GLRef.render_reference with the edited shader and the volume bound (window.cpp:213-295)."""
    L = g.L
    vs = (REFERENCE_SHADERS / "raytrace.vert").read_text()
    p = g.program(vs, shader(cls))
    L.glref_use(p)
    w, h = int(params["width"]), int(params["height"])
    handles = []
    for name, arr, comps, unit in [("u_vertBuffer", scene["vert"], 3, 2), ("u_triBuffer", scene["tri"], 4, 3), ("u_matBuffer", scene["mat"], 3, 4),
                                   ("u_lightBuffer", scene["light"], 4, 5), ("u_bvhBuffer", scene["bvh"], 3, 6)]:
        hdl = g.tbo(arr, comps)
        handles.append(hdl)
        L.glref_bind_tbo(unit, hdl[0])
        L.glref_uniform1i(p, name.encode(), unit)
    texs = [tex3d(7, vol["density"]), tex3d(8, vol["temperature"])]
    g._set_uniforms(p, {
        "u_c2wMat": params["c2w"], "u_s2cMat": params["s2c"], "u_apertureRadius": float(params.get("aperture", 0.0)),
        "u_focalLength": float(params.get("focal", 1.0)), "u_nSamples": int(params["n_samples"]), "u_maxDepth": int(params["max_depth"]),
        "u_windowSize": (float(w), float(h)), "u_nTris": int(scene["tri"].shape[0]), "u_nLights": int(np.asarray(scene["light"]).reshape(-1, 4).shape[0]),
        "u_hasVolume": 1, "u_bboxMin": vol["bbox_min"], "u_bboxMax": vol["bbox_max"], "u_densityMax": float(vol["density_max"]),
        "u_densityTex": 7, "u_temperatureTex": 8})
    z3, z1 = np.zeros((h, w, 3), np.float32), np.zeros((h, w), np.float32)
    tex = [[L.glref_tex2d(w, h, 3, z3.ctypes.data), L.glref_tex2d(w, h, 1, z1.ctypes.data)] for _ in range(2)]
    fbo = [L.glref_fbo(2, (C.c_uint * 2)(*tex[i])) for i in range(2)]
    if not all(fbo):
        raise RuntimeError(g.err())
    sel = 0
    for sd in ([params["seed"]] if frames is None else list(frames)):
        sel ^= 1
        L.glref_uniform2f(p, b"u_seed", float(sd[0]), float(sd[1]))
        L.glref_bind_tex2d(0, tex[sel ^ 1][0])
        L.glref_uniform1i(p, b"u_framebuffer", 0)
        L.glref_bind_tex2d(1, tex[sel ^ 1][1])
        L.glref_uniform1i(p, b"u_counter", 1)
        if L.glref_draw(fbo[sel], w, h, 1) != 0:
            raise RuntimeError(g.err())
    rgb, cnt = np.empty((h, w, 3), np.float32), np.empty((h, w), np.float32)
    L.glref_read_tex2d(tex[sel][0], 3, rgb.ctypes.data)
    L.glref_read_tex2d(tex[sel][1], 1, cnt.ctypes.data)
    for f in fbo:
        L.glref_fbo_free(f)
    for pair in tex:
        for t in pair:
            L.glref_tex_free(t)
    for hdl in handles:
        L.glref_tbo_free(hdl[0], hdl[1])
    for t in texs:
        glDeleteTextures(1, C.byref(t))
    return rgb, cnt


def save(name, scene, params, vol, cls, frames=None):
    vol = dict(vol)
    vol.setdefault("density_max", float(np.max(vol["density"])))
    rgb, cnt = render_volume(scene, params, vol, cls, frames)
    np.savez_compressed(
        OUT / f"{name}.npz",
        vert=scene["vert"], tri=scene["tri"], mat=scene["mat"], light=scene["light"], bvh=scene["bvh"],
        c2w=params["c2w"], s2c=params["s2c"],
        scalars=np.array([params["width"], params["height"], params["max_depth"], params["n_samples"]], np.int32),
        fparams=np.array([params["seed"][0], params["seed"][1], params["aperture"], params["focal"]], np.float32),
        rows=np.array((0, params["height"]), np.int32),
        frames=np.array(frames if frames is not None else np.zeros((0, 2)), np.float32).reshape(-1, 2),
        density=np.asarray(vol["density"], np.float32), temperature=np.asarray(vol["temperature"], np.float32),
        bbox=np.array([*vol["bbox_min"], *vol["bbox_max"]], np.float32), density_max=np.float32(vol["density_max"]),
        shader_class=np.array(cls), out_rgb=rgb, out_count=cnt, renderer=np.array(g.info()))
    magenta = int(np.count_nonzero((rgb[..., 0] > 0) & (rgb[..., 1] == 0) & (rgb[..., 2] > 0)))
    print(f"{name} [{cls}]: {rgb.shape} mean {rgb.mean(axis=(0, 1))} max {rgb.max():.3f} nan {int(np.isnan(rgb).sum())} "
          f"pixels at the clamp {int((rgb >= 100.0 * params['n_samples']).any(-1).sum())} magenta-ish {magenta}")


def fire_scene(w, h, depth, spp, lo=(-1.0, 0.05, -1.0), hi=(1.0, 2.05, 1.0), open_box=False, seed=(0.31, 0.67), floor=None, eye=(0.4, 2.4, 5.5)):
    """A media box over a floor (diffuse unless given), a lamp above (open_box: its back and top faces left out, so that trial rays leave the scene)."""
    b = SceneBuilder()
    fog = b.add_material(media())
    grey = b.add_material(floor or diffuse((0.7, 0.7, 0.7)))
    lamp = b.add_material(emitter((6.0, 6.0, 6.0)))
    pos, nrm = scenes.box(lo, hi)
    if open_box:  # faces in box() order: -z, +z, -y, +y, -x, +x (two triangles each)
        keep = np.r_[2:6, 8:12]
        pos, nrm = pos[keep], nrm[keep]
    b.add_mesh(pos, nrm, fog)
    b.add_mesh(*quad((-6, 0, 6), (12, 0, 0), (0, 0, -12)), grey)
    b.add_mesh(*quad((-1, 4, -1), (2, 0, 0), (0, 0, 2)), lamp)
    sc = b.build()
    c2w, s2c = camera(eye, (0, 1, 0), (0, 1, 0), 42.0, w, h)
    return sc, make_params(c2w, s2c, w, h, depth, spp, seed=seed), dict(bbox_min=lo, bbox_max=hi)


def const_vol(v, dens, temp, n=(4, 4, 4)):
    nx, ny, nz = n
    return dict(v, density=np.full((nz, ny, nx), dens, np.float32), temperature=np.full((nz, ny, nx), temp, np.float32))


def main():
    # constant grids, both classes (nearest == linear on them, so "switch" is the reference shader with only its define flipped)
    sc, pr, v = fire_scene(64, 48, 8, 4)
    save("vol_const_switch", sc, pr, const_vol(v, 0.5, 7.0), "switch")
    save("vol_const_lod", sc, pr, const_vol(v, 0.5, 7.0), "lod")
    # a smooth fire blob at 16^3
    d, t = scenes.fire_grids((16, 16, 16), 10.0)
    save("vol_fire16", sc, pr, dict(v, density=d, temperature=t), "lod")
    # noise on a non-cubic 12 x 7 x 5 grid in a non-cubic box: pins the axis order; density_max above the grid's maximum
    rng = np.random.default_rng(20261015)
    sc2, pr2, v2 = fire_scene(64, 48, 8, 3, lo=(-1.3, 0.05, -0.7), hi=(1.1, 1.6, 0.9), seed=(0.53, 0.12))
    noise = dict(v2, density=rng.random((5, 7, 12), dtype=np.float32), temperature=(6.0 + 2.0 * rng.random((5, 7, 12))).astype(np.float32),
                 density_max=1.25)
    save("vol_noise_12x7x5", sc2, pr2, noise, "lod")
    # cold: exp() overflows and blackBody gives 0 (T = 5 K); hot: radiance's final min(L, 1.0e2) is reached (T = 9000 K)
    save("vol_cold", sc, pr, dict(v, density=d, temperature=np.full_like(t, 0.05)), "lod")
    save("vol_hot", sc, with_seed(pr, (0.77, 0.21)), dict(v, density=d, temperature=(90.0 * d / d.max()).astype(np.float32)), "lod")
    # an open media mesh: trial rays that leave it hit nothing and radiance() returns magenta
    sc3, pr3, v3 = fire_scene(64, 48, 8, 2, open_box=True, seed=(0.41, 0.93))
    save("vol_open", sc3, pr3, dict(v3, density=(0.3 * d).astype(np.float32), temperature=t), "lod")
    # the medium seen in a polished copper floor: entered at depth > 0
    sc4, pr4, v4 = fire_scene(64, 48, 8, 3, floor=conductor(scenes.COPPER["eta"], scenes.COPPER["kappa"], 0.05), eye=(0.4, 0.9, 5.5), seed=(0.19, 0.44))
    save("vol_through_conductor", sc4, pr4, dict(v4, density=d, temperature=t), "lod")
    # several frames through the accumulation loop (a power-of-two image: the previous frame is read back through a LINEAR sampler)
    sc5, pr5, v5 = fire_scene(64, 32, 8, 2)
    save("vol_frames3", sc5, pr5, dict(v5, density=d, temperature=t), "lod", frames=[host.frame_seed(f) for f in range(3)])
    math_sweeps()


def with_seed(params, seed):
    p = dict(params)
    p["seed"] = (float(np.float32(seed[0])), float(np.float32(seed[1])))
    return p


MATH_FS = """#version 410
uniform samplerBuffer u_in;
uniform int u_width;
layout(location = 0) out vec4 o;
void main() {
    float x = texelFetch(u_in, int(gl_FragCoord.y) * u_width + int(gl_FragCoord.x)).x;
    o = vec4(exp(x), log(x), acos(x), 0.0);
}
"""
LOOKUP_FS = """#version 410
uniform samplerBuffer u_in;
uniform int u_width;
uniform sampler3D u_tex;
uniform vec3 u_bboxMin;
uniform vec3 u_bboxMax;
layout(location = 0) out vec4 o;
void main() {
    vec3 pos = texelFetch(u_in, int(gl_FragCoord.y) * u_width + int(gl_FragCoord.x)).xyz;
    vec3 uvw = (pos - u_bboxMin) / (u_bboxMax - u_bboxMin);
    o = vec4(textureLod(u_tex, uvw, 0.0).x, 0.0, 0.0, 0.0);
}
"""


def blackbody_fs():
    """A probe around the reference's own blackBody functions (raytrace.frag:125-142), cut from its text at run time."""
    fs = (REFERENCE_SHADERS / "raytrace.frag").read_text()
    m = re.search(r"Float blackBody\(Float l, Float T\) \{.*?\n\}\n\s*Vec3 blackBody\(Float T\) \{.*?\n\}\n", fs, re.S)
    assert m, "blackBody not found in the reference shader"
    return ("#version 410\n#define Float float\n#define Vec3 vec3\nuniform samplerBuffer u_in;\nuniform int u_width;\n"
            "layout(location = 0) out vec4 o;\n" + m.group(0) +
            "void main() {\n    float v = texelFetch(u_in, int(gl_FragCoord.y) * u_width + int(gl_FragCoord.x)).x;\n"
            "    o = vec4(blackBody(v * 1.0e2), 0.0);\n}\n")


def run_sweep(fs, x, comps, extra=None):
    x = np.asarray(x, np.float32)
    n = x.shape[0]
    w = 256
    assert n % w == 0
    (out,) = g.run_fragment(fs, w, n // w, out_comps=(4,), tbos=[("u_in", x, comps)], uniforms=dict({"u_width": w}, **(extra or {})))
    return out.reshape(n, 4)


def math_sweeps():
    rng = np.random.default_rng(314159)
    q = 65536 // 8
    x = np.concatenate([
        rng.uniform(-90.0, 90.0, q), rng.uniform(-3.0, 3.0, q),                        # exp: the blackbody's exponent range and around 0
        np.exp(rng.uniform(np.log(1e-6), np.log(1e6), q)), rng.uniform(1e-4, 1.0, q),   # log: max(EPS, 1 - rand()) and a wide range
        rng.uniform(0.999, 1.001, q), rng.uniform(-1.0, 1.0, q),                        # log near 1; acos on its domain
        1.0 - np.exp(rng.uniform(np.log(1e-7), 0.0, q)), np.linspace(-1.0, 1.0, q),    # acos near +-1
    ]).astype(np.float32)
    o = run_sweep(MATH_FS, x, 1)
    temps = np.concatenate([np.linspace(0.0, 100.0, 4096), np.exp(rng.uniform(np.log(1e-3), np.log(200.0), 4096))]).astype(np.float32)
    bb = run_sweep(blackbody_fs(), temps, 1)[:, :3]
    grid = rng.random((5, 7, 12), dtype=np.float32)
    lo, hi = np.array([-1.3, 0.05, -0.7], np.float32), np.array([1.1, 1.6, 0.9], np.float32)
    pos = (lo + (hi - lo) * rng.uniform(-0.3, 1.3, (8192, 3))).astype(np.float32)
    pos[:256] = lo + (hi - lo) * ((np.arange(256)[:, None] % np.array([12, 7, 5])) + 0.5) / np.array([12, 7, 5])  # texel centres
    t = tex3d(7, grid)
    look = run_sweep(LOOKUP_FS, pos, 3, {"u_tex": 7, "u_bboxMin": lo, "u_bboxMax": hi})[:, 0]
    glDeleteTextures(1, C.byref(t))
    np.savez_compressed(OUT / "math_volume.npz", x=x, exp=o[:, 0], log=o[:, 1], acos=o[:, 2], temp=temps, blackbody=bb,
                        grid=grid, bbox=np.concatenate([lo, hi]), pos=pos, lookup=look, renderer=np.array(g.info()))
    print(f"math_volume: {x.size} exp/log/acos, {temps.size} blackbody, {pos.shape[0]} lookups")


if __name__ == "__main__":
    main()
