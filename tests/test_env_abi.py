"""The environment calls (include/glrtx.h "Environment"; include/glrt_host.h) without a GPU: the headers declare them and carry the contract's key lines;
glrtx_env_cfg is 60 bytes with the offsets of the ctypes mirror, through a compiled C program; both libraries export the calls and the Python bindings carry
them; the ABI version and the stats record are what they were; without a context every call fails cleanly and every refusal names its offender."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

MAP = r"const glrtx_texture \*map, const void \*texels, size_t texel_bytes, const glrtx_env_cfg \*cfg"
HMAP = MAP.replace("glrtx_", "glrt_")
DEVICE_CALLS = {
    "glrtx_upload_environment": rf"glrtx_ctx \*ctx, {MAP}",
    "glrtx_set_environment_cfg": r"glrtx_ctx \*ctx, const glrtx_env_cfg \*cfg",
    "glrtx_debug_env_weights": rf"{MAP}, float \*weights_out, int32_t \*grid_out",
    "glrtx_debug_env_sample": rf"{MAP}, const float \*u, size_t n, float \*out",
    "glrtx_debug_env_eval": rf"{MAP}, const float \*dir, size_t n, float \*out",
}
HOST_CALLS = {
    "glrt_env_weights": rf"{HMAP}, float \*weights_out, int32_t \*grid_out",
    "glrt_env_alias": r"const float \*weights, int32_t grid, float \*row_q, int32_t \*row_alias, float \*col_q, int32_t \*col_alias, float \*cell_p",
    "glrt_env_sample": rf"{HMAP}, const float \*u, size_t n, float \*out",
    "glrt_env_eval": rf"{HMAP}, const float \*dir, size_t n, float \*out",
    "glrt_env_from_latlong": r"const float \*rgb, int32_t width, int32_t height, int32_t n, float \*rgba_out",
}


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert "enum glrtx_env_mode { GLRTX_ENV_ESCAPE = 0, GLRTX_ENV_SAMPLED = 1 };" in text
    assert "typedef struct glrtx_env_cfg { int32_t mode; int32_t grid; float light_pick; float scale[3]; float rotation[9]; } glrtx_env_cfg;" in text
    assert text.index("---- Textures") < text.index("---- Environment") < text.index("---- Groups")
    for line in ("OCTAHEDRAL with +y as the fold axis", "l = (|ex| + |ey|) + |ez|", "l zero or not finite: the radiance is 0", "sgn(0) = sgn(-0) = +1",
                 "s = px * 0.5 + 0.5,  t = pz * 0.5 + 0.5", "u = s * 2 - 1,  v = t * 2 - 1,  y = (1 - |u|) - |v|", "dOmega = 4 n1^3 ds dt", "J = 4 * ((n1 * n1) * n1)",
                 "across the fold seams is NOT", "L += beta * Le(d), at every depth", "lid = (int)(((rl - p_env) / (1 - p_env)) * nLights)",
                 "forced to 1 for a scene without lights", "pdf = ((cell_p[cj * G + ci] * (G * G)) / J) * p_env", "the BSDF VALUE", "accepted when the ray hits nothing",
                 "WHY SAMPLED FOR A SUN", "WIDENED by one on every side", "p[k] += p[k + h] for h = 32, 16, .. 1", "Vose's alias method", "An all-zero grid is legal",
                 "map == NULL unbinds", "KEPT across glrtx_upload_scene", "an environment is bound", "GLRTX_EXT_VOLUME does not", "NOT BUILT"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name, args in HOST_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", host_h), name


def test_libraries_export_the_calls_and_bindings_carry_them():
    from glrt_amd import device, host, scenes
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in HOST_CALLS:
        assert hasattr(H, name), name
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for name in ("upload_environment", "set_environment_cfg"):
        assert callable(getattr(device.Device, name, None)), name
    assert callable(device.debug_env_weights) and callable(device.debug_env_sample) and callable(device.debug_env_eval) and device.EnvCfg is host.EnvCfg
    for fn in (host.env_weights, host.env_alias, host.env_sample, host.env_eval, host.env_from_latlong, host.env_cfg, scenes.config_env_quad, scenes.config_env_sky,
               scenes.config_env_box, scenes.env_octant_map):
        assert callable(fn)
    assert C.sizeof(device.Stats) == 168 and (device.ENV_ESCAPE, device.ENV_SAMPLED) == (0, 1)


def test_env_cfg_layout_equals_the_ctypes_mirror(tmp_path):
    from glrt_amd import device
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glrtx.h"\n#include "glrt_host.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(glrtx_ctx *, const glrtx_texture *, const void *, size_t, const glrtx_env_cfg *) = glrtx_upload_environment;\n"
                   "    int (*b)(const glrt_texture *, const void *, size_t, const glrt_env_cfg *, float *, int32_t *) = glrt_env_weights;\n"
                   '    printf("%d %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", GLRTX_ABI_VERSION, sizeof(glrtx_env_cfg), sizeof(glrt_env_cfg), offsetof(glrtx_env_cfg, mode),\n'
                   "           offsetof(glrtx_env_cfg, grid), offsetof(glrtx_env_cfg, light_pick), offsetof(glrtx_env_cfg, scale), offsetof(glrtx_env_cfg, rotation),\n"
                   "           sizeof(glrtx_stats), (int)GLRTX_ENV_ESCAPE, (int)GLRTX_ENV_SAMPLED);\n"
                   "    return a && b ? 0 : 1;\n}\n")
    exe = tmp_path / "layout"
    lib = PKG / "lib"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lglrtx", "-lglrt_host",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    E = device.EnvCfg
    mirror = [10, C.sizeof(E), C.sizeof(E), E.mode.offset, E.grid.offset, E.light_pick.offset, E.scale.offset, E.rotation.offset, 168, 0, 1]
    assert r.returncode == 0 and [int(v) for v in r.stdout.split()] == mirror == [10, 60, 60, 0, 4, 8, 12, 24, 168, 0, 1], (r.stdout, r.stderr, mirror)


def test_without_a_context_every_call_fails_cleanly():
    """The context calls refuse a NULL context; the debug hooks check their arguments before they touch a device -- every refusal names its offender -- and with
    valid arguments either run (a GPU is there) or report the device's error through glrtx_last_error."""
    from glrt_amd import device, host
    L = device.lib()
    env_map = (np.full((4, 4, 3), 0.25, np.float32), "rgba32f", "bilinear")
    desc, blob = host.pack_environment(env_map)
    cfg = host.env_cfg()
    assert L.glrtx_upload_environment(None, desc.ctypes.data, blob.ctypes.data, blob.size, C.addressof(cfg)) == -1
    assert b"NULL context" in L.glrtx_last_error(None)
    assert L.glrtx_set_environment_cfg(None, C.addressof(cfg)) == -1 and b"NULL context" in L.glrtx_last_error(None)

    def refused(words, m=(desc, blob), c=cfg):
        for call in (lambda: device.debug_env_weights(m, c), lambda: device.debug_env_sample(m, c, np.zeros((1, 6))), lambda: device.debug_env_eval(m, c, [[0, 1, 0]])):
            with pytest.raises(device.GlrtxError) as e:
                call()
            assert e.value.code == -1 and words in str(e.value), str(e.value)
        assert lib_host_refuses(m, c)

    def lib_host_refuses(m, c):
        with pytest.raises(RuntimeError, match="failed: -1"):
            host.env_weights(m, c)
        return True

    def edited(field, value):
        d = desc.copy()
        d[field][0] = value
        return d, blob

    refused("NULL configuration", c=None)
    refused("4 x 3 texels (an octahedral map is square", edited("height", 3))
    one = host.pack_environment((np.zeros((1, 1, 3), np.float32), "rgba32f", "nearest"))
    refused("1 x 1 texels (an octahedral map is square, 2 ..", one)
    refused("wrap mode 0 / 1 (an octahedral map clamps", edited("wrap_s", 0))
    refused("wrap mode 1 / 0", edited("wrap_t", 0))
    refused("map: texture 0: unknown format 3", edited("format", 3))
    refused("map: texture 0: unknown filter 2", edited("filter", 2))
    refused("map: texture 0: offset 4 is not a multiple of 16", edited("offset", 4))
    refused("map: texture 0: 4 x 16385 texels", edited("height", 16385))
    refused("last texel lies past", (desc, blob[:-16]))
    refused("mode 2 (0 escape, 1 sampled)", c=host.env_cfg(2))
    refused("mode -1", c=host.env_cfg(-1))
    refused("grid 1025", c=host.env_cfg(grid=1025))
    refused("grid -1", c=host.env_cfg(grid=-1))
    refused("light_pick -0.5 lies outside [0, 1]", c=host.env_cfg(light_pick=-0.5))
    refused("light_pick 1.25", c=host.env_cfg(light_pick=1.25))
    refused("light_pick nan", c=host.env_cfg(light_pick=float("nan")))
    refused("scale[0] = -1 is negative or not finite", c=host.env_cfg(scale=(-1, 1, 1)))
    refused("scale[2] = inf", c=host.env_cfg(scale=(1, 1, np.inf)))
    refused("scale[1] = nan", c=host.env_cfg(scale=(1, np.nan, 1)))
    refused("rotation[8] = inf is not finite", c=host.env_cfg(rotation=(1, 0, 0, 0, 1, 0, 0, 0, np.inf)))
    refused("rotation[3] = nan", c=host.env_cfg(rotation=(1, 0, 0, np.nan, 1, 0, 0, 0, 1)))
    try:
        got = device.debug_env_eval(env_map, cfg, [[0, 1, 0]])
    except device.GlrtxError as e:
        assert e.code == -2
    else:
        assert got[0, :3].tolist() == [0.25, 0.25, 0.25]
