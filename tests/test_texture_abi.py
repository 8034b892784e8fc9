"""The texture calls (include/glrtx.h "Textures"; include/glrt_host.h) without a GPU: the headers declare them and the three enumerations and carry the
contract's key lines; glrtx_texture is 32 bytes; both libraries export the calls and the Python bindings carry them; the ABI version and the stats record are
what they were; a C file that includes both headers compiles; without a context every call fails cleanly through glrtx_last_error."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_upload_textures": r"glrtx_ctx \*ctx, const glrtx_texture \*tex, size_t n_tex, const void \*texels, size_t texel_bytes, const int32_t \*material_texture,"
                             r"\s+size_t n_mat",
    "glrtx_debug_texture_lookup": r"const glrtx_texture \*tex, size_t n_tex, const void \*texels, size_t texel_bytes, const int32_t \*which, const float \*st, size_t n,"
                                  r"\s+float \*rgb_out",
}
HOST_CALLS = {
    "glrt_texture_lookup": r"const glrt_texture \*tex, size_t n_tex, const void \*texels, size_t texel_bytes, const int32_t \*which, const float \*st, size_t n,"
                           r"\s+float \*rgb_out",
    "glrt_texture_albedo": r"const float \*vert, size_t n_vert, const float \*tri, size_t n_tri, const float \*mat, size_t n_mat, const glrt_texture \*tex, size_t n_tex,"
                           r"\s+const void \*texels, size_t texel_bytes, const int32_t \*material_texture, const float \*hits, size_t n, float \*rgb_out",
}


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert "enum glrtx_tex_format { GLRTX_TEX_RGBA32F = 0, GLRTX_TEX_RGBA8_UNORM = 1, GLRTX_TEX_RGBA8_SRGB = 2 };" in text
    assert "enum glrtx_tex_wrap { GLRTX_TEX_REPEAT = 0, GLRTX_TEX_CLAMP = 1 };" in text
    assert "enum glrtx_tex_filter { GLRTX_TEX_NEAREST = 0, GLRTX_TEX_BILINEAR = 1 };" in text
    assert text.index("---- Rebuilding normals") < text.index("---- Textures") < text.index("---- Groups")
    for line in ("x = s - floor(s)", "x = s > 0 ? s : 0, then x = x < 1 ? x : 1", "a = x * (float)N", "i = (int)floor(a)", "b = a - 0.5, fl = floor(b), f = b - fl",
                 "c0 = t00 + fx * (t10 - t00),  c1 = t01 + fx * (t11 - t01)", "c = c0 + fy * (c1 - c0)", "(float)b / 255.0f", "A non-finite s or t is 0",
                 "w0 = (1 - u) - v,  s = (w0 * s0 + u * s1) + v * s2", "REPLACES param0", "FROZEN from then on", "glrtx_upload_scene drops the set",
                 "n_tex = 0 unbinds", "textures are bound", "No mip levels", "row 0 is t = 0", "Alpha is never read"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name, args in HOST_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", host_h), name
    assert "const float *glrt_srgb_table(void);" in host_h and "#define GLRT_TEX_RGBA8_SRGB 2" in host_h


def test_libraries_export_the_calls_and_bindings_carry_them():
    from glrt_amd import device, host, scenes
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in list(HOST_CALLS) + ["glrt_srgb_table"]:
        assert hasattr(H, name), name
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    assert callable(getattr(device.Device, "upload_textures", None)) and callable(device.debug_texture_lookup)
    assert callable(host.texture_lookup) and callable(host.texture_albedo) and callable(host.srgb_table) and callable(scenes.config_textured_wall)
    assert host.TEXTURE_DTYPE.itemsize == 32 and [host.TEXTURE_DTYPE.fields[k][1] for k in host.TEXTURE_DTYPE.names] == [0, 8, 12, 16, 20, 24, 28]
    assert C.sizeof(device.Stats) == 168


def test_a_c_file_including_both_headers_compiles(tmp_path):
    src = tmp_path / "both.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glrtx.h"\n#include "glrt_host.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(glrtx_ctx *, const glrtx_texture *, size_t, const void *, size_t, const int32_t *, size_t) = glrtx_upload_textures;\n"
                   "    int (*b)(const glrt_texture *, size_t, const void *, size_t, const int32_t *, const float *, size_t, float *) = glrt_texture_lookup;\n"
                   '    printf("%d %zu %zu %zu %zu %zu %d %d %d %d\\n", GLRTX_ABI_VERSION, sizeof(glrtx_texture), sizeof(glrt_texture), offsetof(glrtx_texture, width),\n'
                   "           offsetof(glrtx_texture, filter), sizeof(glrtx_stats), (int)GLRTX_TEX_RGBA8_SRGB, (int)GLRTX_TEX_CLAMP, (int)GLRTX_TEX_BILINEAR, GLRTX_TEX_MAX);\n"
                   "    return a && b && glrt_srgb_table()[255] == 1.0f ? 0 : 1;\n}\n")
    exe = tmp_path / "both"
    lib = PKG / "lib"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lglrtx", "-lglrt_host",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["10", "32", "32", "8", "28", "168", "2", "1", "1", "4096"], (r.stdout, r.stderr)


def test_without_a_context_every_call_fails_cleanly():
    """glrtx_upload_textures refuses a NULL context; the debug hook checks its arguments before it touches a device, and with valid arguments either runs (a GPU
    is there) or reports the device's error through glrtx_last_error."""
    from glrt_amd import device, host
    L = device.lib()
    tex = [(np.full((2, 3, 3), 0.25, np.float32), "rgba32f", "repeat", "bilinear")]
    desc, blob = host.pack_textures(tex)
    bind = np.zeros(1, np.int32)
    assert L.glrtx_upload_textures(None, desc.ctypes.data, 1, blob.ctypes.data, blob.size, bind.ctypes.data_as(C.POINTER(C.c_int32)), 1) == -1
    for field, value, words in (("width", 0, "0 x 2 texels"), ("height", 16385, "3 x 16385"), ("format", 3, "unknown format 3"), ("wrap_s", 2, "unknown wrap mode"),
                                ("filter", -1, "unknown filter -1"), ("offset", 4, "not a multiple of 16"), ("height", 3, "last texel lies past")):
        d = desc.copy()
        d[field][0] = value
        with pytest.raises(device.GlrtxError) as e:
            device.debug_texture_lookup((d, blob), [0], [[0.5, 0.5]])
        assert e.value.code == -1 and "texture 0" in str(e.value) and words in str(e.value), str(e.value)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_texture_lookup(tex, [1], [[0.5, 0.5]])
    assert e.value.code == -1 and "names texture 1 of 1" in str(e.value)
    try:
        got = device.debug_texture_lookup(tex, [0], [[0.5, 0.5]])
    except device.GlrtxError as e:
        assert e.code == -2 and "glrtx_debug_texture_lookup" in str(e)
    else:
        assert got.tolist() == [[0.25, 0.25, 0.25]]
