"""The cutout calls (include/glrtx.h "Cutouts"; include/glrt_host.h) without a GPU: the headers declare them and carry the contract's key lines; glrtx_cutout
is 16 bytes with offsets 0 / 4 / 8 / 12, checked from a compiled C program; both libraries export the calls and the Python bindings carry them; the ABI
version and the stats record are what they were; tools/isa_report.py --check passes and reports the eight CUT forms of pt_render_persistent without spills
or scratch; glrt_main --help names the JSON key and nothing else new; a NULL context gives -1 and the debug hook checks its arguments before it touches a device."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_bind_cutouts": r"glrtx_ctx \*ctx, const glrtx_cutout \*cut, size_t n_mat",
    "glrtx_debug_texture_channel": r"const glrtx_texture \*tex, size_t n_tex, const void \*texels, size_t texel_bytes,\s+const int32_t \*which, "
                                   r"const int32_t \*channel, const float \*st, size_t n, float \*value_out",
}
HOST_CALLS = {
    "glrt_texture_channel": r"const glrt_texture \*tex, size_t n_tex, const void \*texels, size_t texel_bytes, const int32_t \*which, const int32_t \*channel, "
                            r"const float \*st,\s+size_t n, float \*value_out",
    "glrt_render_features_geom_cutout": r"const float \*vert, size_t n_vert, .*?const glrt_texture \*tex, size_t n_tex,\s+const void \*texels, size_t texel_bytes, "
                                        r"const int32_t \*material_texture, const glrt_cutout \*cut, float \*out_n, float \*out_a,\s+float \*out_g",
}


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert "typedef struct glrtx_cutout { int32_t texture, channel; float cutoff; int32_t reserved; } glrtx_cutout;" in text
    assert text.index("---- Material maps") < text.index("---- Cutouts") < text.index("---- Groups")
    for line in ("accepted iff value >= cutoff", "A NaN value rejects", "A rejected candidate changes nothing", "(float)byte / 255.0f for BOTH 8-bit formats",
                 "shadow rays to triangle lights (with or without the shadow range limit) and shadow rays to the environment", "are never cut",
                 "Only diffuse (type 2) and conductor (type 3) materials may be bound", "DROP the records", "cut == NULL or n_mat == 0 unbinds",
                 "one 4-byte gather for every would-be-closest candidate", "a channel outside 0 .. 3; a cutoff that is not finite", "reserved non-zero; a vine tree",
                 "cutouts are bound", "glrtx_set_texture_wavefront does not take them", "NOT BUILT: stochastic or blended transparency", "cutouts in glrtx_trace_rays",
                 "mip levels"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name, args in HOST_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", host_h, re.S), name
    assert "typedef struct glrt_cutout { int32_t texture, channel; float cutoff; int32_t reserved; } glrt_cutout;" in host_h


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
    assert callable(getattr(device.Device, "bind_cutouts", None)) and callable(device.debug_texture_channel)
    assert callable(host.texture_channel) and callable(host.render_features_geom_cutout) and callable(scenes.config_cutout_wall)
    dt = host.CUTOUT_DTYPE
    assert dt.itemsize == 16 and dt.names == ("texture", "channel", "cutoff", "reserved") and [dt.fields[k][1] for k in dt.names] == [0, 4, 8, 12]
    assert C.sizeof(device.Stats) == 168


def test_a_c99_file_including_both_headers_compiles(tmp_path):
    src = tmp_path / "both.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glrtx.h"\n#include "glrt_host.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(glrtx_ctx *, const glrtx_cutout *, size_t) = glrtx_bind_cutouts;\n"
                   "    int (*b)(const glrtx_texture *, size_t, const void *, size_t, const int32_t *, const int32_t *, const float *, size_t, float *) = glrtx_debug_texture_channel;\n"
                   "    int (*c)(const glrt_texture *, size_t, const void *, size_t, const int32_t *, const int32_t *, const float *, size_t, float *) = glrt_texture_channel;\n"
                   '    printf("%d %zu %zu %zu %zu %zu %zu %zu\\n", GLRTX_ABI_VERSION, sizeof(glrtx_cutout), offsetof(glrtx_cutout, texture), offsetof(glrtx_cutout, channel),\n'
                   "           offsetof(glrtx_cutout, cutoff), offsetof(glrtx_cutout, reserved), sizeof(glrt_cutout), sizeof(glrtx_stats));\n"
                   "    return a && b && c ? 0 : 1;\n}\n")
    exe = tmp_path / "both"
    lib = PKG / "lib"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lglrtx", "-lglrt_host",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["10", "16", "0", "4", "8", "12", "16", "168"], (r.stdout, r.stderr)


def test_isa_report_checks_pass_and_list_the_eight_cut_forms():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if re.search(r"pt_render_persistent<(\w+, ){6}true>", ln)]
    forms = sorted(re.search(r"<(.*)>", " ".join(row)).group(1) for row in rows)
    assert forms == sorted(f"{count}, true, false, true, {env}, {maps}, true" for count in ("false", "true") for env in ("false", "true") for maps in ("false", "true")), forms
    for row in rows:
        vgpr, _, _, vspill, sspill, scratch, _ = (int(x) for x in row[-7:])
        assert vspill == 0 and sspill == 0 and scratch == 0 and vgpr <= 128, row


def test_glrt_main_help_names_the_json_key_and_nothing_else_new():
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "--help"], capture_output=True, text=True, timeout=60)
    text = r.stdout + r.stderr
    assert "--cutout" not in text and "--alpha" not in text
    if '"texture"' in text:  # the help lists the shapes' JSON keys: then "cutout" is one of them
        assert '"cutout"' in text


def test_without_a_context_every_call_fails_cleanly():
    from glrt_amd import device, host
    L = device.lib()
    rec = host.cutouts(1, texture=[0])
    assert L.glrtx_bind_cutouts(None, rec.ctypes.data, 1) == -1
    assert L.glrtx_bind_cutouts(None, None, 0) == -1
    assert L.glrtx_debug_last_kernel(None) == b""
    L.glrtx_last_error.restype = C.c_char_p
    tex = [(np.full((2, 2, 4), 0.25, np.float32), "rgba32f", "repeat", "nearest")]
    desc, blob = host.pack_textures(tex)
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    one, st, out = np.zeros(1, np.int32), np.zeros(2, np.float32), np.zeros(1, np.float32)
    args = (desc.ctypes.data, 1, blob.ctypes.data, blob.size)
    assert L.glrtx_debug_texture_channel(*args, one.ctypes.data_as(i32p), one.ctypes.data_as(i32p), st.ctypes.data_as(fp), 1, None) == -1
    assert b"NULL buffer" in L.glrtx_last_error(None)
    assert L.glrtx_debug_texture_channel(*args, one.ctypes.data_as(i32p), None, st.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) == -1
    four = np.full(1, 4, np.int32)
    assert L.glrtx_debug_texture_channel(*args, one.ctypes.data_as(i32p), four.ctypes.data_as(i32p), st.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) == -1
    assert b"channel 4" in L.glrtx_last_error(None)
    assert L.glrtx_debug_texture_channel(*args, four.ctypes.data_as(i32p), one.ctypes.data_as(i32p), st.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) == -1
    assert b"texture 4 of 1" in L.glrtx_last_error(None)
    assert L.glrtx_debug_texture_channel(*args, None, None, None, 0, None) == 0
    try:
        got = device.debug_texture_channel(tex, [0], 3, [[0.5, 0.5]])
    except device.GlrtxError as e:
        assert e.code == -2 and "glrtx_debug_texture_channel" in str(e)
    else:
        assert got.tolist() == [0.25]
