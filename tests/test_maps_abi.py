"""The material-map calls (include/glrtx.h "Material maps"; include/glrt_host.h) without a GPU: the headers declare them and carry the contract's key lines;
glrtx_material_map is 16 bytes with offsets 0 / 4 / 8 / 12; both libraries export the calls and the Python bindings carry them; the ABI version and the stats
record are what they were; a C99 file that includes both headers compiles; a NULL context gives -1; the debug hook checks its arguments before it touches a device."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_bind_material_maps": r"glrtx_ctx \*ctx, const glrtx_material_map \*maps, size_t n_mat",
    "glrtx_debug_map_normal": r"const float \*records, size_t n, float scale, float \*normal_out",
}
HOST_CALLS = {
    "glrt_map_decode": r"const float \*rgb, size_t n, float \*m_out",
    "glrt_map_normal": r"const float \*records, size_t n, float scale, float \*normal_out",
    "glrt_map_alpha": r"const float \*rgb, size_t n, float \*alpha_out",
}


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert "#define GLRTX_MAP_ALPHA_MIN 1e-3f" in text
    assert "typedef struct glrtx_material_map { int32_t normal, roughness; float normal_scale; int32_t reserved; } glrtx_material_map;" in text
    assert text.index("---- Environment") < text.index("---- Material maps") < text.index("---- Groups")
    for line in ("m = c * 2 + -1", "det = ds1 * dt2 - ds2 * dt1", "Tr = e1 * dt2 - e2 * dt1,  Br = e2 * ds1 - e1 * ds2", "for det < 0 the sign bits of both are inverted",
                 "k = dot(n, Tr),  Tp = Tr - k * n,  l2 = dot(Tp, Tp),  T = Tp * rsq(l2)", "sign bits inverted iff dot(C, Br) < 0", "(x x' + y y') + z z'",
                 "p = (a * T + b * B) + m.z * n", "q = dot(p, p);  n' = p * rsq(q)", "a and b are both zero", "TANGENTS ARE PER TRIANGLE AND ARE NOT INTERPOLATED",
                 "REPLACE alpha.x / alpha.y", "Channel b and alpha are not read", "DROP the maps", "maps == NULL or", "textures are bound", "NOT BUILT: emission maps",
                 "GLRTX_TEX_RGBA8_SRGB; a scale that is not finite; reserved non-zero"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name, args in HOST_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", host_h), name
    assert "#define GLRT_MAP_ALPHA_MIN 1e-3f" in host_h and "#define GLRT_MAP_RECORD_FLOATS 18" in host_h


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
    assert callable(getattr(device.Device, "bind_material_maps", None)) and callable(device.debug_map_normal)
    assert callable(host.map_normal) and callable(host.map_alpha) and callable(scenes.config_mapped_wall)
    dt = host.MATERIAL_MAP_DTYPE
    assert dt.itemsize == 16 and dt.names == ("normal", "roughness", "normal_scale", "reserved") and [dt.fields[k][1] for k in dt.names] == [0, 4, 8, 12]
    assert C.sizeof(device.Stats) == 168


def test_a_c99_file_including_both_headers_compiles(tmp_path):
    src = tmp_path / "both.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glrtx.h"\n#include "glrt_host.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(glrtx_ctx *, const glrtx_material_map *, size_t) = glrtx_bind_material_maps;\n"
                   "    int (*b)(const float *, size_t, float, float *) = glrtx_debug_map_normal;\n"
                   "    int (*c)(const float *, size_t, float, float *) = glrt_map_normal;\n"
                   "    int (*d)(const float *, size_t, float *) = glrt_map_alpha;\n"
                   '    printf("%d %zu %zu %zu %zu %zu %zu %zu %d %d\\n", GLRTX_ABI_VERSION, sizeof(glrtx_material_map), offsetof(glrtx_material_map, normal),\n'
                   "           offsetof(glrtx_material_map, roughness), offsetof(glrtx_material_map, normal_scale), offsetof(glrtx_material_map, reserved),\n"
                   "           sizeof(glrt_material_map), sizeof(glrtx_stats), GLRTX_MAP_RECORD_FLOATS, GLRTX_MAP_ALPHA_MIN == GLRT_MAP_ALPHA_MIN);\n"
                   "    return a && b && c && d ? 0 : 1;\n}\n")
    exe = tmp_path / "both"
    lib = PKG / "lib"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lglrtx", "-lglrt_host",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["10", "16", "0", "4", "8", "12", "16", "168", "18", "1"], (r.stdout, r.stderr)


def test_without_a_context_every_call_fails_cleanly():
    """glrtx_bind_material_maps refuses a NULL context; the debug hook checks its arguments before it touches a device, and with valid arguments either runs (a
    GPU is there) or reports the device's error through glrtx_last_error."""
    from glrt_amd import device, host
    L = device.lib()
    rec = host.material_maps(1, normal=[0])
    assert L.glrtx_bind_material_maps(None, rec.ctypes.data, 1) == -1
    assert L.glrtx_bind_material_maps(None, None, 0) == -1
    L.glrtx_last_error.restype = C.c_char_p
    out = np.zeros(3, np.float32)
    fp = C.POINTER(C.c_float)
    assert L.glrtx_debug_map_normal(None, 1, C.c_float(1.0), out.ctypes.data_as(fp)) == -1 and b"NULL buffer" in L.glrtx_last_error(None)
    one = np.zeros(18, np.float32)
    assert L.glrtx_debug_map_normal(one.ctypes.data_as(fp), 1, C.c_float(1.0), None) == -1 and b"NULL buffer" in L.glrtx_last_error(None)
    assert L.glrtx_debug_map_normal(one.ctypes.data_as(fp), (2 ** 31) // 18 + 1, C.c_float(1.0), out.ctypes.data_as(fp)) == -1 and b"too many" in L.glrtx_last_error(None)
    assert L.glrtx_debug_map_normal(None, 0, C.c_float(1.0), None) == 0
    flat = host.map_records([[0, 1, 0]], [[1, 0, 0]], [[0, 0, -1]], [[0, 0]], [[1, 0]], [[0, 1]], [[0, 0, 1]])
    try:
        got = device.debug_map_normal(flat)
    except device.GlrtxError as e:
        assert e.code == -2 and "glrtx_debug_map_normal" in str(e)
    else:
        assert got.tolist() == [[0.0, 1.0, 0.0]]
