"""The emission-map calls (include/glrtx.h "Emission maps"; include/glrt_host.h) without a GPU: the headers declare them and carry the contract's key lines,
placed after "Cutouts"; both libraries export the calls and the Python bindings carry them; the ABI version and the stats record are what they were;
tools/isa_report.py --check passes and reports the eight emission-map forms of pt_render_persistent without spills or scratch, and the forms that existed keep
their seven-argument names; a NULL context fails cleanly."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_bind_emission_maps": r"glrtx_ctx \*ctx, const int32_t \*material_emission, size_t n_mat",
    "glrtx_debug_light_emission": r"glrtx_ctx \*ctx, const int32_t \*lid, const float \*u, size_t n, float \*out",
}
HOST_CALLS = ("glrt_light_st", "glrt_light_emission", "glrt_emission_albedo", "glrt_emission_bind_check")


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert text.index("---- Cutouts") < text.index("---- Emission maps") < text.index("---- Groups")
    for line in ("Le = emission * c, per channel", "ONE\n *   rounded fp32 product", "The texture multiplies the emission; it does not replace it", "Both\n *   faces emit",
                 "w0 = (1 - ua) - ub, s = (w0 * s0 + ua * s1) + ub * s2", "The lookup happens only for a sample that contributes", "the light pick stays uniform",
                 "Analytic spheres have no coordinates and emit their plain emission", "NULL or n_mat == 0 unbinds", "DROP the bindings",
                 "any type except media (type 5)", "Seals an open fed launch", "glrtx_set_texture_wavefront does not take them", "emission maps are bound",
                 "SUPERSEDES", "NOT BUILT: picking lights by power", "emission maps on the wavefront kernel, beside the volume or beside cutouts", "MIS; mip levels"):
        assert line in text, line
    # the two remarks the section supersedes stay as text
    assert "NOT BUILT: emission maps" in text and "an emitter may not, because" in text
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name in HOST_CALLS:
        assert re.search(rf"\bint {name}\(", host_h), name


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
    assert callable(getattr(device.Device, "bind_emission_maps", None)) and callable(device.debug_light_emission)
    assert callable(host.light_emission) and callable(host.emission_albedo) and callable(host.light_st) and callable(scenes.config_emissive_wall)
    assert C.sizeof(device.Stats) == 168


def test_a_c99_file_including_both_headers_compiles(tmp_path):
    src = tmp_path / "both.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "glrtx.h"\n#include "glrt_host.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(glrtx_ctx *, const int32_t *, size_t) = glrtx_bind_emission_maps;\n"
                   "    int (*b)(glrtx_ctx *, const int32_t *, const float *, size_t, float *) = glrtx_debug_light_emission;\n"
                   "    int (*c)(const float *, size_t, const float *, size_t, float *) = glrt_light_st;\n"
                   '    printf("%d %zu\\n", GLRTX_ABI_VERSION, sizeof(glrtx_stats));\n'
                   "    return a && b && c ? 0 : 1;\n}\n")
    exe = tmp_path / "both"
    lib = PKG / "lib"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lglrtx", "-lglrt_host",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["10", "168"], (r.stdout, r.stderr)


def test_isa_report_checks_pass_and_list_the_eight_emission_forms():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py"), "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    rows = [ln.split() for ln in r.stdout.splitlines() if re.search(r"pt_render_persistent<(\w+, ){7}glrtx::Emit>", ln)]
    forms = sorted(re.search(r"<(.*)>", " ".join(row)).group(1) for row in rows)
    assert forms == sorted(f"{count}, true, false, true, {env}, {maps}, false, glrtx::Emit" for count in ("false", "true") for env in ("false", "true")
                           for maps in ("false", "true")), forms
    for row in rows:
        vgpr, _, _, vspill, sspill, scratch, _ = (int(x) for x in row[-7:])
        assert vspill == 0 and sspill == 0 and scratch == 0 and vgpr <= 128, row
    # every form that existed keeps its seven-argument name: 28 of them, the eight CUT forms among them
    old = [ln for ln in r.stdout.splitlines() if re.search(r"pt_render_persistent<(\w+, ){6}\w+>", ln)]
    assert len(old) == 28, len(old)


def test_without_a_context_every_call_fails_cleanly():
    from glrt_amd import device
    L = device.lib()
    L.glrtx_last_error.restype = C.c_char_p
    one = np.zeros(1, np.int32)
    i32p, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    assert L.glrtx_bind_emission_maps(None, one.ctypes.data_as(i32p), 1) == -1
    assert b"glrtx_bind_emission_maps: NULL context" in L.glrtx_last_error(None)
    assert L.glrtx_bind_emission_maps(None, None, 0) == -1
    u, out = np.zeros(2, np.float32), np.zeros(5, np.float32)
    assert L.glrtx_debug_light_emission(None, one.ctypes.data_as(i32p), u.ctypes.data_as(fp), 1, out.ctypes.data_as(fp)) == -1
    assert b"glrtx_debug_light_emission: NULL context" in L.glrtx_last_error(None)
