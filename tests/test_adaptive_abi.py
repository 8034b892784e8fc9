"""Adaptive sampling (glrtx_render_adaptive and its companions, include/glrtx.h) without a GPU: the header declares it, libglrtx.so exports it,
the Python binding carries it and its ctypes structure has the C layout (checked against the header by the C compiler itself)."""
import ctypes as C
import re
import subprocess

from conftest import PKG, ROOT

ADAPTIVE = ["glrtx_render_adaptive", "glrtx_adaptive_active_tiles", "glrtx_read_tile_mask", "glrtx_read_adaptive_half", "glrtx_debug_adaptive_select",
            "glrtx_group_render_adaptive", "glrtx_group_adaptive_active_tiles"]


def test_header_declares_adaptive_calls_and_struct():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name in ADAPTIVE:
        assert re.search(rf"\bint {name}\(", text), name
    assert re.search(r"typedef struct glrtx_adaptive \{\s*float threshold;[^}]*int min_samples;[^}]*\} glrtx_adaptive;", text)
    assert "#define GLRTX_ABI_VERSION 10" in text  # (additive: the version and glrtx_stats stay as they are)


def test_library_exports_adaptive_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in ADAPTIVE:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10


def test_binding_carries_adaptive_calls():
    from glrt_amd import device
    assert set(ADAPTIVE) <= set(device.EXPORTS)
    for cls in (device.Device, device.Group):
        for m in ("render_adaptive", "adaptive_active_tiles", "tile_mask", "read_adaptive_half"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
    assert callable(device.adaptive_select)
    assert C.sizeof(device.Stats) == 168


def test_ctypes_adaptive_matches_the_c_layout(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu\\n", sizeof(glrtx_adaptive), offsetof(glrtx_adaptive, threshold), offsetof(glrtx_adaptive, min_samples),\n'
                   "         sizeof(glrtx_stats));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(device.Adaptive), device.Adaptive.threshold.offset, device.Adaptive.min_samples.offset, C.sizeof(device.Stats)]


def test_lum_floor_is_the_kernels():
    import adaptive_math as am
    text = (PKG / "csrc" / "pt_kernel.hip.h").read_text()
    m = re.search(r"constexpr float kAdaptLumFloor = ([0-9.e+-]+)f;", text)
    assert m and float(am.LUM_FLOOR) == float(__import__("numpy").float32(m.group(1)))
