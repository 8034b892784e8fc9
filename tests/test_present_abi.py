"""Presentation (glrtx_present_*, include/glrtx.h) without a GPU: the header declares it, libglrtx.so exports it, the Python binding carries it and its
ctypes structures have the C layout (checked against the header by the C compiler itself)."""
import ctypes as C
import re
import subprocess

from conftest import PKG, ROOT

PRESENT = ["glrtx_present_enable", "glrtx_present_acquire", "glrtx_present_release", "glrtx_present_get_stats",
           "glrtx_group_present_enable", "glrtx_group_present_acquire", "glrtx_group_present_release", "glrtx_group_present_get_stats"]


def test_header_declares_presentation_and_ebusy():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name in PRESENT:
        assert re.search(rf"\bint {name}\(", text), name
    m = re.search(r"#define GLRTX_EBUSY \((-?\d+)\)", text)
    assert m and int(m.group(1)) == -6
    assert "#define GLRTX_ABI_VERSION 10" in text  # (additive: the version and glrtx_stats stay as they are)


def test_library_exports_presentation():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in PRESENT:
        assert hasattr(L, name), name


def test_binding_carries_presentation():
    from glrt_amd import device
    assert device.GLRTX_EBUSY == -6
    assert set(PRESENT) <= set(device.EXPORTS)
    for cls in (device.Device, device.Group):
        for m in ("present_enable", "present_acquire", "present_release", "present_stats"):
            assert callable(getattr(cls, m, None)), (cls.__name__, m)
    assert C.sizeof(device.Stats) == 168


def test_ctypes_structs_match_the_c_layout(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\n'
                   "int main(void) {\n"
                   '  printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(glrtx_image), offsetof(glrtx_image, frame), sizeof(glrtx_present_stats),\n'
                   "         offsetof(glrtx_present_stats, ring_images), offsetof(glrtx_present_stats, pass_ms_last), sizeof(glrtx_stats));\n"
                   "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(device.Image), device.Image.frame.offset, C.sizeof(device.PresentStats),
                   device.PresentStats.ring_images.offset, device.PresentStats.pass_ms_last.offset, C.sizeof(device.Stats)]
