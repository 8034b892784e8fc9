"""The volume on the wavefront kernel (glrtx_set_volume_wavefront, include/glrtx.h) without a GPU: the header declares it, libglrtx.so exports it,
the binding and the façade carry it, the ABI version is unchanged, and the V form's instantiations of pt_render_wgwf keep the register budget of
the other ones (tools/isa_report.py on the built code object)."""
import ctypes as C
import re
import subprocess
import sys

from conftest import PKG, ROOT


def test_header_declares_the_switch():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert re.search(r"\bint glrtx_set_volume_wavefront\(glrtx_ctx \*ctx, int enable\);", text)
    assert "#define GLRTX_ABI_VERSION 10" in text  # (additive: the version and glrtx_stats stay as they are)


def test_library_and_binding_carry_the_switch():
    from glrt_amd import device
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    assert hasattr(L, "glrtx_set_volume_wavefront")
    assert L.glrtx_abi_version() == 10
    assert "glrtx_set_volume_wavefront" in device.EXPORTS
    assert callable(getattr(device.Device, "set_volume_wavefront", None))
    L.glrtx_set_volume_wavefront.argtypes = [C.c_void_p, C.c_int]
    assert L.glrtx_set_volume_wavefront(None, 1) != 0  # a NULL context is refused (GLRTX_EINVAL), no device touched


def test_glrt_main_usage_names_the_flag():
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--volume-wavefront" in r.stdout


def test_v_form_instantiations_keep_the_register_budget():
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py"), "--check"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    for inst in ("false, false, 16", "true, false, 16", "false, false, 20", "true, false, 20"):
        rows = [ln.replace(f"glrtx::pt_render_wgwf<{inst}>", "K").split() for ln in r.stdout.splitlines() if ln.startswith(f"glrtx::pt_render_wgwf<{inst}>")]
        assert rows, (inst, r.stdout)
        vgpr, agpr, sgpr, vspill, sspill, scratch = (int(v) for v in rows[0][1:7])
        assert vspill == 0 and sspill == 0 and scratch == 0 and vgpr + agpr <= 128, (inst, rows[0])
