"""Textured scenes on the wavefront kernel (glrtx_set_texture_wavefront, include/glrtx.h "Textures") without a GPU: the header declares it, libglrtx.so
exports it, the binding and the façade carry it, the ABI version is unchanged, and the T and TM forms' instantiations of pt_render_wgwf keep the register
budget of the other ones (tools/isa_report.py on the built code object)."""
import ctypes as C
import functools
import re
import subprocess
import sys

import pytest

from conftest import PKG, ROOT

# pt_render_wgwf<COUNT_RAYS, VINE, FLAGS>: kWgwfTextured = 32, kWgwfMaps = 64 (with kWgwfTextured), on top of the node fetch (0 one record per lane, 1 pair-cooperative,
# 8 the compact array) and kWgwfAdaptive = 4
T, M, ADAPT = 32, 64, 4
FETCHES = (0, 1, 8)
T_FORMS = [T | f | a for f in FETCHES for a in (0, ADAPT)]
TM_FORMS = [T | M | f | a for f in FETCHES for a in (0, ADAPT)]
INSTANTIATIONS = [f"{count}, false, {flags}" for flags in T_FORMS + TM_FORMS for count in ("false", "true")]


def test_header_declares_the_switch():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert re.search(r"\bint glrtx_set_texture_wavefront\(glrtx_ctx \*ctx, int enable\);", text)
    assert "#define GLRTX_ABI_VERSION 10" in text  # (additive: the version and glrtx_stats stay as they are)
    assert "GLRTX_TEXTURE_WAVEFRONT=0/1" in text


def test_library_and_binding_carry_the_switch():
    from glrt_amd import device
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    assert hasattr(L, "glrtx_set_texture_wavefront")
    assert L.glrtx_abi_version() == 10
    assert C.sizeof(device.Stats) == 168
    assert "glrtx_set_texture_wavefront" in device.EXPORTS
    assert callable(getattr(device.Device, "set_texture_wavefront", None))
    L.glrtx_set_texture_wavefront.argtypes = [C.c_void_p, C.c_int]
    assert L.glrtx_set_texture_wavefront(None, 1) == -1  # a NULL context is refused (GLRTX_EINVAL), no device touched


def test_glrt_main_usage_names_the_flag():
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "--no-such-flag"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0
    assert "--texture-wavefront" in r.stdout


@functools.lru_cache(maxsize=None)
def _isa_check():
    return subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py"), "--check"], capture_output=True, text=True, timeout=300)


def test_isa_check_passes_with_the_new_instantiations():
    r = _isa_check()
    assert r.returncode == 0, r.stdout + r.stderr
    assert len(INSTANTIATIONS) == 24


@pytest.mark.parametrize("inst", INSTANTIATIONS)
def test_t_and_tm_instantiations_keep_the_register_budget(inst):
    """vgpr + agpr <= 128 (four waves a SIMD), no vector or scalar spills, no scratch."""
    r = _isa_check()
    rows = [ln.replace(f"glrtx::pt_render_wgwf<{inst}>", "K").split() for ln in r.stdout.splitlines() if ln.startswith(f"glrtx::pt_render_wgwf<{inst}>")]
    assert rows, (inst, r.stdout)
    vgpr, agpr, sgpr, vspill, sspill, scratch = (int(v) for v in rows[0][1:7])
    assert vspill == 0 and sspill == 0 and scratch == 0 and vgpr + agpr <= 128, (inst, rows[0])
