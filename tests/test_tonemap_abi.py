"""Tone mapping (include/glrtx.h "Tone mapping", include/glrt_host.h) without a GPU: the headers declare the calls, both libraries export them, the Python
bindings carry them, the ABI version is what it was, the two new structures have the C layout, the refusals that need no device are refusals, and the new
kernels spill nothing and use no scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = ["glrtx_exposure_measure", "glrtx_exposure_reset", "glrtx_read_exposure", "glrtx_tonemap", "glrtx_read_tonemapped",
                "glrtx_resolve_tonemapped_rgba8", "glrtx_debug_tonemap", "glrtx_debug_tonemap_burst"]
HOST_CALLS = ["glrt_exposure_measure", "glrt_tonemap"]
CFG_FIELDS = ["op", "source", "auto_exposure", "exposure", "key", "low_permille", "high_permille", "adapt", "white", "gamma", "flip_y"]
EXP_FIELDS = ["hist", "counted", "kept", "mean_log2", "target", "exposure", "measurements"]


def test_headers_declare_the_calls_and_keep_the_abi_version():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert "#define GLRTX_ABI_VERSION 10" in text
    for name in DEVICE_CALLS:
        assert re.search(rf"\bint {name}\(", text), name
    m = re.search(r"typedef struct glrtx_tonemap_cfg \{(.*?)\} glrtx_tonemap_cfg;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == CFG_FIELDS
    assert re.search(r"typedef struct glrtx_exposure \{ uint32_t hist\[256\]; uint64_t counted, kept; float mean_log2, target, exposure; int measurements; \}", text)
    host_text = (ROOT / "include" / "glrt_host.h").read_text()
    for name in HOST_CALLS:
        assert re.search(rf"\bint {name}\(", host_text), name


def test_libraries_export_the_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in HOST_CALLS:
        assert hasattr(H, name), name


def test_bindings_carry_the_calls_and_the_defaults():
    from glrt_amd import device, host
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for m in ("exposure_measure", "exposure_reset", "read_exposure", "tonemap", "read_tonemapped", "resolve_tonemapped_rgba8"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_tonemap) and callable(host.exposure_measure) and callable(host.tonemap)
    c = device.TonemapCfg.default()
    assert [getattr(c, k) for k in CFG_FIELDS] == [0, 0, 0, 1.0, np.float32(0.18), 500, 950, 1.0, 4.0, np.float32(2.2), 1]
    c = device.TonemapCfg.default(op="aces", auto_exposure=True, exposure=2.0)
    assert (c.op, c.auto_exposure, c.exposure, c.high_permille) == (2, 1, 2.0, 950)
    with pytest.raises(TypeError):
        device.TonemapCfg.default(colour=1)
    import tonemap_math as tm
    assert tm.DEFAULTS == host.TONEMAP_DEFAULTS


def test_structures_have_the_c_layout(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d", sizeof(glrtx_tonemap_cfg), sizeof(glrtx_exposure), sizeof(glrtx_stats), sizeof(glrtx_denoise_var_cfg), GLRTX_ABI_VERSION);\n'
                   + "".join(f'  printf(" %zu", offsetof(glrtx_tonemap_cfg, {k}));\n' for k in CFG_FIELDS)
                   + "".join(f'  printf(" %zu", offsetof(glrtx_exposure, {k}));\n' for k in EXP_FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:5] == [44, 1056, 168, 20, 10]
    assert got[:4] == [C.sizeof(device.TonemapCfg), C.sizeof(device.Exposure), C.sizeof(device.Stats), C.sizeof(device.DenoiseVarCfg)]
    assert got[5:5 + len(CFG_FIELDS)] == [getattr(device.TonemapCfg, k).offset for k in CFG_FIELDS]
    assert got[5 + len(CFG_FIELDS):] == [getattr(device.Exposure, k).offset for k in EXP_FIELDS]


BAD_CFGS = [dict(op=3), dict(op=-1), dict(source=2), dict(exposure=0.0), dict(exposure=float("nan")), dict(exposure=float("inf")), dict(key=-1.0), dict(adapt=0.0),
            dict(adapt=1.0001), dict(low_permille=-1), dict(low_permille=950, high_permille=500), dict(high_permille=1001), dict(white=0.0), dict(white=1e-30),
            dict(gamma=0.0)]


@pytest.mark.parametrize("bad", BAD_CFGS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_CFGS])
def test_bad_configurations_are_refused_before_any_device_work(bad):
    from glrt_amd import device
    with pytest.raises(device.GlrtxError) as e:
        device.debug_tonemap(np.ones((3, 5, 4), np.float32), **bad)
    assert e.value.code == -1 and "glrtx_debug_tonemap" in str(e.value)


def test_null_and_size_refusals():
    from glrt_amd import device
    L = device.lib()
    z = np.ones((3, 5, 4), np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    cfg = device.TonemapCfg.default()
    assert L.glrtx_debug_tonemap(p, 0, 3, C.byref(cfg), None, None, None, None) == -1
    assert L.glrtx_debug_tonemap(p, 5, 70000, C.byref(cfg), None, None, None, None) == -1
    assert L.glrtx_debug_tonemap(None, 5, 3, C.byref(cfg), None, None, None, None) == -1
    assert L.glrtx_debug_tonemap(p, 5, 3, None, None, None, None, None) == -1
    assert L.glrtx_exposure_measure(None, C.byref(cfg)) == -1 and L.glrtx_exposure_reset(None) == -1 and L.glrtx_read_exposure(None, None) == -1
    assert L.glrtx_tonemap(None, C.byref(cfg)) == -1 and L.glrtx_read_tonemapped(None, None, 0) == -1
    assert L.glrtx_resolve_tonemapped_rgba8(None, None, 0, C.byref(cfg)) == -1


def test_the_kernels_spill_nothing_and_use_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the rows of the four tone-mapping kernels (vgpr agpr sgpr vspill sspill scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("glrtx::tonemap::")]
    assert sorted(row[0] for row in rows) == ["glrtx::tonemap::exposure_histogram", "glrtx::tonemap::exposure_reduce", "glrtx::tonemap::tonemap_plane",
                                              "glrtx::tonemap::tonemap_resolve<2>"], r.stdout
    for row in rows:
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in row[-7:])
        assert vspill == 0 and sspill == 0 and scratch == 0, row
