"""Bloom (include/glrtx.h "Bloom", include/glrt_host.h) without a GPU: the headers declare the calls, both libraries export them, the Python bindings carry them,
the ABI version is what it was, glrtx_bloom_cfg has the C layout, the refusals that need no device are refusals, and the new kernels spill nothing and use no
scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = ["glrtx_bloom", "glrtx_read_bloomed", "glrtx_tonemap_bloomed", "glrtx_resolve_bloomed_rgba8", "glrtx_debug_bloom", "glrtx_debug_bloom_burst"]
HOST_CALLS = ["glrt_bloom"]
CFG_FIELDS = ["source", "threshold", "strength", "levels"]


def test_headers_declare_the_calls_and_keep_the_abi_version():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert "#define GLRTX_ABI_VERSION 10" in text
    for name in DEVICE_CALLS:
        assert re.search(rf"\bint {name}\(", text), name
    m = re.search(r"typedef struct glrtx_bloom_cfg \{(.*?)\} glrtx_bloom_cfg;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert re.findall(r"(\w+)\s*[,;]", body) == CFG_FIELDS
    assert "conventional values, not tuned on anything" in text
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
    for m in ("bloom", "read_bloomed", "tonemap_bloomed", "resolve_bloomed_rgba8"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_bloom) and callable(host.bloom)
    c = device.BloomCfg.default()
    assert [getattr(c, k) for k in CFG_FIELDS] == [0, 1.0, 0.25, 5]
    c = device.BloomCfg.default(source=1, strength=2.0)
    assert (c.source, c.threshold, c.strength, c.levels) == (1, 1.0, 2.0, 5)
    with pytest.raises(TypeError):
        device.BloomCfg.default(radius=1)
    import bloom_math as bm
    assert bm.DEFAULTS == host.BLOOM_DEFAULTS


def test_the_structure_has_the_c_layout(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d", sizeof(glrtx_bloom_cfg), sizeof(glrtx_tonemap_cfg), sizeof(glrtx_stats), GLRTX_ABI_VERSION);\n'
                   + "".join(f'  printf(" %zu", offsetof(glrtx_bloom_cfg, {k}));\n' for k in CFG_FIELDS) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:4] == [16, 44, 168, 10]
    assert got[:3] == [C.sizeof(device.BloomCfg), C.sizeof(device.TonemapCfg), C.sizeof(device.Stats)]
    assert got[4:] == [getattr(device.BloomCfg, k).offset for k in CFG_FIELDS] == [0, 4, 8, 12]


BAD_CFGS = [dict(source=2), dict(source=-1), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(strength=-0.5),
            dict(strength=1.0001e4), dict(strength=float("nan")), dict(strength=float("inf")), dict(levels=0), dict(levels=9), dict(levels=-3)]


@pytest.mark.parametrize("bad", BAD_CFGS, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD_CFGS])
def test_bad_configurations_are_refused_before_any_device_work(bad):
    from glrt_amd import device
    with pytest.raises(device.GlrtxError) as e:
        device.debug_bloom(np.ones((3, 5, 4), np.float32), **bad)
    assert e.value.code == -1 and "glrtx_debug_bloom" in str(e.value)


def test_null_and_size_refusals():
    from glrt_amd import device
    L = device.lib()
    z = np.ones((3, 5, 4), np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    cfg, tcfg = device.BloomCfg.default(), device.TonemapCfg.default()
    assert L.glrtx_debug_bloom(p, 0, 3, C.byref(cfg), None, None) == -1
    assert L.glrtx_debug_bloom(p, 5, 70000, C.byref(cfg), None, None) == -1
    assert L.glrtx_debug_bloom(None, 5, 3, C.byref(cfg), None, None) == -1
    assert L.glrtx_debug_bloom(p, 5, 3, None, None, None) == -1
    assert L.glrtx_bloom(None, C.byref(cfg)) == -1 and L.glrtx_read_bloomed(None, None, 0) == -1
    assert L.glrtx_tonemap_bloomed(None, C.byref(tcfg)) == -1 and L.glrtx_resolve_bloomed_rgba8(None, None, 0, C.byref(tcfg)) == -1
    assert L.glrtx_debug_bloom_burst(None, C.byref(cfg), 1, None) == -1


def test_the_kernels_spill_nothing_and_use_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the rows of the four bloom kernels (vgpr agpr sgpr vspill sspill scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("glrtx::bloom::")]
    assert sorted(row[0] for row in rows) == ["glrtx::bloom::bloom_down<false>", "glrtx::bloom::bloom_down<true>", "glrtx::bloom::bloom_up<false>",
                                              "glrtx::bloom::bloom_up<true>"], r.stdout
    for row in rows:
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in row[-7:])
        assert vspill == 0 and sspill == 0 and scratch == 0, row
        assert 0 < lds <= 40 * 1024, row  # (both passes stage their footprint in LDS; four workgroups of the down pass fit a CU)
