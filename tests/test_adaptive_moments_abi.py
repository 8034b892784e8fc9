"""Adaptive sampling by variance (include/glrtx.h "Adaptive sampling by variance", include/glrt_host.h) without a GPU: the headers declare the calls, both
libraries export them, the Python bindings carry them, the ABI version and glrtx_stats are what they were, the luminance floor is the one constant the H form
uses, the refusals that need no device are refusals, and the two new kernels spill nothing and use no scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np

from conftest import PKG, ROOT

import adaptive_moments_math as amm

DEVICE_CALLS = ["glrtx_render_adaptive_moments", "glrtx_debug_adaptive_select_moments"]
HOST_CALLS = ["glrt_adaptive_select_moments"]


def test_headers_declare_the_calls_and_keep_the_abi_version():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert re.search(r"\bint glrtx_render_adaptive_moments\(glrtx_ctx \*ctx, const glrtx_params \*params, const float \*seeds_xy, int n_frames, "
                     r"const glrtx_adaptive \*cfg\);", text)
    assert re.search(r"\bint glrtx_debug_adaptive_select_moments\(const float \*moments, int width, int rows, float threshold, int min_samples, uint8_t \*mask_out, "
                     r"float \*err_out, int \*list_out,\s+int \*count_out\);", text)
    assert "NOT INTERCHANGEABLE" in text  # (the thresholds of the two forms)
    host_text = (ROOT / "include" / "glrt_host.h").read_text()
    assert re.search(r"\bint glrt_adaptive_select_moments\(const float \*moments, int width, int rows, float threshold, int min_samples, uint8_t \*mask_out, "
                     r"float \*err_out\);", host_text)


def test_libraries_export_the_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in HOST_CALLS:
        assert hasattr(H, name), name


def test_bindings_carry_the_calls():
    from glrt_amd import device, host
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    assert callable(getattr(device.Device, "render_adaptive_moments", None))
    assert callable(device.adaptive_select_moments) and callable(host.adaptive_select_moments)
    for name in device.EXPORTS:
        assert hasattr(device.lib(), name), name


def test_stats_and_abi_version_are_what_they_were(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "glrtx.h"\nint main(void) { printf("%zu %zu %d", sizeof(glrtx_stats), sizeof(glrtx_adaptive), GLRTX_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [168, 8, 10]
    assert C.sizeof(device.Stats) == 168 and C.sizeof(device.Adaptive) == 8


def test_the_luminance_floor_is_the_h_forms_constant():
    """One constant on the device (kAdaptLumFloor, defined once, used by both selection kernels); the host statement's and the numpy statement's equal it."""
    kern = (PKG / "csrc" / "pt_kernel.hip.h").read_text()
    m = re.findall(r"constexpr float kAdaptLumFloor = ([0-9.e+-]+)f;", kern)
    assert len(m) == 1
    assert np.float32(float(m[0])).view(np.uint32) == np.float32(amm.LUM_FLOOR).view(np.uint32)
    var = (PKG / "csrc" / "variance.hip.h").read_text()
    assert "mu1 + kAdaptLumFloor" in var and "constexpr float kAdaptLumFloor" not in var
    host = (PKG / "host" / "variance.cpp").read_text()
    h = re.findall(r"constexpr float kAdaptLumFloor = ([0-9.e+-]+)f;", host)
    assert len(h) == 1 and np.float32(float(h[0])).view(np.uint32) == np.float32(amm.LUM_FLOOR).view(np.uint32)


def test_null_and_size_refusals():
    from glrt_amd import device, host
    L = device.lib()
    z = np.ones((3, 5, 4), np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    mask = np.zeros(1, np.uint8)
    mp = mask.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.glrtx_render_adaptive_moments(None, None, None, 0, None) == -1
    assert L.glrtx_debug_adaptive_select_moments(None, 5, 3, 0.0, 2, mp, None, None, None) == -1
    assert L.glrtx_debug_adaptive_select_moments(p, 5, 3, 0.0, 2, None, None, None, None) == -1
    assert L.glrtx_debug_adaptive_select_moments(p, 0, 3, 0.0, 2, mp, None, None, None) == -1
    assert L.glrtx_debug_adaptive_select_moments(p, 5, 70000, 0.0, 2, mp, None, None, None) == -1
    H = host.lib()
    assert H.glrt_adaptive_select_moments(None, 5, 3, 0.0, 2, mp, None) != 0
    assert H.glrt_adaptive_select_moments(p, 5, 3, 0.0, 2, None, None) != 0
    assert H.glrt_adaptive_select_moments(p, 0, 3, 0.0, 2, mp, None) != 0
    assert H.glrt_adaptive_select_moments(p, 5, 70000, 0.0, 2, mp, None) != 0
    assert H.glrt_adaptive_select_moments(p, 5, 3, 0.0, 2, mp, None) == 0  # (err_out may be NULL)


def test_the_kernels_spill_nothing_and_use_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the rows of the selection kernel and of the masked fold (vgpr agpr sgpr vspill sspill scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("glrtx::adaptive_moments::")]
    assert sorted(row[0] for row in rows) == ["glrtx::adaptive_moments::accumulate_kernel", "glrtx::adaptive_moments::select_kernel"], r.stdout
    for row in rows:
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in row[1:8])
        assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0 and agpr == 0, row
