"""Variance guidance (include/glrtx.h "Variance guidance", include/glrt_host.h) without a GPU: the headers declare the calls, both libraries export them, the
Python bindings carry them, the ABI version and the sizes of the existing structures are what they were, the new configuration structure has the C layout,
the refusals that need no device are refusals, and the new kernels spill nothing and use no scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = ["glrtx_track_moments", "glrtx_render_moments", "glrtx_read_moments", "glrtx_denoise_variance", "glrtx_debug_denoise_variance",
                "glrtx_debug_reproject_moments", "glrtx_debug_reproject_motion_moments"]
HOST_CALLS = ["glrt_fold_moments", "glrt_variance_estimate", "glrt_denoise_variance", "glrt_reproject_moments", "glrt_reproject_motion_moments"]


def test_headers_declare_the_calls_and_keep_the_abi_version():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert "#define GLRTX_ABI_VERSION 10" in text
    for name in DEVICE_CALLS:
        assert re.search(rf"\bint {name}\(", text), name
    assert re.search(r"typedef struct glrtx_denoise_var_cfg \{\s*int\s+iterations;[^}]*float\s+sigma_lum;[^}]*float\s+sigma_normal;[^}]*float\s+sigma_depth;[^}]*"
                     r"int\s+demodulate;[^}]*\} glrtx_denoise_var_cfg;", text)
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
    for m in ("track_moments", "render_moments", "read_moments", "denoise_variance"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_denoise_variance) and callable(host.variance_estimate) and callable(host.denoise_variance) and callable(host.fold_moments)
    assert callable(device.debug_reproject_moments) and callable(device.debug_reproject_motion_moments)
    assert callable(host.reproject_moments) and callable(host.reproject_motion_moments)
    d, c = host.DENOISE_VAR_DEFAULTS, device.denoise_var_cfg()
    assert (c.iterations, c.sigma_lum, c.demodulate) == (d["iterations"], np.float32(d["sigma_lum"]), int(d["demodulate"]))
    assert c.sigma_normal == np.float32(d["sigma_normal"]) and c.sigma_depth == np.float32(d["sigma_depth"])
    c = device.denoise_var_cfg(iterations=2, sigma_lum=0.5)
    assert (c.iterations, c.sigma_lum, c.sigma_depth) == (2, 0.5, np.float32(d["sigma_depth"]))


def test_existing_structures_keep_their_sizes(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    f = ["iterations", "sigma_lum", "sigma_normal", "sigma_depth", "demodulate"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %d", sizeof(glrtx_denoise_cfg), sizeof(glrtx_reproject_cfg), sizeof(glrtx_stats), sizeof(glrtx_denoise_var_cfg), GLRTX_ABI_VERSION);\n'
                   + "".join(f'  printf(" %zu", offsetof(glrtx_denoise_var_cfg, {k}));\n' for k in f) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[:5] == [20, 12, 168, 20, 10]
    assert got[:4] == [C.sizeof(device.DenoiseCfg), C.sizeof(device.ReprojectCfg), C.sizeof(device.Stats), C.sizeof(device.DenoiseVarCfg)]
    assert got[5:] == [getattr(device.DenoiseVarCfg, k).offset for k in f]


BAD_CFGS = [dict(iterations=0), dict(iterations=7), dict(sigma_lum=0.0), dict(sigma_lum=float("nan")), dict(sigma_lum=float("inf")), dict(sigma_normal=-1.0),
            dict(sigma_depth=float("nan")), dict(sigma_depth=float("inf"))]


@pytest.mark.parametrize("bad", BAD_CFGS, ids=[f"{k}={v}" for b in BAD_CFGS for k, v in b.items()])
def test_bad_configurations_are_refused_before_any_device_work(bad):
    from glrt_amd import device, host
    z = np.ones((3, 5, 4), np.float32)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_denoise_variance(z, z, z, z, **bad)
    assert e.value.code == -1
    with pytest.raises(RuntimeError):
        host.denoise_variance(z, z, z, z, **bad)


def test_null_and_size_refusals():
    from glrt_amd import device
    L = device.lib()
    z = np.ones((3, 5, 4), np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    cfg = device.denoise_var_cfg()
    assert L.glrtx_debug_denoise_variance(p, p, p, p, 0, 3, C.byref(cfg), p, None) == -1
    assert L.glrtx_debug_denoise_variance(p, p, p, p, 5, 70000, C.byref(cfg), p, None) == -1
    assert L.glrtx_debug_denoise_variance(p, None, p, p, 5, 3, C.byref(cfg), p, None) == -1
    assert L.glrtx_debug_denoise_variance(p, p, p, p, 5, 3, None, p, None) == -1
    assert L.glrtx_debug_denoise_variance(p, p, p, p, 5, 3, C.byref(cfg), None, None) == -1
    assert L.glrtx_track_moments(None, 1) == -1 and L.glrtx_render_moments(None, None, None, 0) == -1
    assert L.glrtx_read_moments(None, None, 0) == -1 and L.glrtx_denoise_variance(None, C.byref(cfg)) == -1


def test_the_kernels_spill_nothing_and_use_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the rows of the variance pass, the fold and the six filter instantiations (vgpr agpr sgpr vspill sspill
    scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if "denoise_atrous_var" in ln or ln.startswith("glrtx::variance::")]
    assert len(rows) == 8, r.stdout
    for row in rows:
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in row[-7:])  # (a template's name holds a space)
        assert vspill == 0 and sspill == 0 and scratch == 0, row
