"""Firefly re-weighting (include/glrtx.h "Firefly re-weighting", include/glrt_host.h) without a GPU: the headers declare the calls, both libraries export
them, the Python bindings carry them, the ABI version and the sizes of the existing structures are what they were, the new configuration structure has the C
layout, the refusals that need no device are refusals, and the two new kernels spill nothing and use no scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = ["glrtx_track_cascades", "glrtx_render_cascades", "glrtx_read_cascades", "glrtx_reweight", "glrtx_debug_fold_cascades", "glrtx_debug_reweight",
                "glrtx_debug_reweight_burst"]
HOST_CALLS = ["glrt_fold_cascades", "glrt_reweight"]


def test_headers_declare_the_calls_and_keep_the_abi_version():
    text = (ROOT / "include" / "glrtx.h").read_text()
    assert "#define GLRTX_ABI_VERSION 10" in text and "Firefly re-weighting" in text
    for name in DEVICE_CALLS:
        assert re.search(rf"\bint {name}\(", text), name
    assert re.search(r"typedef struct glrtx_reweight_cfg \{\s*float\s+kappa;[^}]*\} glrtx_reweight_cfg;", text)
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
    for m in ("track_cascades", "render_cascades", "read_cascades", "reweight"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_fold_cascades) and callable(device.debug_reweight) and callable(host.fold_cascades) and callable(host.reweight)
    assert host.REWEIGHT_DEFAULTS == dict(kappa=4.0, start=1.0)
    assert device.reweight_cfg().kappa == 4.0 and device.reweight_cfg(kappa=0.5).kappa == 0.5 and isinstance(device.reweight_cfg(), device.ReweightCfg)


def test_structure_sizes(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %zu", sizeof(glrtx_reweight_cfg), sizeof(glrtx_denoise_cfg), sizeof(glrtx_reproject_cfg), sizeof(glrtx_stats),\n'
                   '         sizeof(glrtx_denoise_var_cfg), sizeof(glrtx_tonemap_cfg), sizeof(glrtx_bloom_cfg), sizeof(glrtx_params), sizeof(glrtx_adaptive), GLRTX_ABI_VERSION,\n'
                   '         offsetof(glrtx_reweight_cfg, kappa));\n  return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got[0] == 4 == C.sizeof(device.ReweightCfg) and got[10] == 0 == device.ReweightCfg.kappa.offset
    assert got[1:5] == [20, 12, 168, 20] and got[9] == 10
    assert got[1:9] == [C.sizeof(t) for t in (device.DenoiseCfg, device.ReprojectCfg, device.Stats, device.DenoiseVarCfg, device.TonemapCfg, device.BloomCfg,
                                               device.Params, device.Adaptive)]


@pytest.mark.parametrize("kappa", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_kappa_is_refused_before_any_device_work(kappa):
    from glrt_amd import device, host
    z = np.ones((6, 3, 5, 4), np.float32)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_reweight(z, kappa=kappa)
    assert e.value.code == -1 and "kappa" in str(e.value)
    with pytest.raises(RuntimeError):
        host.reweight(z, kappa)


@pytest.mark.parametrize("start", [0.0, float("nan"), float("inf"), 2.0 ** -21, 2.0 ** 21])
def test_bad_start_is_refused_before_any_device_work(start):
    from glrt_amd import device, host
    z = np.ones((6, 3, 5, 4), np.float32)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_fold_cascades(z[0], z, z[:2], start)
    assert e.value.code == -1 and "start" in str(e.value)
    with pytest.raises(RuntimeError):
        host.fold_cascades(z, z[:2], start=start)


def test_null_and_size_refusals():
    from glrt_amd import device
    L = device.lib()
    z = np.ones((6, 3, 5, 4), np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    cfg = device.reweight_cfg()
    assert L.glrtx_debug_reweight(p, 0, 3, C.byref(cfg), p) == -1
    assert L.glrtx_debug_reweight(p, 5, 70000, C.byref(cfg), p) == -1
    assert L.glrtx_debug_reweight(None, 5, 3, C.byref(cfg), p) == -1
    assert L.glrtx_debug_reweight(p, 5, 3, None, p) == -1
    assert L.glrtx_debug_reweight(p, 5, 3, C.byref(cfg), None) == -1
    assert L.glrtx_debug_fold_cascades(p, p, p, 1, 0, 3, 1.0, p, p) == -1
    assert L.glrtx_debug_fold_cascades(p, p, p, 1, 5, 65537, 1.0, p, p) == -1
    assert L.glrtx_debug_fold_cascades(None, p, p, 1, 5, 3, 1.0, p, p) == -1
    assert L.glrtx_debug_fold_cascades(p, None, p, 1, 5, 3, 1.0, p, p) == -1
    assert L.glrtx_debug_fold_cascades(p, p, None, 1, 5, 3, 1.0, p, p) == -1
    assert L.glrtx_debug_fold_cascades(p, p, p, -1, 5, 3, 1.0, p, p) == -1
    assert L.glrtx_track_cascades(None, 1, 1.0) == -1 and L.glrtx_render_cascades(None, None, None, 0) == -1
    assert L.glrtx_read_cascades(None, None, 0) == -1 and L.glrtx_reweight(None, C.byref(cfg)) == -1
    ms = C.c_float()
    assert L.glrtx_debug_reweight_burst(None, C.byref(cfg), 1, C.byref(ms)) == -1


def test_the_kernels_spill_nothing_and_use_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the rows of the fold and of the resolve (vgpr agpr sgpr vspill sspill scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("glrtx::reweight::")]
    assert sorted(row[0] for row in rows) == ["glrtx::reweight::accumulate_cascades_kernel", "glrtx::reweight::reweight_kernel"], r.stdout
    for row in rows:
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in row[-7:])
        assert vspill == 0 and sspill == 0 and scratch == 0, row
        assert lds == (6480 if row[0].endswith("reweight_kernel") else 0), row
