"""The reprojection's calls (include/glrtx.h "Reprojection", include/glrt_host.h) without a GPU: the headers declare them, both libraries export them, the
Python bindings carry them, the configuration structure has the C layout, the ABI version and glrtx_stats are what they were, the refusals that need no
device are refusals, and the new kernel spills nothing and uses no scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_reproject": r"glrtx_ctx \*ctx, const glrtx_params \*cur, const glrtx_reproject_cfg \*cfg",
    "glrtx_reproject_last": r"glrtx_ctx \*ctx, int \*carried, int \*hit_pixels",
    "glrtx_debug_reproject": r"const float \*accum, const float \*n0, const float \*a0, const float \*n1, const float \*a1, const float \*c2w_prev, "
                             r"const float \*s2c_prev,\s+const float \*c2w_cur, const float \*s2c_cur, int width, int rows, const glrtx_reproject_cfg \*cfg, "
                             r"float \*out, int \*carried, int \*hit_pixels",
}


def test_headers_declare_the_calls():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert re.search(r"typedef struct glrtx_reproject_cfg \{\s*int\s+max_history;[^}]*float\s+depth_tolerance;[^}]*float\s+normal_tolerance;[^}]*\} glrtx_reproject_cfg;", text)
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert re.search(r"\bint glrt_reproject\(", (ROOT / "include" / "glrt_host.h").read_text())


def test_libraries_export_the_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    assert hasattr(C.CDLL(str(PKG / "lib" / "libglrt_host.so")), "glrt_reproject")


def test_bindings_carry_the_calls_and_the_defaults():
    from glrt_amd import device, host
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for m in ("reproject", "reproject_last"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_reproject) and callable(host.reproject)
    assert C.sizeof(device.Stats) == 168
    d, c = host.REPROJECT_DEFAULTS, device.ReprojectCfg.default()
    assert c.max_history == d["max_history"] >= 1 and c.depth_tolerance == np.float32(d["depth_tolerance"]) > 0 and c.normal_tolerance == np.float32(d["normal_tolerance"])
    c = device.ReprojectCfg.default(max_history=3, normal_tolerance=0.5)
    assert (c.max_history, c.normal_tolerance, c.depth_tolerance) == (3, 0.5, np.float32(d["depth_tolerance"]))


def test_ctypes_cfg_matches_the_c_layout(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    f = ["max_history", "depth_tolerance", "normal_tolerance"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\nint main(void) {\n  printf("%zu %zu %d", sizeof(glrtx_stats), sizeof(glrtx_reproject_cfg), GLRTX_ABI_VERSION);\n'
                   + "".join(f'  printf(" %zu", offsetof(glrtx_reproject_cfg, {k}));\n' for k in f) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(device.Stats), C.sizeof(device.ReprojectCfg), 10] + [getattr(device.ReprojectCfg, k).offset for k in f]
    assert got[0] == 168 and got[1] == 12


BAD_CFGS = [dict(max_history=0), dict(max_history=-1), dict(depth_tolerance=0.0), dict(depth_tolerance=-0.5), dict(depth_tolerance=float("nan")),
            dict(depth_tolerance=float("inf")), dict(normal_tolerance=float("nan")), dict(normal_tolerance=float("inf")), dict(normal_tolerance=float("-inf"))]


@pytest.mark.parametrize("bad", BAD_CFGS, ids=[f"{k}={v}" for b in BAD_CFGS for k, v in b.items()])
def test_bad_configurations_are_refused_before_any_device_work(bad):
    """glrtx_debug_reproject checks its configuration and the previous camera before it touches a device (so this runs without one); glrt_reproject refuses the same."""
    from glrt_amd import device, host, scenes
    z = np.ones((3, 5, 4), np.float32)
    _, params = scenes.config_c1(5, 3, max_depth=4, subdiv=1)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_reproject(z, z, z, z, z, params, params, **bad)
    assert e.value.code == -1
    with pytest.raises(RuntimeError):
        host.reproject(z, z, z, z, z, params, params, **bad)


def test_singular_cameras_null_and_size_refusals():
    from glrt_amd import device, scenes
    _, params = scenes.config_c1(5, 3, max_depth=4, subdiv=1)
    z = np.ones((3, 5, 4), np.float32)
    for key in ("c2w", "s2c"):
        with pytest.raises(device.GlrtxError) as e:
            device.debug_reproject(z, z, z, z, z, dict(params, **{key: np.zeros(16, np.float32)}), params)
        assert e.value.code == -1 and "singular" in str(e.value)
    L = device.lib()
    cfg = device.ReprojectCfg.default()
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    m = np.eye(4, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
    arrays, mats = [p] * 5, [m] * 4
    assert L.glrtx_debug_reproject(*arrays, *mats, 0, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject(*arrays, *mats, 5, 70000, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject(None, p, p, p, p, *mats, 5, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject(*arrays, m, None, m, m, 5, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject(*arrays, *mats, 5, 3, None, p, None, None) == -1
    assert L.glrtx_debug_reproject(*arrays, *mats, 5, 3, C.byref(cfg), None, None, None) == -1
    assert L.glrtx_reproject(None, None, C.byref(cfg)) == -1 and L.glrtx_reproject_last(None, None, None) == -1


def test_the_kernel_spills_nothing_and_uses_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the reprojection kernel's row (vgpr agpr sgpr vspill sspill scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("glrtx::reproject::reproject_kernel")]
    assert len(rows) == 1, r.stdout
    vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in rows[0][1:8])
    assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0 and agpr == 0 and vgpr <= 64, rows[0]


def test_one_matrix_inverse_and_one_centre_ray():
    """The shared sources: both libraries invert with host/mat4_inverse.h, the kernel calls features::centre_ray, the CPU statement host/centre_ray.h's."""
    hip = (PKG / "csrc" / "glrtx.hip").read_text()
    assert '#include "../host/reproject_setup.h"' in hip and "glrt_detail::reproject_setup(" in hip
    assert '#include "mat4_inverse.h"' in (PKG / "host" / "reproject_setup.h").read_text() and "glrt_detail::mat4_inverse(m, out)" in (PKG / "host" / "camera.cpp").read_text()
    assert "features::centre_ray(" in (PKG / "csrc" / "reproject.hip.h").read_text()
    assert "glrt_detail::centre_ray(" in (PKG / "host" / "reproject.cpp").read_text() and "using glrt_detail::centre_ray;" in (PKG / "host" / "features.cpp").read_text()
