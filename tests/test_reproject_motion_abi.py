"""The motion-aware reprojection's calls (include/glrtx.h "Reprojection across a geometry move", include/glrt_host.h) without a GPU: the headers declare them,
both libraries export them, the Python bindings carry them, the ABI version and glrtx_stats are what they were, the refusals that need no device are refusals,
the new kernels spill no vector register and use no scratch memory, and the kernels without the geometry plane are still there under their names."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_track_motion": r"glrtx_ctx \*ctx, int enable",
    "glrtx_read_features_geom": r"glrtx_ctx \*ctx, float \*geom, size_t pitch_bytes",
    "glrtx_reproject_motion": r"glrtx_ctx \*ctx, const glrtx_params \*cur, const glrtx_reproject_cfg \*cfg",
    "glrtx_debug_reproject_motion": r"const float \*accum, const float \*n0, const float \*a0, const float \*g1, const float \*a1, const float \*vert_prev, size_t n_vert,\s+"
                                    r"const float \*tri, size_t n_tri, const float \*c2w_prev, const float \*s2c_prev, int width, int rows, "
                                    r"const glrtx_reproject_cfg \*cfg,\s+float \*out, int \*carried, int \*hit_pixels",
}
HOST_CALLS = ("glrt_reproject_motion", "glrt_render_features_geom")


def test_headers_declare_the_calls():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
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


def test_bindings_carry_the_calls():
    from glrt_amd import device, host
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for m in ("track_motion", "read_features_geom", "reproject_motion"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_reproject_motion) and callable(host.reproject_motion) and callable(host.render_features_geom)
    assert C.sizeof(device.Stats) == 168 and C.sizeof(device.ReprojectCfg) == 12


BAD_CFGS = [dict(max_history=0), dict(depth_tolerance=0.0), dict(depth_tolerance=float("nan")), dict(depth_tolerance=float("inf")), dict(normal_tolerance=float("nan")),
            dict(normal_tolerance=float("-inf"))]


@pytest.mark.parametrize("bad", BAD_CFGS, ids=[f"{k}={v}" for b in BAD_CFGS for k, v in b.items()])
def test_bad_configurations_are_refused_before_any_device_work(bad):
    from glrt_amd import device, host, scenes
    z = np.ones((3, 5, 4), np.float32)
    _, params = scenes.config_c1(5, 3, max_depth=4, subdiv=1)
    vert, tri = np.zeros((3, 15), np.float32), np.array([[0, 1, 2, 0]], np.float32)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_reproject_motion(z, z, z, z, z, vert, tri, params, **bad)
    assert e.value.code == -1
    with pytest.raises(RuntimeError):
        host.reproject_motion(z, z, z, z, z, vert, tri, params, **bad)


def test_singular_cameras_bad_triangles_null_and_size_refusals():
    from glrt_amd import device, scenes
    _, params = scenes.config_c1(5, 3, max_depth=4, subdiv=1)
    z = np.ones((3, 5, 4), np.float32)
    vert, tri = np.zeros((3, 15), np.float32), np.array([[0, 1, 2, 0]], np.float32)
    for key in ("c2w", "s2c"):
        with pytest.raises(device.GlrtxError) as e:
            device.debug_reproject_motion(z, z, z, z, z, vert, tri, dict(params, **{key: np.zeros(16, np.float32)}))
        assert e.value.code == -1 and "singular" in str(e.value)
    for bad_tri in ([[0, 1, 3, 0]], [[-1, 1, 2, 0]], [[0, float("nan"), 2, 0]]):
        with pytest.raises(device.GlrtxError) as e:
            device.debug_reproject_motion(z, z, z, z, z, vert, np.array(bad_tri, np.float32), params)
        assert e.value.code == -1 and "vertex index" in str(e.value)
    L = device.lib()
    cfg = device.ReprojectCfg.default()
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    m = np.eye(4, dtype=np.float32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))
    v, t = vert.ctypes.data_as(C.POINTER(C.c_float)), tri.ctypes.data_as(C.POINTER(C.c_float))
    geo = [v, 3, t, 1]
    assert L.glrtx_debug_reproject_motion(p, p, p, p, p, *geo, m, m, 0, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject_motion(p, p, p, p, p, *geo, m, m, 5, 70000, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject_motion(p, p, p, None, p, *geo, m, m, 5, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject_motion(p, p, p, p, p, None, 3, t, 1, m, m, 5, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject_motion(p, p, p, p, p, *geo, m, None, 5, 3, C.byref(cfg), p, None, None) == -1
    assert L.glrtx_debug_reproject_motion(p, p, p, p, p, *geo, m, m, 5, 3, None, p, None, None) == -1
    assert L.glrtx_debug_reproject_motion(p, p, p, p, p, *geo, m, m, 5, 3, C.byref(cfg), None, None, None) == -1
    assert L.glrtx_reproject_motion(None, None, C.byref(cfg)) == -1 and L.glrtx_track_motion(None, 1) == -1 and L.glrtx_read_features_geom(None, None, 0) == -1


def test_the_new_kernels_spill_no_vector_register_and_use_no_scratch():
    """tools/isa_report.py on the built libglrtx.so (vgpr agpr sgpr vspill sspill scratch lds).  The vine kernel keeps its scalar registers in lanes of a
    vector register as features_vine does (sspill, no memory); the others spill nothing."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = {}
    for ln in r.stdout.splitlines():
        m = re.match(r"(glrtx::.*?)((?:\s+\d+){7})\s*$", ln)
        if m:
            rows[m.group(1)] = [int(v) for v in m.group(2).split()]
    for name, lds_free in (("glrtx::motion::reproject_motion_kernel", True), ("glrtx::motion::snapshot_kernel", True), ("glrtx::features::features_vine_geom", True),
                           ("glrtx::features::features_tree<true, glrtx::features::GeomArgs>", False),
                           ("glrtx::features::features_tree<false, glrtx::features::GeomArgs>", False)):
        assert name in rows, (name, sorted(rows))
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = rows[name]
        assert vspill == 0 and scratch == 0 and agpr == 0 and vgpr <= 64, (name, rows[name])
        if lds_free:
            assert lds == 0, (name, rows[name])
        if "vine" not in name:
            assert sspill == 0, (name, rows[name])
    for name in ("glrtx::features::features_vine", "glrtx::features::features_tree<true, glrtx::features::Args>",
                 "glrtx::features::features_tree<false, glrtx::features::Args>", "glrtx::reproject::reproject_kernel"):
        assert name in rows, name
    # (lane spills of scalars, like the kernel it extends)
    assert rows["glrtx::features::features_vine_geom"][4] <= rows["glrtx::features::features_vine"][4] + 8


def test_shared_sources():
    """One statement of each piece: the kernel calls surf_tri and reproject.hip.h's helpers, the CPU statement uses host/reproject_setup.h, the geometry kernels
    use the feature pass's own store."""
    k = (PKG / "csrc" / "reproject_motion.hip.h").read_text()
    assert "surf_tri(prev, h)" in k and "using reproject::pos_finite;" in k and '#include "reproject.hip.h"' in k
    assert "glrt_detail::reproject_setup(" in (PKG / "host" / "reproject_motion.cpp").read_text()
    f = (PKG / "csrc" / "features.hip.h").read_text()
    assert "store(static_cast<const Args &>(q), id, h);" in f


def test_each_persistent_loop_is_stated_once():
    """The feature pass's tree loop and the megakernel's regeneration and bounce loop each live in one kernel template (their instantiations' instructions are
    pinned, tools/isa_diff.py): no second copy of either text, and no shared body behind wrappers."""
    f = (PKG / "csrc" / "features.hip.h").read_text()
    assert "tree_body" not in f
    loops = f.split("for (;;)")[1:]
    assert sum("trav_step<true, COMPACT>" in part for part in loops) == 1 and f.count("bool fin = trav_step<true, COMPACT>") == 1
    k = (PKG / "csrc" / "pt_kernel.hip.h").read_text()
    assert k.count("atomicAdd(work_counter, (unsigned)kChunk)") == 1
    assert "pt_render_persistent_" not in k
