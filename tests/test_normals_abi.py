"""The normal-rebuild calls (include/glrtx.h "Rebuilding normals"; include/glrt_host.h) without a GPU: the headers declare them, the chunk size and the flag, and
carry the contract's key lines; both libraries export them and the Python bindings carry them; the ABI version and the stats record are what they were; a C file
that includes both headers compiles; without a device every call fails cleanly through glrtx_last_error; the four kernels spill nothing and use no scratch
memory and no LDS."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

import normals_cases as nc
from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_upload_normal_topology": r"glrtx_ctx \*ctx, const float \*rest_vert, size_t n_vert, const float \*tri, size_t n_tri, unsigned flags",
    "glrtx_update_positions": r"glrtx_ctx \*ctx, const float \*pos, size_t n_vert",
    "glrtx_update_positions_device": r"glrtx_ctx \*ctx, const void \*dev_pos, size_t n_vert",
    "glrtx_set_pose_normals": r"glrtx_ctx \*ctx, int enable",
    "glrtx_debug_rebuild_normals": r"const float \*vert_in, size_t n_vert, const float \*tri, size_t n_tri, const uint32_t \*class_of_vertex, const uint8_t \*flip,"
                                   r"\s+float \*vert_out",
    "glrtx_debug_normals_burst": r"glrtx_ctx \*ctx, int reps, float \*ms_per_launch",
}
HOST_CALLS = {
    "glrt_normal_topology": r"const float \*rest_vert, size_t n_vert, const float \*tri, size_t n_tri, unsigned flags, uint32_t \*class_of_vertex_out, "
                            r"uint8_t \*flip_out,\s+size_t \*n_classes_out",
    "glrt_rebuild_normals": r"float \*vert_inout, size_t n_vert, const float \*tri, size_t n_tri, const uint32_t \*class_of_vertex, const uint8_t \*flip",
    "glrt_positions_to_vertices": r"const float \*rest_vert, const float \*pos, size_t n_vert, float \*vert_out",
}


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text and "#define GLRTX_NORMAL_CHUNK 256u" in text and "#define GLRTX_NORMALS_WELD_POSITIONS 1u" in text
    assert text.index("---- Deforming") < text.index("---- Rebuilding normals") < text.index("---- Groups")
    for line in ("equal as 32-bit patterns; +0 and -0", "only the three position words are compared", "Class ids ascend with each class's smallest member",
                 "each once, in ascending triangle index", "FLIPPED iff, in the rest pose, dot(f, m) < 0", "m = (n0 + n1) + n2", "A NaN or a zero does not flip",
                 "e1 = p[i1] - p[i0]  and  e2 = p[i2] - p[i0]", "f.x = e1.y e2.z - e1.z e2.y    f.y = e1.z e2.x - e1.x e2.z    f.z = e1.x e2.y - e1.y e2.x",
                 "the three sign bits are inverted", "in chunks of GLRTX_NORMAL_CHUNK = 256 entries", "c = f_first, then c = c + f_next",
                 "s = c_0, then s = s + c_k", "l = sqrt(dot(s, s))", "If l == 0 the normal words in place are KEPT", "n = s / l, three IEEE quotients",
                 "no word is both read and written", "16 n_tri + 4 n_vert +", "4 (n_classes + 1) + 4 entries bytes",
                 "glrtx_upload_scene\n *                     forgets the topology and the switch", "exactly glrtx_update_vertices_device's path",
                 "A class with l == 0 keeps its posed normal", "Enabling without a topology is GLRTX_EINVAL"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name, args in HOST_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", host_h), name
    assert "#define GLRT_NORMAL_CHUNK 256u" in host_h and "#define GLRT_NORMALS_WELD_POSITIONS 1u" in host_h


def test_libraries_export_the_calls_and_bindings_carry_them():
    from glrt_amd import device, host
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in HOST_CALLS:
        assert hasattr(H, name), name
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for name in ("upload_normal_topology", "update_positions", "set_pose_normals", "normals_burst_ms"):
        assert callable(getattr(device.Device, name, None)), name
    assert callable(device.debug_rebuild_normals) and callable(host.normal_topology) and callable(host.rebuild_normals) and callable(host.positions_to_vertices)
    assert host.NORMAL_CHUNK == 256 and host.NORMALS_WELD_POSITIONS == 1
    assert C.sizeof(device.Stats) == 168


def test_a_c_file_including_both_headers_compiles(tmp_path):
    src = tmp_path / "both.c"
    src.write_text('#include <stdio.h>\n#include "glrtx.h"\n#include "glrt_host.h"\n'
                   "int main(void) {\n"
                   "    int (*a)(glrtx_ctx *, const float *, size_t, const float *, size_t, unsigned) = glrtx_upload_normal_topology;\n"
                   "    int (*b)(float *, size_t, const float *, size_t, const uint32_t *, const uint8_t *) = glrt_rebuild_normals;\n"
                   '    printf("%d %u %u %u %u %zu\\n", GLRTX_ABI_VERSION, GLRTX_NORMAL_CHUNK, GLRTX_NORMALS_WELD_POSITIONS, GLRT_NORMAL_CHUNK,\n'
                   "           GLRT_NORMALS_WELD_POSITIONS, sizeof(glrtx_stats));\n"
                   "    return a && b ? 0 : 1;\n}\n")
    exe = tmp_path / "both"
    lib = PKG / "lib"
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", f"-I{ROOT / 'include'}", str(src), "-o", str(exe), f"-L{lib}", "-lglrtx", "-lglrt_host",
                        f"-Wl,-rpath,{lib}"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.split() == ["10", "256", "1", "256", "1", "168"], (r.stdout, r.stderr)


def test_without_a_context_every_call_fails_cleanly():
    """The context calls refuse a NULL context; the debug hook checks its arguments before it touches a device, and with valid arguments either runs (a GPU is
    there) or reports the device's error through glrtx_last_error."""
    from glrt_amd import device, host
    L = device.lib()
    _, rest, tri, moved, _ = nc.cases()[1]
    cls, flip, _ = host.normal_topology(rest, tri)
    n, nt = rest.shape[0], tri.shape[0]
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    pc, pf = cls.ctypes.data_as(C.POINTER(C.c_uint32)), flip.ctypes.data_as(C.POINTER(C.c_uint8))
    ms = C.c_float(0)
    assert L.glrtx_upload_normal_topology(None, fp(rest), n, fp(tri), nt, 0) == -1
    assert L.glrtx_update_positions(None, fp(rest), n) == -1 and L.glrtx_update_positions_device(None, None, n) == -1
    assert L.glrtx_set_pose_normals(None, 1) == -1 and L.glrtx_debug_normals_burst(None, 2, C.byref(ms)) == -1
    out = np.zeros_like(moved)
    call = L.glrtx_debug_rebuild_normals
    assert call(None, n, fp(tri), nt, pc, pf, fp(out)) == -1 and b"NULL" in L.glrtx_last_error(None)
    assert call(fp(moved), n, None, nt, pc, pf, fp(out)) == -1
    assert call(fp(moved), n, fp(tri), nt, None, pf, fp(out)) == -1
    assert call(fp(moved), n, fp(tri), nt, pc, None, fp(out)) == -1
    assert call(fp(moved), n, fp(tri), nt, pc, pf, None) == -1
    bad = cls.copy(); bad[2] = n
    with pytest.raises(device.GlrtxError) as e:
        device.debug_rebuild_normals(moved, tri, bad, flip)
    assert e.value.code == -1 and f"vertex 2: class id {n}" in str(e.value)
    for value in (float(n), -1.0, 1.5, np.nan):
        t = tri.copy(); t[1, 0] = value
        with pytest.raises(device.GlrtxError) as e:
            device.debug_rebuild_normals(moved, t, cls, flip)
        assert e.value.code == -1 and "triangle 1, corner 0: vertex index" in str(e.value)
    assert call(fp(moved), n, fp(tri), 2 ** 31, pc, pf, fp(out)) == -1 and b"2^31" in L.glrtx_last_error(None)
    assert not out.any()
    rc = call(fp(moved), n, fp(tri), nt, pc, pf, fp(out))
    if rc == 0:
        assert (out.view(np.uint32) == host.rebuild_normals(moved, tri, cls, flip).view(np.uint32)).all()
    else:
        assert rc == -2 and b"glrtx_debug_rebuild_normals" in L.glrtx_last_error(None), L.glrtx_last_error(None)


def test_the_kernels_spill_nothing():
    """tools/isa_report.py on the built libglrtx.so (vgpr agpr sgpr vspill sspill scratch lds): no spills, no scratch memory, no LDS, eight waves a SIMD."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for name in ("positions_kernel", "face_kernel", "class_kernel", "vertex_kernel"):
        rows = [ln.split() for ln in lines if ln.startswith(f"glrtx::normals::{name}")]
        assert len(rows) == 1, (name, r.stdout)
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in rows[0][1:8])
        assert (agpr, vspill, sspill, scratch, lds) == (0, 0, 0, 0, 0) and vgpr <= 64, (name, rows[0])
