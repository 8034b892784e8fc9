"""Posing's calls (include/glrtx.h "Posing", include/glrt_host.h) without a GPU: the headers declare them, both libraries export them, the Python bindings carry
them, the ABI version is what it was, the refusals that need no device are refusals, and the new kernel spills nothing and uses no scratch memory."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

import skin_math as sm
from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_upload_rig": r"glrtx_ctx \*ctx, const float \*rest_vert, size_t n_vert, const int32_t \*bones4, const float \*weights4, int n_bones",
    "glrtx_pose": r"glrtx_ctx \*ctx, const float \*matrices, int n_bones",
    "glrtx_debug_skin_burst": r"glrtx_ctx \*ctx, int reps, float \*ms_per_launch",
    "glrtx_debug_skin": r"const float \*rest, size_t n_vert, const int32_t \*bones4, const float \*weights4, const float \*matrices, int n_bones, float \*vert_out",
}


def test_headers_declare_the_calls():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text
    assert "---- Posing" in text
    for entry in ("C00 = L11 L22 - L12 L21", "C01 = L12 L20 - L10 L22", "C02 = L10 L21 - L11 L20", "C10 = L21 L02 - L22 L01", "C11 = L22 L00 - L20 L02",
                  "C12 = L20 L01 - L21 L00", "C20 = L01 L12 - L02 L11", "C21 = L02 L10 - L00 L12", "C22 = L00 L11 - L01 L10"):
        assert entry in text, entry  # all nine cofactors are written out
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    assert re.search(r"\bint glrt_skin_vertices\(const float \*rest_vert, size_t n_vert, const int32_t \*bones4, const float \*weights4, const float \*matrices, "
                     r"int n_bones,\s+float \*vert_out\);", host_h)


def test_the_header_cofactors_are_the_cofactor_matrix():
    """The nine entries as the header writes them, evaluated in float64 on a random matrix: det(L) L^-T."""
    text = (ROOT / "include" / "glrtx.h").read_text()
    rng = np.random.default_rng(5)
    L = rng.standard_normal((3, 3))
    Cm = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            m = re.search(rf"C{i}{j} = L(\d)(\d) L(\d)(\d) - L(\d)(\d) L(\d)(\d)", text)
            a = [int(v) for v in m.groups()]
            Cm[i, j] = L[a[0], a[1]] * L[a[2], a[3]] - L[a[4], a[5]] * L[a[6], a[7]]
    assert np.allclose(Cm, np.linalg.det(L) * np.linalg.inv(L).T, rtol=1e-10, atol=1e-12)
    assert np.allclose(sm.cofactor(L[None].astype(np.float32))[0], Cm, rtol=1e-4, atol=1e-5)


def test_libraries_export_the_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    assert hasattr(C.CDLL(str(PKG / "lib" / "libglrt_host.so")), "glrt_skin_vertices")


def test_bindings_carry_the_calls():
    from glrt_amd import device, host, rig
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for m in ("upload_rig", "pose", "skin_burst_ms"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_skin) and callable(host.skin_vertices) and callable(rig.rigid)
    assert C.sizeof(device.Stats) == 168
    b, w = rig.rigid(np.array([3, 0, 2]))
    assert b.tolist() == [[3, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0]] and w.tolist() == [[1, 0, 0, 0]] * 3
    assert rig.identity_pose(2).reshape(2, 3, 4)[1].tolist() == np.eye(3, 4).tolist()


def test_refusals_before_any_device_work():
    """glrtx_debug_skin checks its arguments before it touches a device (so this runs without one); the context calls refuse a NULL context."""
    from glrt_amd import device
    rest, bones, weights, mats = sm.hostile_rig(10, 3, 1)
    for bad in (np.where(bones == 2, 3, bones), np.where(bones == 0, -1, bones)):
        with pytest.raises(device.GlrtxError) as e:
            device.debug_skin(rest, bad, weights, mats)
        assert e.value.code == -1 and "bone" in str(e.value)
    L = device.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = bones.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros_like(rest)
    assert L.glrtx_debug_skin(fp(rest), 10, ip, fp(weights), fp(mats), 0, fp(out)) == -1
    assert L.glrtx_debug_skin(fp(rest), 10, ip, fp(weights), fp(mats), 65537, fp(out)) == -1
    assert L.glrtx_debug_skin(None, 10, ip, fp(weights), fp(mats), 3, fp(out)) == -1
    assert L.glrtx_debug_skin(fp(rest), 10, None, fp(weights), fp(mats), 3, fp(out)) == -1
    assert L.glrtx_debug_skin(fp(rest), 10, ip, None, fp(mats), 3, fp(out)) == -1
    assert L.glrtx_debug_skin(fp(rest), 10, ip, fp(weights), None, 3, fp(out)) == -1
    assert L.glrtx_debug_skin(fp(rest), 10, ip, fp(weights), fp(mats), 3, None) == -1
    assert L.glrtx_debug_skin_burst(None, 1, C.byref(C.c_float())) == -1
    assert L.glrtx_pose(None, fp(mats), 3) == -1 and L.glrtx_upload_rig(None, fp(rest), 10, ip, fp(weights), 3) == -1


def test_the_kernel_spills_nothing_and_uses_no_scratch():
    """tools/isa_report.py on the built libglrtx.so: the skinning kernel's row (vgpr agpr sgpr vspill sspill scratch lds)."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    rows = [ln.split() for ln in r.stdout.splitlines() if ln.startswith("glrtx::skin::skin_kernel")]
    assert len(rows) == 1, r.stdout
    vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in rows[0][1:8])
    assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0 and agpr == 0 and vgpr <= 128, rows[0]
