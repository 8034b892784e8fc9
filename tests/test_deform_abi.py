"""Deforming's calls (include/glrtx.h "Deforming", include/glrt_host.h) without a GPU: the headers declare them and carry the contract's key lines, both libraries
export them, the Python bindings carry them, the ABI version and the stats record are what they were, the refusals that need no device are refusals, and the
new kernels spill nothing, use no scratch memory and no LDS, and keep the skinning kernel's occupancy."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

import deform_math as dm
from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_upload_morph_targets": r"glrtx_ctx \*ctx, const float \*deltas, int n_targets, size_t n_vert",
    "glrtx_pose_morph": r"glrtx_ctx \*ctx, const float \*matrices, int n_bones, const float \*morph_weights, int n_targets",
    "glrtx_pose_dualquat": r"glrtx_ctx \*ctx, const float \*dualquats, int n_bones, const float \*morph_weights, int n_targets",
    "glrtx_debug_deform": r"const float \*rest, size_t n_vert, const int32_t \*bones4, const float \*weights4, const float \*bone_data, int n_bones, int mode,"
                          r"\s+const float \*deltas, const float \*morph_weights, int n_targets, float \*vert_out",
    "glrtx_debug_deform_burst": r"glrtx_ctx \*ctx, int reps, float \*ms_per_launch",
}


def test_headers_declare_the_calls():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text and "#define GLRTX_MAX_MORPH_TARGETS 64" in text
    assert text.index("---- Posing") < text.index("---- Deforming") < text.index("---- Groups")
    for line in ("a target is active iff |w| >= 2^-126", "Inactive targets are not read at all", "p[i] = p[i] + w_k * dpos_k[i]", "n[i] = n[i] + w_k * dnormal_k[i]",
                 "Morphing runs before skinning", "{r.x, r.y, r.z, r.w, d.x, d.y, d.z, d.w}", "dot4(a, b) = ((a.w b.w + a.z b.z) + a.y b.y) + a.x b.x",
                 "s_k = h < 0 ? -w_k : w_k", "a NaN h keeps w_k", "l = sqrt(dot4(R, R))", "l > 0 ? x / l : x",
                 "L00 = 1 - 2 (yy + zz)", "L01 = 2 (xy - wz)", "L02 = 2 (xz + wy)", "L10 = 2 (xy + wz)", "L11 = 1 - 2 (xx + zz)", "L12 = 2 (yz - wx)",
                 "L20 = 2 (xz - wy)", "L21 = 2 (yz + wx)", "L22 = 1 - 2 (xx + yy)", "t.x = 2 (((R.w D.x - D.w R.x) + R.y D.z) - R.z D.y)"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    assert re.search(r"\bint glrt_deform_vertices\(const float \*rest_vert, size_t n_vert, const int32_t \*bones4, const float \*weights4, const float \*bone_data, "
                     r"int n_bones, int mode,\s+const float \*deltas, const float \*morph_weights, int n_targets, float \*vert_out\);", host_h)
    assert "void glrt_dualquat_from_matrix(const float m[12], float dq[8]);" in host_h and "#define GLRT_MAX_MORPH_TARGETS 64" in host_h


def test_the_header_rotation_is_the_quaternions_rotation():
    """The nine entries and the translation as the header writes them, evaluated in float64 on a random unit dual quaternion: the rotation matrix of r, and t."""
    text = (ROOT / "include" / "glrtx.h").read_text()
    rng = np.random.default_rng(9)
    r = rng.standard_normal(4)
    r /= np.linalg.norm(r)
    t = rng.standard_normal(3)
    x, y, z, w = r
    v = dict(xx=x * x, yy=y * y, zz=z * z, xy=x * y, xz=x * z, yz=y * z, wx=w * x, wy=w * y, wz=w * z)
    L = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            m = re.search(rf"L{i}{j} = (1 - )?2 \((\w\w) ([+-]) (\w\w)\)", text)
            inner = v[m.group(2)] + (v[m.group(4)] if m.group(3) == "+" else -v[m.group(4)])
            L[i, j] = 1 - 2 * inner if m.group(1) else 2 * inner
    K = np.array([[0, -z, y], [z, 0, -x], [-y, x, 0]])
    assert np.allclose(L, np.eye(3) + 2 * w * K + 2 * K @ K, atol=1e-12)
    assert np.allclose(L @ L.T, np.eye(3), atol=1e-12) and np.isclose(np.linalg.det(L), 1)
    q = dm.dualquat_matrix(np.zeros((1, 4), np.int32), np.array([[1, 0, 0, 0]], np.float32),
                           np.concatenate([r, 0.5 * np.array([w * t[0] + t[1] * z - t[2] * y, w * t[1] + t[2] * x - t[0] * z, w * t[2] + t[0] * y - t[1] * x,
                                                                -(t @ r[:3])])]).astype(np.float32)[None])[0]
    assert np.allclose(q[:, :3], L, atol=1e-6) and np.allclose(q[:, 3], t, atol=1e-6)


def test_libraries_export_the_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    assert hasattr(H, "glrt_deform_vertices") and hasattr(H, "glrt_dualquat_from_matrix")


def test_bindings_carry_the_calls():
    from glrt_amd import device, host, rig
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    for m in ("upload_morph_targets", "pose_morph", "pose_dualquat", "deform_burst_ms"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_deform) and callable(host.deform_vertices) and callable(rig.dualquat) and callable(rig.identity_dualquats)
    assert C.sizeof(device.Stats) == 168
    assert rig.identity_dualquats(2).tolist() == [[0, 0, 0, 1, 0, 0, 0, 0]] * 2
    assert rig.dualquat(rig.identity_pose(3)).tolist() == rig.identity_dualquats(3).tolist()


def test_refusals_before_any_device_work():
    """glrtx_debug_deform checks its arguments before it touches a device (so this runs without one); the context calls refuse a NULL context."""
    from glrt_amd import device
    rest, bones, weights, mats, deltas, mw = dm.hostile_case(10, 3, 0, 3, 1)
    for bad in (np.where(bones == 2, 3, bones), np.where(bones == 0, -1, bones)):
        with pytest.raises(device.GlrtxError) as e:
            device.debug_deform(rest, bad, weights, mats, 0, deltas, mw)
        assert e.value.code == -1 and "bone" in str(e.value)
    for v in (np.nan, np.inf, -np.inf):
        w2 = mw.copy(); w2[2] = v
        with pytest.raises(device.GlrtxError) as e:
            device.debug_deform(rest, bones, weights, mats, 0, deltas, w2)
        assert e.value.code == -1 and "morph weight" in str(e.value)
    L = device.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = bones.ctypes.data_as(C.POINTER(C.c_int32))
    out = np.zeros_like(rest)
    big = np.zeros(65, np.float32)
    call = L.glrtx_debug_deform
    assert call(None, 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, None, fp(weights), fp(mats), 3, 0, fp(deltas), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, None, fp(mats), 3, 0, fp(deltas), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), None, 3, 0, fp(deltas), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, None, fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), None, 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(mw), 3, None) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 0, 0, fp(deltas), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 65537, 0, fp(deltas), fp(mw), 3, fp(out)) == -1
    for mode in (-1, 2):
        assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, mode, fp(deltas), fp(mw), 3, fp(out)) == -1
        assert b"mode" in L.glrtx_last_error(None)
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(big), 65, fp(out)) == -1
    assert b"65 morph targets" in L.glrtx_last_error(None)
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, fp(deltas), fp(mw), -1, fp(out)) == -1
    assert L.glrtx_debug_deform_burst(None, 1, C.byref(C.c_float())) == -1
    assert L.glrtx_pose_morph(None, fp(mats), 3, fp(mw), 3) == -1 and L.glrtx_pose_dualquat(None, fp(mats), 3, fp(mw), 3) == -1
    assert L.glrtx_upload_morph_targets(None, fp(deltas), 3, 10) == -1


def _waves(vgpr):
    """Waves a SIMD of gfx950 holds at that many vector registers a lane: 512 registers, allocated in eights, at most 8 waves."""
    return min(8, 512 // (8 * ((vgpr + 7) // 8)))


def test_the_kernels_spill_nothing_and_keep_the_occupancy():
    """tools/isa_report.py on the built libglrtx.so (vgpr agpr sgpr vspill sspill scratch lds).  skin_kernel has 67 VGPRs, 7 waves a SIMD; deform_kernel<false>
    has 67 (7 waves) and deform_kernel<true> 61 (8 waves).  The skinning kernel's row is still the only one with its prefix."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    skin = [ln.split() for ln in lines if ln.startswith("glrtx::skin::skin_kernel")]
    assert len(skin) == 1, r.stdout
    floor = _waves(int(skin[0][1]))
    assert floor >= 7
    for name in ("glrtx::skin::deform_kernel<false>", "glrtx::skin::deform_kernel<true>"):
        rows = [ln[len(name):].split() for ln in lines if ln.startswith(name)]
        assert len(rows) == 1, (name, r.stdout)
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in rows[0][0:7])
        assert vspill == 0 and sspill == 0 and scratch == 0 and lds == 0 and agpr == 0, (name, rows[0])
        assert _waves(vgpr) >= floor, (name, vgpr, floor)
