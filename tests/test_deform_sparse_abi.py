"""The sparse-target calls (include/glrtx.h "Deforming", SPARSE TARGETS; include/glrt_host.h) without a GPU: the headers declare them and the two caps and carry
the contract's key lines, both libraries export them, the Python bindings carry them, the ABI version, the dense cap and the stats record are what they were,
the refusals that need no device are refusals, and the two new kernels spill nothing, use no scratch memory, keep the skinning kernel's occupancy and hold the
weight table, 4 KB, in LDS."""
import ctypes as C
import re
import subprocess
import sys

import numpy as np
import pytest

import deform_sparse_math as ds
from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_upload_morph_targets_sparse": r"glrtx_ctx \*ctx, const uint64_t \*offsets, const uint32_t \*vertex, const float \*deltas, int n_targets, size_t n_vert",
    "glrtx_debug_deform_sparse": r"const float \*rest, size_t n_vert, const int32_t \*bones4, const float \*weights4, const float \*bone_data, int n_bones, int mode,"
                                 r"\s+const uint64_t \*offsets, const uint32_t \*vertex, const float \*deltas, const float \*morph_weights, int n_targets, "
                                 r"float \*vert_out",
}
HOST_CALLS = {
    "glrt_deform_vertices_sparse": r"const float \*rest_vert, size_t n_vert, const int32_t \*bones4, const float \*weights4, const float \*bone_data, int n_bones, "
                                   r"int mode,\s+const uint64_t \*offsets, const uint32_t \*vertex, const float \*deltas, const float \*morph_weights, int n_targets, "
                                   r"float \*vert_out",
    "glrt_morph_sparsify": r"const float \*dense_deltas, int n_targets, size_t n_vert, uint64_t \*offsets, uint32_t \*vertex_out, float \*deltas_out",
}


def test_headers_declare_the_calls_and_carry_the_contract():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert "#define GLRTX_ABI_VERSION 10" in text and "#define GLRTX_MAX_MORPH_TARGETS 64" in text and "#define GLRTX_MAX_SPARSE_MORPH_TARGETS 1024" in text
    assert text.index("---- Deforming") < text.index("SPARSE TARGETS.") < text.index("---- Groups")
    for line in ("offsets[n_targets + 1]  uint64, offsets[0] = 0, non-decreasing; nnz = offsets[n_targets] < 2^31",
                 "vertex[nnz]             uint32, strictly ascending inside a target, each < n_vert",
                 "deltas[nnz x 6]         float {dpos, dnormal}, not checked",
                 "a target is active iff |w| >= 2^-126",
                 "over the entries that list this vertex and belong to an active target, in ascending target index",
                 "p = p + w_k * dpos", "n = n + w_k * dnormal",
                 "keeps its rest p and n untouched: no + 0 is formed",
                 "an entry of an inactive target never enters the arithmetic", "It MAY BE LOADED",
                 "With no active target the result is Posing's, bit for bit",
                 "every target lists every vertex performs the dense form's operation sequence: it equals the dense form bit for bit on any data",
                 "changes the result at most in the sign of a zero",
                 "when no rest position or normal component is a negative zero or a negative denormal (precondition)",
                 "A rounded sum is -0 only if both",
                 "Uploading either", "kind of set replaces the other", "the message names the target and the entry",
                 "4 (n_vert + 1) + 32 nnz bytes"):
        assert line in text, line
    host_h = (ROOT / "include" / "glrt_host.h").read_text()
    for name, args in HOST_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", host_h), name
    assert "#define GLRT_MAX_SPARSE_MORPH_TARGETS 1024" in host_h and "#define GLRT_MAX_MORPH_TARGETS 64" in host_h


def test_libraries_export_the_calls():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    for name in DEVICE_CALLS:
        assert hasattr(L, name), name
    assert L.glrtx_abi_version() == 10
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    for name in HOST_CALLS:
        assert hasattr(H, name), name
    assert hasattr(C.CDLL(str(PKG / "lib" / "libglrt.so")), "glrt_scene_morph_sparse_probe")


def test_bindings_carry_the_calls():
    from glrt_amd import device, host
    assert set(DEVICE_CALLS) <= set(device.EXPORTS)
    assert callable(getattr(device.Device, "upload_morph_targets_sparse", None))
    assert callable(device.debug_deform_sparse) and callable(host.deform_vertices_sparse) and callable(host.morph_sparsify)
    assert C.sizeof(device.Stats) == 168
    o, v, d = host.morph_sparsify(np.zeros((2, 3, 6), np.float32))
    assert o.tolist() == [0, 0, 0] and v.size == 0 and d.shape == (0, 6)


def test_refusals_before_any_device_work():
    """glrtx_debug_deform_sparse checks its arguments before it touches a device (so this runs without one); the context call refuses a NULL context."""
    from glrt_amd import device
    rest, bones, weights, mats, dense, mw = ds.hostile_sparse(10, 3, 0, 3, 1)
    o, v, d, mw = ds.pattern("all", dense, mw, 1)
    for bad in (np.where(bones == 2, 3, bones), np.where(bones == 0, -1, bones)):
        with pytest.raises(device.GlrtxError) as e:
            device.debug_deform_sparse(rest, bad, weights, mats, 0, o, v, d, mw)
        assert e.value.code == -1 and "bone" in str(e.value)
    for bad in (np.nan, np.inf, -np.inf):
        w2 = mw.copy(); w2[2] = bad
        with pytest.raises(device.GlrtxError) as e:
            device.debug_deform_sparse(rest, bones, weights, mats, 0, o, v, d, w2)
        assert e.value.code == -1 and "morph weight" in str(e.value)
    v2 = v.copy(); v2[13] = 10
    with pytest.raises(device.GlrtxError) as e:
        device.debug_deform_sparse(rest, bones, weights, mats, 0, o, v2, d, mw)
    assert e.value.code == -1 and "target 1, entry 3: vertex index 10 of 10" in str(e.value)
    v2 = v.copy(); v2[25] = 4
    with pytest.raises(device.GlrtxError) as e:
        device.debug_deform_sparse(rest, bones, weights, mats, 0, o, v2, d, mw)
    assert "target 2, entry 5: vertex index 4 after 4, not strictly ascending" in str(e.value)
    L = device.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    ip = bones.ctypes.data_as(C.POINTER(C.c_int32))
    po, pv = o.ctypes.data_as(C.POINTER(C.c_uint64)), v.ctypes.data_as(C.POINTER(C.c_uint32))
    out = np.zeros_like(rest)
    call = L.glrtx_debug_deform_sparse
    assert call(None, 10, ip, fp(weights), fp(mats), 3, 0, po, pv, fp(d), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), None, 3, 0, po, pv, fp(d), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, None, pv, fp(d), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, None, fp(d), fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, pv, None, fp(mw), 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, pv, fp(d), None, 3, fp(out)) == -1
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, pv, fp(d), fp(mw), 3, None) == -1
    for mode in (-1, 2):
        assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, mode, po, pv, fp(d), fp(mw), 3, fp(out)) == -1
        assert b"mode" in L.glrtx_last_error(None)
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, pv, fp(d), fp(mw), 1025, fp(out)) == -1
    assert b"1025 sparse morph targets (0 .. 1024)" in L.glrtx_last_error(None)
    assert call(fp(rest), 10, ip, fp(weights), fp(mats), 3, 0, po, pv, fp(d), fp(mw), -1, fp(out)) == -1
    assert L.glrtx_upload_morph_targets_sparse(None, po, pv, fp(d), 3, 10) == -1
    assert not out.any()


def _waves(vgpr):
    """Waves a SIMD of gfx950 holds at that many vector registers a lane: 512 registers, allocated in eights, at most 8 waves."""
    return min(8, 512 // (8 * ((vgpr + 7) // 8)))


def test_the_kernels_spill_nothing_and_keep_the_occupancy():
    """tools/isa_report.py on the built libglrtx.so (vgpr agpr sgpr vspill sspill scratch lds).  deform_sparse_kernel<false> has 67 VGPRs (7 waves a SIMD, as
    skin_kernel) and deform_sparse_kernel<true> 61 (8 waves); LDS is the weight table, 1024 floats.  The names do not start with the existing kernels' prefixes."""
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "isa_report.py")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    skin = [ln.split() for ln in lines if ln.startswith("glrtx::skin::skin_kernel")]
    assert len(skin) == 1, r.stdout
    floor = _waves(int(skin[0][1]))
    assert floor >= 7
    assert len([ln for ln in lines if ln.startswith("glrtx::skin::deform_kernel<")]) == 2
    for name in ("glrtx::skin::deform_sparse_kernel<false>", "glrtx::skin::deform_sparse_kernel<true>"):
        rows = [ln[len(name):].split() for ln in lines if ln.startswith(name)]
        assert len(rows) == 1, (name, r.stdout)
        vgpr, agpr, sgpr, vspill, sspill, scratch, lds = (int(v) for v in rows[0][0:7])
        assert vspill == 0 and sspill == 0 and scratch == 0 and agpr == 0, (name, rows[0])
        assert _waves(vgpr) >= floor >= 7, (name, vgpr, floor)
        assert 0 < lds <= 4096 + 256, (name, lds)
