"""The denoiser's calls (include/glrtx.h "Denoising", include/glrt_host.h) without a GPU: the headers declare them, both libraries export them, the
Python bindings carry them, the configuration structure has the C layout, the ABI version and glrtx_stats are what they were, and the refusals that
need no device are refusals."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG, ROOT

DEVICE_CALLS = {
    "glrtx_render_features": r"glrtx_ctx \*ctx, const glrtx_params \*params",
    "glrtx_read_features": r"glrtx_ctx \*ctx, float \*normal_depth, float \*albedo_id, size_t pitch_bytes",
    "glrtx_denoise": r"glrtx_ctx \*ctx, const glrtx_denoise_cfg \*cfg",
    "glrtx_read_denoised": r"glrtx_ctx \*ctx, float \*dst_rgba, size_t dst_pitch_bytes",
    "glrtx_resolve_denoised_rgba8": r"glrtx_ctx \*ctx, uint8_t \*dst, size_t dst_pitch_bytes, float gamma, int flip_y",
    "glrtx_debug_denoise": r"const float \*accum, const float \*normal_depth, const float \*albedo_id, int width, int rows, const glrtx_denoise_cfg \*cfg, float \*out",
}
HOST_CALLS = ["glrt_render_features", "glrt_denoise_atrous"]


def test_headers_declare_the_calls():
    text = (ROOT / "include" / "glrtx.h").read_text()
    for name, args in DEVICE_CALLS.items():
        assert re.search(rf"\bint {name}\({args}\);", text), name
    assert re.search(r"typedef struct glrtx_denoise_cfg \{\s*int\s+iterations;[^}]*float\s+sigma_color;[^}]*float\s+sigma_normal;[^}]*float\s+sigma_depth;[^}]*"
                     r"int\s+demodulate;[^}]*\} glrtx_denoise_cfg;", text)
    assert "#define GLRTX_ABI_VERSION 10" in text
    host = (ROOT / "include" / "glrt_host.h").read_text()
    for name in HOST_CALLS:
        assert re.search(rf"\bint {name}\(", host), name


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
    for m in ("render_features", "read_features", "denoise", "read_denoised", "resolve_denoised_rgba8"):
        assert callable(getattr(device.Device, m, None)), m
    assert callable(device.debug_denoise) and callable(host.render_features) and callable(host.denoise_atrous)
    assert C.sizeof(device.Stats) == 168
    d = host.DENOISE_DEFAULTS
    c = device.denoise_cfg()
    assert (c.iterations, c.demodulate) == (d["iterations"], int(d["demodulate"])) and 1 <= c.iterations <= 6
    assert c.sigma_color == np.float32(d["sigma_color"]) and c.sigma_normal == np.float32(d["sigma_normal"]) and c.sigma_depth == np.float32(d["sigma_depth"])
    text = (PKG / "host" / "window.h").read_text()  # the facade's defaults (glrt_main --denoise) are the binding's
    m = re.search(r"glrtx_denoise_cfg denoiseCfg_ = \{(\d+), ([0-9.e+-]+)f, ([0-9.e+-]+)f, ([0-9.e+-]+)f, (\d)\};", text)
    assert m and [float(v) for v in m.groups()] == [float(d[k]) for k in ("iterations", "sigma_color", "sigma_normal", "sigma_depth", "demodulate")]


def test_ctypes_cfg_matches_the_c_layout(tmp_path):
    from glrt_amd import device
    src = tmp_path / "sizes.c"
    f = ["iterations", "sigma_color", "sigma_normal", "sigma_depth", "demodulate"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "glrtx.h"\nint main(void) {\n  printf("%zu %zu", sizeof(glrtx_stats), sizeof(glrtx_denoise_cfg));\n'
                   + "".join(f'  printf(" %zu", offsetof(glrtx_denoise_cfg, {k}));\n' for k in f) + "  return 0;\n}\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-I", str(ROOT / "include"), "-o", str(exe), str(src)], check=True, capture_output=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(device.Stats), C.sizeof(device.DenoiseCfg)] + [getattr(device.DenoiseCfg, k).offset for k in f]
    assert got[0] == 168


BAD_CFGS = [dict(iterations=0), dict(iterations=7), dict(iterations=-1), dict(sigma_color=0.0), dict(sigma_color=-1.0), dict(sigma_normal=float("nan")),
            dict(sigma_depth=float("inf")), dict(sigma_normal=0.0), dict(sigma_depth=-0.5)]


@pytest.mark.parametrize("bad", BAD_CFGS, ids=[f"{k}={v}" for b in BAD_CFGS for k, v in b.items()])
def test_bad_configurations_are_refused_before_any_device_work(bad):
    """glrtx_debug_denoise checks its configuration before it touches a device (so this runs without one); glrt_denoise_atrous refuses the same."""
    from glrt_amd import device, host
    z = np.ones((3, 5, 4), np.float32)
    with pytest.raises(device.GlrtxError) as e:
        device.debug_denoise(z, z, z, **bad)
    assert e.value.code == -1
    with pytest.raises(RuntimeError):
        host.denoise_atrous(z, z, z, **bad)


def test_null_and_size_refusals():
    from glrt_amd import device
    L = device.lib()
    cfg = device.denoise_cfg()
    z = np.ones((2, 2, 4), np.float32)
    p = z.ctypes.data_as(C.POINTER(C.c_float))
    assert L.glrtx_debug_denoise(p, p, p, 0, 2, C.byref(cfg), p) == -1
    assert L.glrtx_debug_denoise(p, p, p, 2, 70000, C.byref(cfg), p) == -1
    assert L.glrtx_debug_denoise(None, p, p, 2, 2, C.byref(cfg), p) == -1
    assert L.glrtx_debug_denoise(p, p, p, 2, 2, None, p) == -1
    for fn, args in ((L.glrtx_render_features, (None, None)), (L.glrtx_denoise, (None, C.byref(cfg))), (L.glrtx_read_denoised, (None, None, 0)),
                     (L.glrtx_read_features, (None, None, None, 0)), (L.glrtx_resolve_denoised_rgba8, (None, None, 0, 2.2, 1))):
        assert fn(*args) == -1


def test_reserved_id_and_floor_are_the_kernels():
    import denoise_math as dm
    text = (PKG / "csrc" / "denoise.hip.h").read_text()
    assert "constexpr int kNoPixel = INT32_MIN;" in text and int(dm.NO_PIXEL) == -2 ** 31
    m = re.search(r"constexpr float kAlbedoFloor = ([0-9.e+-]+)f;", text)
    assert m and float(dm.ALBEDO_FLOOR) == float(np.float32(m.group(1)))
