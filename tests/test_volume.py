"""The volume branch (GLRTX_EXT_VOLUME) without a GPU: the stored llvmpipe sweeps against the numpy statement of the device's
sequences (tests/volume_math.py), the fixtures' own contract, the VOL grid files, and the C ABI's argument errors."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN, PKG, assert_bit_equal
import volume_math as vm

VOLUME = GOLDEN / "volume"
FIXTURES = sorted(p.stem for p in VOLUME.glob("vol_*.npz"))


@pytest.fixture(scope="module")
def sweep():
    return np.load(VOLUME / "math_volume.npz")


@pytest.mark.parametrize("fn", ["exp", "log", "acos"])
def test_llvmpipe_transcendentals_match_the_restated_sequence(sweep, fn):
    x = sweep["x"]
    assert x.size >= 65536
    assert_bit_equal(getattr(vm, f"lp_{fn}")(x), sweep[fn], fn)


def test_the_restatement_is_not_libm(sweep):
    """What the sweep pins is llvmpipe's own polynomial, not the correctly rounded function: they differ on many inputs."""
    x = sweep["x"].astype(np.float64)
    with np.errstate(all="ignore"):
        libm_exp = np.exp(x).astype(np.float32)
    finite = np.isfinite(libm_exp) & (libm_exp > 1e-30)
    assert (libm_exp[finite].view(np.uint32) != sweep["exp"][finite].view(np.uint32)).mean() > 0.2


def test_blackbody_matches_the_references_function_on_llvmpipe(sweep):
    assert_bit_equal(vm.blackbody(sweep["temp"]), sweep["blackbody"], "blackBody")
    bb = sweep["blackbody"]
    assert (bb[sweep["temp"] < 0.05] == 0).all()  # exp() overflows: blackBody is 0, not NaN
    assert np.isfinite(bb).all() and bb.max() > 1.0


def test_lookup_is_the_magnification_filter_with_repeat(sweep):
    pos = sweep["pos"]
    got = vm.lookup(sweep["grid"], sweep["bbox"][:3], sweep["bbox"][3:], pos)
    assert_bit_equal(got, sweep["lookup"], "textureLod(..., 0.0)")
    lo, hi = sweep["bbox"][:3], sweep["bbox"][3:]
    uvw = (pos - lo) / (hi - lo)
    assert ((uvw < 0) | (uvw > 1)).any(axis=1).sum() > 1000  # the sweep covers the wrap


def test_lookup_returns_texel_values_at_texel_centres(sweep):
    """The first 256 sweep positions lie at texel centres (i + 0.5) / n -- in float32, so a weight may come out a few ulps off 0."""
    g = sweep["grid"]
    assert g.shape == (5, 7, 12)  # (nz, ny, nx): x fastest
    i = np.arange(256)
    np.testing.assert_allclose(sweep["lookup"][:256], g[i % 5, i % 7, i % 12], rtol=0, atol=1e-5)


def test_fixture_set_is_complete():
    want = {"vol_const_switch", "vol_const_lod", "vol_fire16", "vol_noise_12x7x5", "vol_cold", "vol_hot", "vol_open",
            "vol_through_conductor", "vol_frames3"}
    assert want <= set(FIXTURES)


@pytest.mark.parametrize("name", FIXTURES)
def test_fixture_contract(name):
    z = np.load(VOLUME / f"{name}.npz")
    cls = str(z["shader_class"])
    assert cls in ("switch", "lod")
    d, t = z["density"], z["temperature"]
    assert d.shape == t.shape and d.ndim == 3 and d.dtype == np.float32
    if cls == "switch":  # only where nearest and linear filtering agree exactly
        assert (d == d.flat[0]).all() and (t == t.flat[0]).all()
    bb = z["bbox"]
    assert (bb[3:] - bb[:3] != 0).all()
    assert np.isfinite(z["out_rgb"]).all()
    assert (z["mat"].reshape(-1, 6, 3)[:, 0, 0] == 5).any()  # a media material


def test_fixtures_cover_the_returns_and_the_clamp():
    def rgb(n):
        z = np.load(VOLUME / f"{n}.npz")
        return z["out_rgb"], int(z["scalars"][3])
    o, _ = rgb("vol_open")
    assert ((o[..., 0] >= 1) & (o[..., 1] == 0) & (o[..., 2] >= 1)).sum() > 100  # magenta returns
    h, spp = rgb("vol_hot")
    assert (h >= 100.0 * 2).any() and (h <= 100.0 * spp).all()  # min(L, 1.0e2) reached by more than one sample of a pixel
    c, _ = rgb("vol_cold")
    f, _ = rgb("vol_fire16")
    assert c[..., 0].mean() < f[..., 0].mean()


# ---------------------------------------------------------------------------------------------------------------- VOL files
def test_vol_round_trip(tmp_path):
    from glrt_amd import scenes
    rng = np.random.default_rng(1)
    g = rng.random((5, 7, 12, 2), dtype=np.float32)
    p = tmp_path / "g.vol"
    scenes.write_vol(p, g, (-1, -2, -3), (1, 2, 3))
    raw = p.read_bytes()
    assert raw[:4] == b"VOL\x03" and len(raw) == 48 + g.nbytes
    back, lo, hi = scenes.read_vol(p)
    assert_bit_equal(back, g, "grid")
    assert lo == (-1, -2, -3) and hi == (1, 2, 3)
    # what the reference uploads: the first nx*ny*nz floats (GL_RED), u_densityMax over every channel
    first, mx = scenes.volume_from_file_grid(back)
    assert first.shape == (5, 7, 12) and mx == float(g.max())
    assert_bit_equal(first.reshape(-1), g.reshape(-1)[: 5 * 7 * 12], "first channel run")


@pytest.mark.parametrize("what", ["magic", "version", "encoding", "short"])
def test_vol_reader_rejects(tmp_path, what):
    from glrt_amd import scenes
    p = tmp_path / "g.vol"
    scenes.write_vol(p, np.zeros((2, 2, 2), np.float32))
    raw = bytearray(p.read_bytes())
    if what == "magic":
        raw[:3] = b"VOX"
    elif what == "version":
        raw[3] = 2
    elif what == "encoding":
        raw[4:8] = np.array([2], "<i4").tobytes()  # 2 = 16-bit floats: not supported
    else:
        raw = raw[:-4]
    p.write_bytes(bytes(raw))
    with pytest.raises(ValueError, match={"magic": "not a VOL", "version": "version", "encoding": "encoding", "short": "size"}[what]):
        scenes.read_vol(p)


# ---------------------------------------------------------------------------------------------------------------- C ABI, no device
@pytest.fixture(scope="module")
def L():
    L = C.CDLL(str(PKG / "lib" / "libglrtx.so"))
    L.glrtx_last_error.restype = C.c_char_p
    L.glrtx_last_error.argtypes = [C.c_void_p]
    fp = C.POINTER(C.c_float)
    L.glrtx_upload_volume.argtypes = [C.c_void_p, fp, fp, C.c_int, C.c_int, C.c_int, fp, fp, C.c_float]
    L.glrtx_debug_volume_math.argtypes = [C.c_int, fp, C.c_size_t, fp]
    L.glrtx_debug_volume_lookup.argtypes = [fp, C.c_int, C.c_int, C.c_int, fp, fp, fp, C.c_size_t, fp]
    return L


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def test_abi_volume_constants():
    from glrt_amd import device
    hdr = (PKG.parent / "include" / "glrtx.h").read_text()
    assert "#define GLRTX_EXT_VOLUME 4" in hdr and device.EXT_VOLUME == 4
    assert "#define GLRTX_ABI_VERSION 10" in hdr


def test_abi_upload_volume_null_context(L):
    g = np.ones((2, 2, 2), np.float32)
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    assert L.glrtx_upload_volume(None, _fp(g), _fp(g), 2, 2, 2, _fp(lo), _fp(hi), 1.0) == -1
    assert b"NULL context" in L.glrtx_last_error(None)


@pytest.mark.parametrize("case", ["negative", "zero_extent", "nan_extent", "too_large"])
def test_abi_lookup_argument_errors(L, case):
    """The lookup export shares glrtx_upload_volume's checks; both fail before they touch a device."""
    g = np.ones(8, np.float32)
    lo, hi = np.zeros(3, np.float32), np.ones(3, np.float32)
    pos, out = np.zeros(3, np.float32), np.zeros(1, np.float32)
    dims = (2, 2, 2)
    if case == "negative":
        dims, msg = (2, -1, 2), b"negative grid dimension"
    elif case == "zero_extent":
        hi[1] = lo[1]
        msg = b"zero or non-finite extent on axis y"
    elif case == "nan_extent":
        hi[2] = np.nan
        msg = b"zero or non-finite extent on axis z"
    else:
        dims, msg = (1024, 1024, 1024), b"exceed 2^29"
    assert L.glrtx_debug_volume_lookup(_fp(g), *dims, _fp(lo), _fp(hi), _fp(pos), 1, _fp(out)) == -1
    assert msg in L.glrtx_last_error(None)


def test_abi_math_unknown_op(L):
    x = np.zeros(4, np.float32)
    assert L.glrtx_debug_volume_math(7, _fp(x), 4, _fp(x)) == -1
    assert b"unknown op" in L.glrtx_last_error(None)


def test_python_binding_exports_the_volume_calls():
    from glrt_amd import device
    for n in ("glrtx_upload_volume", "glrtx_group_upload_volume", "glrtx_debug_volume_math", "glrtx_debug_volume_lookup"):
        assert n in device.EXPORTS
    assert hasattr(device.Device, "upload_volume") and hasattr(device.Group, "upload_volume")
