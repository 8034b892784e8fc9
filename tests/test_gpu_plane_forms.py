"""What the C ABI promises about the image planes a context owns (csrc/glrtx.hip), pinned through the raw entry points at 44 x 20 -- a 704-byte row in a
768-byte accumulator pitch, 20 rows that fill neither a 4-row nor an 8-row tile: every read-back honours the caller's pitch and touches nothing beside its rows;
a plane of another shape is refused (or, for the planes that follow the accumulator, zeroed) after a resize; a member that owns no rows copies nothing.
No expected value comes from the code under test: each is a self-consistency check, a text of the library's source, or -- the reads a member without rows
accepts -- what the library did before the planes' bookkeeping was stated once."""
import ctypes as C

import numpy as np
import pytest

from glrt_amd import device, host, scenes

pytestmark = pytest.mark.gpu

W, H = 44, 20
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx(gpu_device):
    scene, params = scenes.config_c1(W, H, max_depth=2, n_samples=1, subdiv=1)
    d = device.Device()
    d.set_variant(2); d.count_rays(False)
    d.upload_scene(scene)
    d.track_motion(True); d.track_moments(True); d.track_cascades(True)
    yield d, params
    d.close()


def _produce(d, params, bloomed=True):
    """Every plane once, one sample, one frame.  reweight and bloom refuse a partitioned context: D is the filter's then, and nothing is bloomed."""
    seeds = [host.frame_seed(0)]
    d.render_adaptive(params, seeds, -1.0)
    d.render_features(params)
    d.denoise()
    d.render_moments(params, seeds)
    d.render_cascades(params, seeds)
    d.exposure_measure()
    if bloomed:
        d.reweight()
    d.tonemap()
    if bloomed:
        d.bloom()


def _reads(d):
    """(name, planes, call(dst addresses, pitch)) of every float read-back; a plane's destination starts rows * pitch behind the one before it."""
    L, h = d.L, d.h
    one = lambda fn: lambda a, pitch: fn(h, a[0], pitch)
    return [("glrtx_read_accum", 1, one(L.glrtx_read_accum)),
            ("glrtx_read_adaptive_half", 1, one(L.glrtx_read_adaptive_half)),
            ("glrtx_read_features", 2, lambda a, pitch: L.glrtx_read_features(h, a[0], a[1], pitch)),
            ("glrtx_read_features_geom", 1, one(L.glrtx_read_features_geom)),
            ("glrtx_read_denoised", 1, one(L.glrtx_read_denoised)),
            ("glrtx_read_moments", 1, one(L.glrtx_read_moments)),
            ("glrtx_read_cascades", 6, one(L.glrtx_read_cascades)),
            ("glrtx_read_tonemapped", 1, one(L.glrtx_read_tonemapped)),
            ("glrtx_read_bloomed", 1, one(L.glrtx_read_bloomed))]


def _resolves(d):
    """(name, call(dst address, pitch)) of the four resolves to bytes."""
    L, h = d.L, d.h
    cfg = device.TonemapCfg.default()
    return [("glrtx_resolve_rgba8", lambda a, pitch: L.glrtx_resolve_rgba8(h, a, pitch, 2.2, 1)),
            ("glrtx_resolve_denoised_rgba8", lambda a, pitch: L.glrtx_resolve_denoised_rgba8(h, a, pitch, 2.2, 1)),
            ("glrtx_resolve_tonemapped_rgba8", lambda a, pitch: L.glrtx_resolve_tonemapped_rgba8(h, a, pitch, C.byref(cfg))),
            ("glrtx_resolve_bloomed_rgba8", lambda a, pitch: L.glrtx_resolve_bloomed_rgba8(h, a, pitch, C.byref(cfg)))]


def _err(d):
    return d.L.glrtx_last_error(d.h).decode()


def _into(call, planes, rows, pitch):
    """call on a sentinel-filled (planes, rows, pitch) byte buffer, plane k at k * rows * pitch.  Returns (rc, buffer)."""
    buf = np.full((planes, max(rows, 1), pitch), SENTINEL, np.uint8)
    rc = call([buf[k].ctypes.data for k in range(planes)], pitch)
    return rc, buf


def _pitched(d, name, call, planes, rows, row_bytes, pad):
    rc, packed = _into(call, planes, rows, row_bytes)
    assert rc == 0, f"{name} at the packed pitch: {_err(d)}"
    rc, wide = _into(call, planes, rows, row_bytes + pad)
    assert rc == 0, f"{name} at a pitch {pad} bytes wider: {_err(d)}"
    print(f"{name}: {planes} plane(s) of {rows} x {row_bytes} bytes")
    assert not (packed.reshape(-1, 4) == SENTINEL).all(-1).any(), f"{name}: the packed read left part of its rows unwritten"
    assert np.array_equal(wide[:, :, :row_bytes], packed), f"{name}: the rows differ between the two pitches"
    assert (wide[:, :, row_bytes:] == SENTINEL).all(), f"{name}: the padding behind a row was written"
    rc, short = _into(call, planes, rows, row_bytes - 1)
    assert rc == -1 and "pitch too small" in _err(d), f"{name} at a pitch one byte short of a row: rc {rc}, '{_err(d)}'"
    assert (short == SENTINEL).all(), f"{name}: a refused read wrote to its destination"


def test_reads_honour_the_destination_pitch(ctx):
    d, params = ctx
    d.set_partition(0, 1, 16); d.resize(W, H)
    _produce(d, params)
    assert d.stats().owned_rows == H
    for name, planes, call in _reads(d):
        # (glrtx_read_cascades takes one address: its six planes lie k * owned_rows * pitch apart, which is how _into lays its buffer out)
        _pitched(d, name, call, planes, H, W * 16, 16)
    for name, call in _resolves(d):
        _pitched(d, name, lambda a, pitch: call(a[0], pitch), 1, H, W * 4, 4)


def test_a_resize_leaves_no_plane_of_the_old_shape(ctx):
    d, params = ctx
    d.set_partition(0, 1, 16); d.resize(W, H)
    _produce(d, params)
    before = d.read_exposure()
    assert before.measurements >= 1
    d.resize(H, W)  # 20 x 44: another width, another pitch, other rows
    refused = {"glrtx_read_denoised": "no feature planes", "glrtx_read_features": "", "glrtx_read_features_geom": "",
               "glrtx_read_tonemapped": "no tone-mapped plane (call glrtx_tonemap first)", "glrtx_read_bloomed": "no bloomed plane (call glrtx_bloom first)"}
    zeros = {"glrtx_read_adaptive_half", "glrtx_read_moments", "glrtx_read_cascades"}
    for name, planes, call in _reads(d):
        rc, buf = _into(call, planes, W, H * 16)
        print(f"{name} after the resize: rc {rc} '{_err(d) if rc else ''}'")
        if name in refused:
            assert rc == -1 and refused[name] in _err(d), f"{name}: rc {rc}, '{_err(d)}'"
            assert (buf == SENTINEL).all(), f"{name}: a refused read wrote to its destination"
        elif name in zeros:
            assert rc == 0, f"{name}: {_err(d)}"
            assert not buf.any(), f"{name}: not zeros of the new shape"
    mask = np.full(64, SENTINEL, np.uint8)
    assert d.L.glrtx_read_tile_mask(d.h, mask.ctypes.data_as(C.POINTER(C.c_uint8))) == -1
    assert "the image changed shape since the last adaptive call" in _err(d)
    assert (mask == SENTINEL).all()
    for call in (d.tonemap, d.bloom):
        with pytest.raises(device.GlrtxError, match="without a denoised image of the current shape"):
            call(source=1)
    after = d.read_exposure()
    assert bytes(after) == bytes(before), "the exposure block has no shape: a resize keeps the measurement"


# the reads a member without rows accepted before the planes' bookkeeping was stated once (observed there, with every plane that such a member can produce)
ACCEPTED_WITHOUT_ROWS = ["glrtx_read_accum", "glrtx_read_adaptive_half", "glrtx_read_features", "glrtx_read_features_geom", "glrtx_read_denoised",
                         "glrtx_read_moments", "glrtx_read_cascades", "glrtx_read_tonemapped"]


def test_a_member_that_owns_nothing_copies_nothing(ctx):
    d, params = ctx
    d.set_partition(0, 1, 16); d.resize(W, H)
    d.set_partition(3, 4, 8)  # three 8-row stripes over four members: the fourth has none
    try:
        assert d.stats().owned_rows == 0
        _produce(d, params, bloomed=False)
        with pytest.raises(device.GlrtxError):
            d.bloom()
        accepted = []
        for name, planes, call in _reads(d):
            rc, buf = _into(call, planes, 1, W * 16)
            print(f"{name} without rows: rc {rc} '{_err(d) if rc else ''}'")
            assert (buf == SENTINEL).all(), f"{name}: wrote to its destination"
            if rc == 0:
                accepted.append(name)
        assert accepted == ACCEPTED_WITHOUT_ROWS
        rc, buf = _into(lambda a, pitch: _resolves(d)[0][1](a[0], pitch), 1, 1, W * 4)
        assert rc == 0, _err(d)
        assert (buf == SENTINEL).all()
    finally:
        d.set_partition(0, 1, 16)
