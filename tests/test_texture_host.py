"""The texture lookup's CPU statements (libglrt_host.so: glrt_texture_lookup, glrt_srgb_table, glrt_texture_albedo; include/glrtx.h "Textures") without a GPU:
against the numpy statement (tests/texture_math.py) word for word on the cases of tests/texture_cases.py, the sRGB constants against the float64 formula, the
equal-texel property the equivalence tests on the GPU rely on, the albedo statement on hand-made hit records, and the refusals."""
import numpy as np
import pytest

import texture_cases as tc
import texture_math as tm
from glrt_amd import host, scenes


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_lookup_equals_numpy_word_for_word():
    tex, which, st = tc.batch()
    assert len(tex) == 120 and which.size > 120 * 4096
    got = host.texture_lookup(tex, which, st)
    ref = tm.lookup(tex, which, st)
    bad = (_bits(got) != _bits(ref)).any(1)
    assert not bad.any(), f"{int(bad.sum())} of {bad.size} lookups differ; first: texture {which[bad][0]} {tex[which[bad][0]][1:]} at {st[bad][0].tolist()}: " \
                          f"{got[bad][0].tolist()} vs {ref[bad][0].tolist()}"


def test_every_path_is_taken():
    """The cases reach both ends of every wrap rule: index -1 and index N under bilinear repeat, both clamps, i == N under nearest."""
    for n in (1, 7, 64):
        s = tc.axis_values(n)
        for wrap in (tm.REPEAT, tm.CLAMP):
            a = tm.mul(tm.coord(s, wrap), np.float32(n))
            assert (np.floor(a) == n).any() and (a == 0).any()
            fl = np.floor(tm.sub(a, np.float32(0.5)))
            assert (fl == -1).any() and (fl == n - 1).any()


def test_srgb_table_is_the_formula_rounded_once():
    ref = tm.srgb_formula()
    assert _bits(host.srgb_table()).tolist() == _bits(ref).tolist()
    assert tm.SRGB_BITS.tolist() == _bits(ref).tolist()
    assert ref[0] == 0.0 and ref[255] == 1.0 and np.all(np.diff(ref) > 0)


@pytest.mark.parametrize("fmt", tc.FORMATS)
def test_equal_texels_return_the_texel_exactly(fmt):
    """A bilinear lookup at the shared corner of a 2x2 block of equal texels -- and anywhere between their centres -- returns that texel's words."""
    rng = np.random.default_rng(3)
    n = 4
    cell = rng.uniform(0.05, 0.95, (n, n, 3)).astype(np.float32) if fmt == "rgba32f" else rng.integers(0, 256, (n, n, 3), dtype=np.uint8)
    big = np.repeat(np.repeat(cell, 2, 0), 2, 1)
    words = _bits(tm.decode(cell, tm._CODES[fmt]))
    ij = np.stack(np.meshgrid(np.arange(n), np.arange(n), indexing="ij"), -1).reshape(-1, 2)  # (row j, column i)
    centre = ((ij[:, ::-1] + 0.5) / n).astype(np.float32)
    for wrap in ("repeat", "clamp"):
        for st in (centre, centre + np.float32(0.2 / (2 * n)), centre - np.float32(0.2 / (2 * n))):
            got = host.texture_lookup([(big, fmt, wrap, "bilinear")], np.zeros(len(st), np.int32), st)
            assert _bits(got).tolist() == words[ij[:, 0], ij[:, 1]].tolist(), (fmt, wrap)
        got = host.texture_lookup([(cell, fmt, wrap, "nearest")], np.zeros(len(centre), np.int32), centre)
        assert _bits(got).tolist() == words[ij[:, 0], ij[:, 1]].tolist(), (fmt, wrap)


def _wall():
    rng = np.random.default_rng(11)
    n = 3
    uv = rng.uniform(-1.0, 2.0, (2 * n * n, 3, 2)).astype(np.float32)
    scene, _, wall = scenes.config_textured_wall(n=n, uv=uv)
    tex = [(tc.texels(5, 4, "rgba32f", 1), "rgba32f", "repeat", "bilinear"), (tc.texels(2, 3, "rgba8_srgb", 2), "rgba8_srgb", ("clamp", "repeat"), "nearest")]
    return scene, wall, tex


def test_albedo_statement_on_hand_made_hits():
    scene, wall, tex = _wall()
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    tri = scene["tri"].reshape(-1, 4)
    types = scene["mat"].reshape(-1, 18)[:, 0].astype(int)
    rng = np.random.default_rng(5)
    ids = np.concatenate([np.arange(tri.shape[0]), [-1, -1]]).astype(np.int32)  # every triangle (floor: unbound diffuse, sphere: conductor, lamp: emitter, wall), two misses
    ids = np.tile(ids, 4)
    u = rng.uniform(0, 1, ids.size).astype(np.float32)
    v = (rng.uniform(0, 1, ids.size) * (1 - u)).astype(np.float32)
    hits = np.zeros((ids.size, 4), np.float32)
    hits[:, 0] = ids.view(np.float32)
    hits[:, 1], hits[:, 2] = u, v
    hits[:4, 1:3] = [[0, 0], [1, 0], [0, 1], [0.5, 0.5]]
    for k in (0, 1):
        bind = np.full(n_mat, -1, np.int32)
        bind[wall["material"]] = k
        got = host.texture_albedo(scene, tex, bind, hits)
        ref = tm.albedo(scene, tex, bind, hits)
        assert _bits(got).tolist() == _bits(ref).tolist()
        mid = tri[np.maximum(ids, 0), 3].astype(int)
        assert (got[ids < 0] == 1).all() and (got[(ids >= 0) & (types[mid] != 2)] == 1).all()          # a miss, an emitter, a conductor
        floor = (ids >= 0) & (mid == 0)
        assert floor.any() and (got[floor] == scene["mat"].reshape(-1, 18)[0, 6:9]).all()               # an unbound diffuse material: param0
        on_wall = (ids >= 0) & (mid == wall["material"])
        assert on_wall.any() and not (got[on_wall] == np.float32(0.5)).all(1).any()                    # bound: the texture, not param0
    # hits shaped like a plane
    assert host.texture_albedo(scene, tex, bind, hits.reshape(2, -1, 4)).shape == (2, ids.size // 2, 3)


def test_refusals():
    scene, wall, tex = _wall()
    desc, blob = host.pack_textures(tex)
    assert desc.dtype.itemsize == 32 and blob.size % 16 == 0 and desc["offset"].tolist() == [0, 5 * 4 * 16]
    one = np.zeros(1, np.int32)
    st = np.zeros((1, 2), np.float32)

    def refused(**edit):
        d = desc.copy()
        for k, v in edit.items():
            d[k][0] = v
        with pytest.raises(RuntimeError):
            host.texture_lookup((d, blob), one, st)

    refused(width=0)
    refused(height=16385)
    refused(format=3)
    refused(wrap_s=2)
    refused(wrap_t=-1)
    refused(filter=2)
    refused(offset=8)
    refused(height=5)  # 5 x 5 x 16 bytes from offset 0: past the blob's end
    with pytest.raises(RuntimeError):
        host.texture_lookup((desc, blob[:-16]), one, st)
    with pytest.raises(RuntimeError):
        host.texture_lookup(tex, np.array([2], np.int32), st)
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    bind = np.full(n_mat, -1, np.int32)
    hits = np.zeros((1, 4), np.float32)
    bind[2] = 0  # the lamp is no diffuse material
    with pytest.raises(RuntimeError):
        host.texture_albedo(scene, tex, bind, hits)
    bind[2], bind[wall["material"]] = -1, 2
    with pytest.raises(RuntimeError):
        host.texture_albedo(scene, tex, bind, hits)


def test_add_mesh_without_uv_is_unchanged():
    a = scenes.config_c1(32, 32)[0]
    assert not a["vert"].reshape(-1, 5, 3)[:, 2].any()
    s, _, wall = scenes.config_textured_wall(n=2)
    uv = s["vert"].reshape(-1, 5, 3)[:, 2]
    assert not uv[: wall["vert"].start].any() and (uv[wall["vert"].start:, 2] == 0).all()
    assert sorted(set(map(tuple, uv[wall["vert"].start:, :2].tolist()))) == [(0.25, 0.25), (0.25, 0.75), (0.75, 0.25), (0.75, 0.75)]
