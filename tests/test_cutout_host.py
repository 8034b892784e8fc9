"""The CPU statements of the alpha cutouts (include/glrtx.h "Cutouts"): glrt_texture_channel equals the numpy statement (tests/cutout_math.py) bit for bit on
the texture tests' batch, for all four channels, and its channels 0 .. 2 are glrt_texture_lookup's columns; glrt_render_features_geom_cutout with every
record -1 is glrt_render_features_geom, and with records it makes the documented decision -- checked pixel by pixel against the numpy statement on the plane
G it writes; hostile inputs (NaN and infinite coordinates, NaN texels, cutoffs of +0 and -0) give the documented decision; and the statements run clean under
the address and undefined-behaviour sanitizers in a stand-alone program."""
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import cutout_math as cm
import texture_cases
import texture_math as tm
from conftest import PKG, ROOT
from glrt_amd import host, scenes

F = np.float32
N = 6


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _same_words(a, b):
    return (_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))


@pytest.mark.parametrize("channel", [0, 1, 2, 3])
def test_channel_equals_the_numpy_statement_and_the_lookups_columns(channel):
    tex, which, st = texture_cases.batch()
    got = host.texture_channel(tex, which, channel, st)
    want = cm.channel(tex, which, channel, st)
    bad = ~_same_words(got, want)
    assert not bad.any(), f"channel {channel}: {int(bad.sum())} of {bad.size} lookups differ; first {np.flatnonzero(bad)[0]}: {got[bad][0]!r} vs {want[bad][0]!r}"
    if channel < 3:
        assert np.array_equal(_bits(got), _bits(host.texture_lookup(tex, which, st)[:, channel]))


def test_alpha_is_the_fourth_float_or_byte_over_255_never_srgb():
    a8 = np.arange(256, dtype=np.uint8).reshape(16, 16)
    rgba8 = np.stack([a8[::-1], a8.T, a8[:, ::-1], a8], -1)
    st = np.stack([(np.arange(256) % 16 + 0.5) / 16, (np.arange(256) // 16 + 0.5) / 16], 1).astype(F)  # every texel's centre
    for fmt in ("rgba8_unorm", "rgba8_srgb"):
        got = host.texture_channel([(rgba8, fmt, "clamp", "nearest")], np.zeros(256, np.int32), 3, st)
        assert np.array_equal(_bits(got), _bits(np.arange(256, dtype=F) / F(255.0))), fmt
    red = host.texture_channel([(rgba8, "rgba8_srgb", "clamp", "nearest")], np.zeros(256, np.int32), 0, st)
    assert np.array_equal(_bits(red), _bits(tm.SRGB[a8[::-1].reshape(-1)]))  # ... while colour channels are decoded
    f = np.random.default_rng(3).uniform(-2, 2, (16, 16, 4)).astype(F)
    got = host.texture_channel([(f, "rgba32f", "clamp", "nearest")], np.zeros(256, np.int32), 3, st)
    assert np.array_equal(_bits(got), _bits(f[..., 3].reshape(-1)))
    three = host.texture_channel([(f[..., :3], "rgba32f", "clamp", "nearest")], np.zeros(256, np.int32), 3, st)  # pack_textures' alpha of a 3-channel array
    assert (three == 1.0).all()


def test_channel_refuses_what_the_header_says():
    tex = [(np.zeros((2, 2, 4), F), "rgba32f", "repeat", "nearest")]
    for which, channel in (([1], 0), ([-1], 0), ([0], 4), ([0], -1)):
        with pytest.raises(RuntimeError, match="glrt_texture_channel failed: -2"):
            host.texture_channel(tex, which, channel, [[0.5, 0.5]])
    assert host.texture_channel(tex, [], 0, np.zeros((0, 2), F)).size == 0


def _free_wall(seed=11):
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-1.0, 2.0, (2 * N * N, 3, 2)).astype(F)
    scene, params, wall = scenes.config_cutout_wall(n=N, uv=uv)
    rgba = np.random.default_rng(seed + 1).uniform(0.0, 1.0, (4, 5, 4)).astype(F)
    return scene, params, wall, rgba


def _records(scene, wall, **kw):
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    t = np.full(n_mat, -1, np.int32)
    t[wall["material"]] = 0
    return host.cutouts(n_mat, texture=t, **kw), np.full(n_mat, -1, np.int32)


def _walk_expected(scene, params, wall, tex, cut):
    """What the rule says of every pixel, from the statements it is made of: the uncut search's hit, then -- while that hit lies on the wall and the numpy
    statement rejects it -- the search again from just behind it.  Only the decision at the FIRST candidate is used: `kept` pixels must keep their triangle and
    barycentrics, the others must not."""
    n0, a0, g0 = host.render_features_geom(scene, params)
    t0 = g0[..., 0].view(np.int32)
    on_wall = np.isin(t0, np.asarray(list(wall["tri"])))
    st, ok, _ = tm.hit_st(scene["vert"], scene["tri"], g0.reshape(-1, 4))
    value = cm.channel(tex, np.zeros(st.shape[0], np.int32), int(cut["channel"][wall["material"]]), st).reshape(t0.shape)
    kept = ~on_wall | cm.accepts(value, cut["cutoff"][wall["material"]])
    return (n0, a0, g0), on_wall, kept


def test_features_with_every_record_minus_one_equal_the_geom_statement():
    scene, params, wall, rgba = _free_wall()
    tex = [(rgba, "rgba32f", "repeat", "bilinear")]
    n_mat = scene["mat"].reshape(-1, 18).shape[0]
    none = np.full(n_mat, -1, np.int32)
    got = host.render_features_geom_cutout(scene, params, tex, none, host.cutouts(n_mat))
    want = host.render_features_geom(scene, params)
    for g, w, name in zip(got, want, "NAG"):
        assert np.array_equal(_bits(g), _bits(w)), f"plane {name}"


def test_features_make_the_documented_decision_at_the_first_candidate():
    scene, params, wall, rgba = _free_wall()
    tex = [(rgba, "rgba32f", "repeat", "bilinear")]
    cut, bind = _records(scene, wall, channel=3, cutoff=0.5)
    (n0, a0, g0), on_wall, kept = _walk_expected(scene, params, wall, tex, cut)
    n, a, g = host.render_features_geom_cutout(scene, params, tex, bind, cut)
    share = (~kept)[on_wall].mean()
    assert 0.2 <= share <= 0.8, share  # the texture cuts inside triangles, and not everything
    # a pixel whose first candidate is accepted keeps its three planes; one whose first candidate is rejected shows another triangle, or none
    for got, want, name in ((n, n0, "N"), (a, a0, "A"), (g, g0, "G")):
        assert np.array_equal(_bits(got)[kept], _bits(want)[kept]), f"plane {name} where the first candidate is accepted"
    assert (g[..., 0].view(np.int32)[~kept] != g0[..., 0].view(np.int32)[~kept]).all()
    # whatever is hit in the end is a hit the rule accepts
    st, ok, ti = tm.hit_st(scene["vert"], scene["tri"], g.reshape(-1, 4))
    hit_wall = ok & np.isin(ti, np.asarray(list(wall["tri"])))
    value = cm.channel(tex, np.zeros(st.shape[0], np.int32), 3, st)
    assert hit_wall.sum() > 300 and cm.accepts(value[hit_wall], 0.5).all()


@pytest.mark.parametrize("cutoff", [0.0, -0.0])
def test_hostile_inputs_give_the_documented_decision(cutoff):
    """NaN and infinite coordinates are 0 ("Textures"), a NaN value rejects, +0 and -0 are one cutoff, and a denormal value is the zero of its sign."""
    nan, inf = F(np.nan), F(np.inf)
    rgba = np.zeros((2, 2, 4), F)
    rgba[0, 0, 3] = 0.0      # the texel every non-finite coordinate reads
    rgba[0, 1, 3] = nan
    rgba[1, 0, 3] = -1e-40   # a negative denormal: -0 >= +-0 accepts
    rgba[1, 1, 3] = -1e-30
    tex = [(rgba, "rgba32f", "clamp", "nearest")]
    st = np.array([[nan, inf], [-inf, nan], [0.25, 0.25], [0.75, 0.25], [0.25, 0.75], [0.75, 0.75]], F)
    value = host.texture_channel(tex, np.zeros(6, np.int32), 3, st)
    assert np.array_equal(_same_words(value, cm.channel(tex, np.zeros(6, np.int32), 3, st)), np.ones(6, bool))
    assert cm.accepts(value, F(cutoff)).tolist() == [True, True, True, False, True, False]
    # the feature statement on a wall whose every corner carries one of those coordinates: a cell is kept iff the rule accepts its value
    cells = np.arange(N * N) % 6
    uv = np.repeat(st[cells], 6, 0).reshape(2 * N * N, 3, 2)
    scene, params, wall = scenes.config_cutout_wall(n=N, uv=uv)
    cut, bind = _records(scene, wall, channel=3, cutoff=cutoff)
    n, a, g = host.render_features_geom_cutout(scene, params, tex, bind, cut)
    n0, a0, g0 = host.render_features_geom(scene, params)
    t, t0 = g[..., 0].view(np.int32), g0[..., 0].view(np.int32)
    first = wall["tri"][0]
    on_wall = np.isin(t0, np.asarray(list(wall["tri"])))
    keep = np.array([True, True, True, False, True, False])[cells[(t0[on_wall] - first) // 2]]
    assert on_wall.sum() > 500 and 0.2 < keep.mean() < 0.8
    assert (t[on_wall][keep] == t0[on_wall][keep]).all() and (t[on_wall][~keep] != t0[on_wall][~keep]).all()
    assert not np.isin(t[on_wall][~keep], np.asarray(list(wall["tri"]))).any()  # (the wall is flat: a ray through a hole meets no other cell of it)


def test_features_refuse_what_the_header_says():
    scene, params, wall, rgba = _free_wall()
    tex = [(rgba, "rgba32f", "repeat", "bilinear")]
    cut, bind = _records(scene, wall)
    t = scene["mat"].reshape(-1, 18)[:, 0].astype(np.int32)
    lamp = int(np.flatnonzero(t == 1)[0])

    def refused(code, **change):
        c = cut.copy()
        for k, (m, v) in change.items():
            c[k][m] = v
        with pytest.raises(RuntimeError, match=f"glrt_render_features_geom_cutout failed: {code}"):
            host.render_features_geom_cutout(scene, params, tex, bind, c)

    w = wall["material"]
    refused(-2, texture=(w, 1))
    refused(-2, texture=(w, -2))
    refused(-2, channel=(w, 4))
    refused(-1, cutoff=(w, np.nan))
    refused(-1, cutoff=(w, np.inf))
    refused(-1, reserved=(w, 1))
    refused(-1, texture=(lamp, 0))


# ---- sanitizers: the statements in a stand-alone program of their own
def test_statements_run_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "the host library's compiler is needed"
    host_dir = PKG / "host"
    exe = tmp_path / "cutout_sanitize"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT / 'include'}",
           f"-I{host_dir}", "-o", str(exe), str(pathlib.Path(__file__).with_name("cutout_sanitize.cpp")), str(host_dir / "features.cpp"), str(host_dir / "query.cpp"),
           str(host_dir / "texture.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "cutout_sanitize ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
