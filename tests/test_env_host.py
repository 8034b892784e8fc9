"""Environment lighting on the CPU (include/glrtx.h "Environment"): the octahedral mapping and its solid-angle factor, the agreement of the host statements
(glrt_env_*, host/environment.cpp) with the numpy statement (tests/env_math.py) bit for bit on hostile maps and directions, the alias tables and the pdf they
realise, the lat-long resampling, and the statements under the address and undefined-behaviour sanitizers in a stand-alone program."""
import functools
import pathlib
import shutil
import subprocess

import numpy as np
import pytest

import env_cases as ec
import env_math as em
from conftest import PKG, ROOT
from glrt_amd import host

F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _cfgs(kw):
    return host.env_cfg(**kw), em.cfg(**kw)


@functools.lru_cache(maxsize=None)
def _case(k):
    """(name, env_map, host cfg, numpy cfg, host weights, numpy weights) of ec.maps()[k], computed once."""
    name, env_map, kw = ec.maps()[k]
    hc, nc = _cfgs(kw)
    return name, env_map, hc, nc, host.env_weights(env_map, hc), em.weights(env_map, nc)


CASES = range(len(ec.maps()))


# ---- mapping and solid angle
def test_round_trip_returns_the_normalised_direction():
    """Direction -> (s, t) -> direction within 4 ulp a component.  The ulp is that of a unit vector's scale, 2^-23: s = px * 0.5 + 0.5 lies in [0, 1] and keeps
    no more of a small component than that, in any fp32 statement of the mapping."""
    d = ec.unit_directions()
    for R in (em.IDENTITY, ec.QUARTER_TURN, ec._rot(7)):
        ok, s, t, n1_fwd = em.dir_to_st(R, d.astype(F))
        assert ok.all()
        back, n1 = em.st_to_dir(R, s, t)
        assert np.abs(n1_fwd - n1).max() < 1e-6
        unit = d.astype(F).astype(np.float64)
        unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        err = np.abs(back.astype(np.float64) - unit).max() / 2.0 ** -23
        print(f"round trip: max error {err:.2f} ulp")
        assert err <= 4.0, err
        assert np.abs(n1.astype(np.float64) - np.abs(unit @ np.asarray(R, np.float64).reshape(3, 3).T).sum(1)).max() < 1e-6


def test_axes_land_on_the_stated_texel_centres_of_a_2x2_map():
    """+y is the centre of the square (where the four texels of a 2 x 2 map meet), -y its corners, +-x the middles of the right / left edge, +-z of the top / bottom
    edge; a direction just inside an upper octant reads that octant's texel of a 2 x 2 map: texel [t > 0.5, s > 0.5]."""
    ok, s, t, _ = em.dir_to_st(em.IDENTITY, ec.axes().astype(F))
    assert ok.all()
    assert np.array_equal(np.stack([s, t], 1), np.array([[1, .5], [0, .5], [.5, .5], [1, 1], [.5, 1], [.5, 0]], F))  # (-y with sgn(0) = +1: the (1, 1) corner)
    arr = np.arange(16, dtype=F).reshape(2, 2, 4)
    for sx in (1, -1):
        for sz in (1, -1):
            d = np.array([[0.3 * sx, 1.0, 0.2 * sz]], F)
            got = host.env_eval((arr, "rgba32f", "nearest"), host.env_cfg(), d)[0, :3]
            assert np.array_equal(got, arr[int(sz > 0), int(sx > 0), :3]), (sx, sz, got)


def test_solid_angle_integrates_to_4pi():
    n = 1024
    c = (np.arange(n) + 0.5) / n
    s, t = np.meshgrid(c, c)
    u, v = 2 * s - 1, 2 * t - 1
    y = 1 - np.abs(u) - np.abs(v)
    x = np.where(y < 0, (1 - np.abs(v)) * np.where(u < 0, -1, 1), u)
    z = np.where(y < 0, (1 - np.abs(u)) * np.where(v < 0, -1, 1), v)
    n1 = (np.abs(x) + np.abs(y) + np.abs(z)) / np.sqrt(x * x + y * y + z * z)
    total = (4 * n1 ** 3).sum() / n ** 2
    assert abs(total - 4 * np.pi) <= 1e-5 * 4 * np.pi, total
    # the fp32 statement's factor is the same function
    _, n1f = em.st_to_dir(em.IDENTITY, s.reshape(-1)[::97].astype(F), t.reshape(-1)[::97].astype(F))
    assert np.abs(n1f - n1.reshape(-1)[::97]).max() < 1e-6


# ---- the statements agree
@pytest.mark.parametrize("k", CASES)
def test_weights_agree(k):
    name, _, _, _, hw, nw = _case(k)
    assert hw.shape == nw.shape
    assert np.array_equal(_bits(hw), _bits(nw)), f"{name}: {int((_bits(hw) != _bits(nw)).sum())} of {hw.size} cell weights differ"
    assert (hw >= 0).all() and np.isfinite(hw).all()


@pytest.mark.parametrize("k", CASES)
def test_alias_tables_agree_word_for_word(k):
    name, _, _, _, hw, _ = _case(k)
    ht, nt = host.env_alias(hw), em.tables(hw)
    for key in ("row_q", "row_alias", "col_q", "col_alias", "cell_p"):
        assert np.array_equal(np.ascontiguousarray(ht[key]).view(np.uint32), np.ascontiguousarray(nt[key]).view(np.uint32)), (name, key)
    g = hw.shape[0]
    assert ((ht["row_alias"] >= 0) & (ht["row_alias"] < g)).all() and ((ht["col_alias"] >= 0) & (ht["col_alias"] < g)).all()


@pytest.mark.parametrize("k", CASES)
def test_sample_and_eval_agree(k):
    name, env_map, hc, nc, hw, _ = _case(k)
    t = em.tables(hw)
    u = ec.uniforms()
    hs, ns = host.env_sample(env_map, hc, u), em.sample(env_map, nc, u, t)
    bad = (_bits(hs) != _bits(ns)).any(1)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} samples differ; first at {u[bad][0].tolist()}: {hs[bad][0].tolist()} vs {ns[bad][0].tolist()}"
    d = ec.directions()
    he, ne = host.env_eval(env_map, hc, d), em.evaluate(env_map, nc, d, t)
    bad = (_bits(he) != _bits(ne)).any(1)
    assert not bad.any(), f"{name}: {int(bad.sum())} of {bad.size} evaluations differ; first at {d[bad][0].tolist()}: {he[bad][0].tolist()} vs {ne[bad][0].tolist()}"
    assert not he[:11].any(), "a direction without an L1 norm has radiance 0 and pdf 0"
    assert np.isfinite(hs).all() and (hs[:, 3] >= 0).all()


# ---- alias tables and pdf
@pytest.mark.parametrize("k", CASES)
def test_tables_realise_the_weights(k):
    name, _, _, _, hw, _ = _case(k)
    t = host.env_alias(hw)
    w = hw.astype(np.float64)
    if w.sum() == 0:
        assert not t["cell_p"].any()
        return
    got = em.realised(t)
    assert np.abs(got - w / w.sum()).max() <= 2.0 ** -22, name
    assert np.abs(t["cell_p"].astype(np.float64) - w / w.sum()).max() <= 2.0 ** -22


@pytest.mark.parametrize("k", CASES)
def test_pdf_integrates_to_one_and_covers_the_radiance(k):
    name, env_map, hc, _, hw, _ = _case(k)
    if not hw.any():
        return
    g, n = hw.shape[0], np.asarray(env_map[0]).shape[0]
    m = 4 * max(g, n)  # a 4x supersampled midpoint grid: every sample lies strictly inside one cell
    while m % g:
        m += 1
    c = ((np.arange(m) + 0.5) / m).astype(F)
    s, t = np.meshgrid(c, c)
    kw = dict(ec.maps()[k][2], light_pick=1.0)
    d, n1 = em.st_to_dir(em.cfg(**kw)["rotation"], s.reshape(-1), t.reshape(-1))
    ev = host.env_eval(env_map, host.env_cfg(**kw), d)
    # the direction's own cell may be a neighbour's at a cell boundary after the round trip; strictly inside it is the cell of (s, t)
    domega = 4.0 * n1.astype(np.float64) ** 3 / m ** 2
    total = (ev[:, 3].astype(np.float64) * domega).sum()
    print(f"{name}: sum of pdf dOmega = {total!r}")
    assert abs(total - 1.0) <= 1e-5, (name, total)
    lit = ev[:, :3].max(1) > 0
    assert (ev[lit, 3] > 0).all(), f"{name}: radiance without pdf at {int((ev[lit, 3] <= 0).sum())} of {int(lit.sum())} lit points"


# ---- lat-long resampling
def test_from_latlong_of_a_constant_image_is_that_constant():
    img = np.broadcast_to(np.array([0.25, 1.5, 3.0], F), (16, 32, 3))
    out = host.env_from_latlong(img, 8)
    assert out.shape == (8, 8, 4) and np.array_equal(out[..., :3], np.broadcast_to(img[0, 0], (8, 8, 3))) and (out[..., 3] == 1).all()


def test_from_latlong_keeps_sky_and_ground_apart():
    sky, ground = np.array([0.2, 0.4, 1.0], F), np.array([0.3, 0.2, 0.1], F)
    img = np.zeros((64, 128, 3), F)
    img[:32], img[32:] = sky, ground
    n = 16
    out = host.env_from_latlong(img, n)
    c = (np.arange(n) + 0.5) / n
    s, t = np.meshgrid(c, c)
    y = 1 - np.abs(2 * s - 1) - np.abs(2 * t - 1)
    up, down = y > 0.1, y < -0.1
    assert up.any() and down.any()
    assert np.array_equal(out[up][:, :3], np.broadcast_to(sky, (int(up.sum()), 3))) and np.array_equal(out[down][:, :3], np.broadcast_to(ground, (int(down.sum()), 3)))
    # and the sides: a column that is red only around +x (a quarter of the way right of the centre column, which is -z)
    img2 = np.zeros((32, 64, 3), F)
    img2[:, 44:52, 0] = 1.0
    o2 = host.env_from_latlong(img2, 16)
    x_texel = host.env_eval((o2, "rgba32f", "nearest"), host.env_cfg(), np.array([[1, 0.05, 0], [-1, 0.05, 0], [0, 0.05, 1], [0, 0.05, -1]], F))
    assert x_texel[0, 0] > 0.9 and not x_texel[1:, 0].any()


# ---- sanitizers: the statements in a stand-alone program of their own
def test_statements_run_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "the host library's compiler is needed"
    host_dir = PKG / "host"
    exe = tmp_path / "env_sanitize"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT / 'include'}",
           f"-I{host_dir}", "-o", str(exe), str(pathlib.Path(__file__).with_name("env_sanitize.cpp")), str(host_dir / "environment.cpp"), str(host_dir / "texture.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "env_sanitize ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
