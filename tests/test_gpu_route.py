"""tests/golden/route_matrix.txt against the device library: a context is put into a state of the file, the request kind's call is made, and
glrtx_stats.variant_last, fallback_last, fallback_launches, glrtx_debug_last_kernel -- or the refusal's text behind the function's name -- are the file's row.
The states: one for every row of the persistent megakernel's table, the wavefront kernel's plain, V, T and TM forms with adaptive twins, the tile kernel, the
three fallback bits, and for every request kind the first state the API can reach of each distinct refusal the file holds for it.  The file was recorded from a
copy of the device layer's logic (its header); this test is what says the copy was true, and test_route_host.py that the statement equals the file everywhere.
No image is compared: the feature tests own that."""
import numpy as np
import pytest

import route_matrix as rm
from glrt_amd import device, host, scenes
from test_gpu_maps import FLAT, _flat_everywhere, _none, _types
from test_route_host import PERSISTENT

pytestmark = pytest.mark.gpu

V, WH = rm.EXT_VOLUME, rm.EXT_WHITTED
MATRIX = rm.Matrix()
SEEDS = [host.frame_seed(0)]


def _two_triangles():
    """A fork with two leaves: a vine, which the wavefront kernel scans as a list.  It lies behind c1's camera: the launches are as short as launches get."""
    b = scenes.SceneBuilder()
    grey = b.add_material(scenes.diffuse((0.7, 0.7, 0.7)))
    lamp = b.add_material(scenes.emitter((10.0, 10.0, 10.0)))
    pos, nrm = scenes.quad((-1, 0, 51), (2, 0, 0), (0, 0, -2))
    b.add_mesh(pos[:1], nrm[:1], grey)
    b.add_mesh(pos[1:], nrm[1:], lamp)
    return b.build("sah")


@pytest.fixture(scope="module")
def world(gpu_device):
    d = device.Device()
    tree, params = scenes.config_c1(16, 8, max_depth=2, n_samples=1, subdiv=1)
    yield d, {0: tree, 2: _two_triangles()}, params
    d.close()


def reachable(s):
    """What the binding calls allow: maps, cutouts and emission maps sit on a texture set; cutouts are not bound on a vine."""
    return (s["tex"] or (not s["maps"] and s["cut_emit"] == "none")) and not (s["cut_emit"] == "cut" and s["vine"]) and s["cut_emit"] != "both"


def _cases():
    cases = []
    for name, (state, _) in PERSISTENT.items():  # every row of kPersistent: selected outright, or as the fallback of variant 2
        cases.append(("ordinary", dict(state, variant=1 if name in ("plain", "volume", "tex+maps+cut") else 2)))
    vol, tex = dict(ext_flags=V, have_volume=1, vol_switch=1), dict(tex=2, tex_switch=1)
    cases += [("ordinary", dict()), ("ordinary", dict(vine=2)), ("ordinary", vol), ("ordinary", tex), ("ordinary", dict(tex, maps=1)),  # plain (tree, list), V, T, TM
              ("adaptive", dict()), ("adaptive", vol), ("adaptive", dict(tex, maps=1)), ("adaptive_moments", tex), ("moments", dict(tex, maps=1)),
              ("cascades", dict(vine=2)), ("calibration", dict()),
              ("ordinary", dict(variant=0)),  # the tile kernel
              ("ordinary", dict(params=rm.PARAMS[1])), ("ordinary", dict(spheres=3, params=rm.PARAMS[1])),  # the depth bit, alone and beside the extension bit
              # the sample bit at the V form's range, which the plain form holds, and at the plain form's: on the scene behind the camera, where a sample is one missed ray
              ("ordinary", dict(vol, vine=2, params=rm.PARAMS[2])), ("ordinary", dict(vine=2, params=rm.PARAMS[2])), ("ordinary", dict(vine=2, params=rm.PARAMS[3]))]
    seen = {(k, rm.index(**s)) for k, s in cases}
    for kind in rm.KINDS:  # each distinct refusal of each kind, at the first state the API reaches
        want = {k for k in set(MATRIX.rows[kind]) if MATRIX.vocab[k][0] == "R"}
        for s, k in zip(rm.states(), MATRIX.rows[kind]):
            if k in want and reachable(s):
                want.discard(k)
                if (kind, rm.index(**s)) not in seen:
                    cases.append((kind, {a: b for a, b in s.items() if b != rm.DEFAULT[a]}))
        assert not want, (kind, [MATRIX.vocab[k] for k in want])
    return cases


CASES = _cases()


def _name(kind, state):
    return kind + "".join(f"-{a}={'x'.join(map(str, b)) if isinstance(b, tuple) else b}" for a, b in state.items())


def _bind(d, scene, s):
    d.set_variant(s["variant"]); d.track_motion(False); d.count_rays(False)
    d.upload_scene(scene)  # (drops a texture set and what sits on it)
    d.upload_spheres([[0.0, 1.0, 60.0 + k, 0.25, 0.0] for k in range(s["spheres"])] if s["spheres"] else None)
    d.set_extensions(s["ext_flags"])
    grid = np.linspace(0.5, 1.5, 64, dtype=np.float32).reshape(4, 4, 4)
    if s["have_volume"]:
        d.upload_volume(grid, 1000.0 * grid, (-1, 0, 50), (1, 2, 52))  # (behind the camera, like the two triangles)
    else:
        d.upload_volume(None, None, (0, 0, 0), (1, 1, 1))
    types = _types(scene)
    if s["tex"]:
        albedo = _none(scene)
        albedo[int(np.flatnonzero(types == 2)[0])] = 1
        d.upload_textures([FLAT, (np.linspace(0.1, 0.9, 48, dtype=np.float32).reshape(4, 4, 3), "rgba32f", "repeat", "bilinear")], albedo)
        assert s["tex"] == 2
    else:
        d.upload_textures(None, None)
    if s["maps"]:
        d.bind_material_maps(normal=_flat_everywhere(scene))
    if s["cut_emit"] == "cut":
        cut = _none(scene)
        cut[int(np.flatnonzero(types == 2)[0])] = 0
        d.bind_cutouts(texture=cut)
    if s["cut_emit"] == "emit":
        emit = _none(scene)
        emit[int(np.flatnonzero(types == 1)[0])] = 0
        d.bind_emission_maps(emit)
    d.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape")) if s["env"] else d.upload_environment(None)
    d.set_volume_wavefront(bool(s["vol_switch"])); d.set_texture_wavefront(bool(s["tex_switch"]))


def _call(d, kind, params, n_tri):
    if kind == "ordinary":
        d.render(params)
    elif kind == "adaptive":
        d.render_adaptive(params, SEEDS, -1.0)
    elif kind == "moments":
        d.render_moments(params, SEEDS)
    elif kind == "adaptive_moments":
        d.render_adaptive_moments(params, SEEDS, -1.0)
    elif kind == "cascades":
        d.render_cascades(params, SEEDS)
    else:
        d.hit_histogram(params, n_tri)
    d.sync()


@pytest.mark.parametrize("kind,state", CASES, ids=[_name(k, s) for k, s in CASES])
def test_the_device_routes_as_the_file_says(world, monkeypatch, kind, state):
    d, scenes_by_vine, params = world
    for name in ("GLRTX_VOLUME_WAVEFRONT", "GLRTX_TEXTURE_WAVEFRONT", "GLRTX_VARIANT", "GLRTX_NO_VINE_SCAN"):
        monkeypatch.delenv(name, raising=False)
    s = {**rm.DEFAULT, **state}
    assert reachable(s)
    expect = MATRIX.outcome(kind, **state)
    scene = scenes_by_vine[s["vine"]]
    n_tri = scene["tri"].reshape(-1, 4).shape[0]
    assert (n_tri == 2) == bool(s["vine"])
    depth, samples = s["params"]
    side = 8 if samples > rm.SAMPLE_MAX else 16  # (2^20 samples a pixel: one tile of them)
    try:
        d.resize(side, 8)
        _bind(d, scene, s)
        d.track_moments(kind in ("moments", "adaptive_moments")); d.track_cascades(kind == "cascades")
        d.clear(); d.reset_stats()
        p = dict(params, width=side, max_depth=depth, n_samples=samples, seed=SEEDS[0])
        if expect[0] == "R":
            with pytest.raises(device.GlrtxError) as err:
                _call(d, kind, p, n_tri)
            assert str(err.value) == f"glrtx error -1: {rm.FUNCTION[kind]}: {expect[1]}"
            return
        _call(d, kind, p, n_tri)
        st = d.stats()
        assert d.last_kernel() == expect[4]
        if kind != "calibration":  # (the calibration frame is not part of the caller's statistics)
            assert (st.variant_last, st.fallback_last, st.fallback_launches) == expect[1:4]
    finally:
        d.track_moments(False); d.track_cascades(False)
        d.upload_environment(None); d.upload_textures(None, None); d.upload_spheres(None); d.set_extensions(0)
        d.upload_volume(None, None, (0, 0, 0), (1, 1, 1)); d.set_volume_wavefront(False); d.set_texture_wavefront(False); d.set_variant(2); d.count_rays(True)
