"""A launch's route (host/route_statement.h, through glrt_launch_route) without a GPU: over every context state and request kind it answers what
tests/golden/route_matrix.txt recorded from the device layer's logic before the statement existed -- kernel family, fallback bits, kernel name, or the
refusal's text; then a handful of rows spelled out, to be checked by eye; the ABI; the statement in a stand-alone program under the sanitizers.
tests/test_gpu_route.py ties the same file to what the device library really does."""
import ctypes as C
import pathlib
import re
import shutil
import subprocess

import pytest

import route_matrix as rm
from conftest import PKG, ROOT
from glrt_amd import host

W, V = rm.EXT_WHITTED, rm.EXT_VOLUME


@pytest.fixture(scope="module")
def matrix():
    return rm.Matrix()


def _outcome(state, kind):
    route, refusal = host.launch_route(state, kind)
    if route is None:
        return ("R", refusal)
    assert route.family == route.variant_last
    return ("K", route.variant_last, route.fallback_last, route.fallback_counts, route.kernel.decode())


@pytest.mark.parametrize("kind", rm.KINDS)
def test_every_state_routes_as_recorded(matrix, kind):
    for both, rows in ((False, matrix.rows[kind]), (True, matrix.both[kind])):
        n = 0
        for s, k in zip(rm.states(both), rows):
            got = _outcome(host.RouteState(**rm.route_state(s)), rm.KINDS.index(kind))
            assert got == matrix.vocab[k], (kind, s, got, matrix.vocab[k])
            n += 1
        assert n == len(rows) == (rm.N_STATES // 3 if both else rm.N_STATES)


def test_the_file_is_one_small_text_file_that_says_where_it_comes_from(matrix):
    path = ROOT / "tests" / "golden" / "route_matrix.txt"
    assert path.stat().st_size < 100 * 1024
    head = path.read_text()[:1500]
    assert "RECORDED from the logic of the commit BEFORE the route statement existed" in head and "36864 states a kind" in head
    assert rm.index() == rm.index(**rm.DEFAULT) and rm.index(tex=2, cut_emit="emit", env=1, tex_switch=1, ext_flags=V | W, spheres=3, have_volume=1, variant=2,
                                                             maps=1, params=rm.PARAMS[3], vine=2, vol_switch=1) == rm.N_STATES - 1
    # the three lists with a side plane are one list; only the adaptive one's kernels carry another name
    assert matrix.rows["moments"] == matrix.rows["cascades"]
    assert [matrix.vocab[k][-1].replace(", adaptive", "").replace(" (adaptive)", "").replace("(adaptive, ", "(") for k in matrix.rows["adaptive_moments"]] == \
           [matrix.vocab[k][-1] for k in matrix.rows["moments"]]


P = "pt_render_persistent"
# the rows of tests/test_gpu_megakernel_forms.py's FORMS, on variant 1 as there: state -> kernel name
PERSISTENT = {
    "plain": (dict(), P),
    "ext": (dict(ext_flags=W), P + " (extensions)"),
    "volume": (dict(ext_flags=V, have_volume=1), P + " (volume)"),
    "tex": (dict(tex=2), P + " (extensions, textures)"),
    "tex+volume": (dict(tex=2, ext_flags=V, have_volume=1), P + " (volume, textures)"),
    "tex+maps": (dict(tex=2, maps=1), P + " (extensions, textures, maps)"),
    "tex+volume+maps": (dict(tex=2, maps=1, ext_flags=V, have_volume=1), P + " (volume, textures, maps)"),
    "env": (dict(env=1), P + " (extensions, environment)"),
    "env+tex": (dict(env=1, tex=2), P + " (extensions, environment, textures)"),
    "env+tex+maps": (dict(env=1, tex=2, maps=1), P + " (extensions, environment, textures, maps)"),
    "tex+cut": (dict(tex=2, cut_emit="cut"), P + " (extensions, textures, cutouts)"),
    "tex+maps+cut": (dict(tex=2, maps=1, cut_emit="cut"), P + " (extensions, textures, maps, cutouts)"),
    "env+tex+cut": (dict(env=1, tex=2, cut_emit="cut"), P + " (extensions, environment, textures, cutouts)"),
    "env+tex+maps+cut": (dict(env=1, tex=2, maps=1, cut_emit="cut"), P + " (extensions, environment, textures, maps, cutouts)"),
    "tex+emit": (dict(tex=2, cut_emit="emit"), P + " (extensions, textures, emission maps)"),
    "tex+maps+emit": (dict(tex=2, maps=1, cut_emit="emit"), P + " (extensions, textures, maps, emission maps)"),
    "env+tex+emit": (dict(env=1, tex=2, cut_emit="emit"), P + " (extensions, environment, textures, emission maps)"),
    "env+tex+maps+emit": (dict(env=1, tex=2, maps=1, cut_emit="emit"), P + " (extensions, environment, textures, maps, emission maps)"),
}


@pytest.mark.parametrize("form", list(PERSISTENT))
def test_the_megakernel_rows_spelled_out(matrix, form):
    state, name = PERSISTENT[form]
    # selected as variant 1 it is no fallback; selected as variant 2, anything bound makes it one -- a plain context stays on the wavefront kernel
    assert matrix.outcome("ordinary", variant=1, **state) == ("K", 1, 0, 0, name) == _outcome(rm.route_state({**rm.DEFAULT, **state, "variant": 1}), "ordinary")
    expect = ("K", 1, 4, 1, name) if state else ("K", 2, 0, 0, "pt_render_wgwf")
    assert matrix.outcome("ordinary", variant=2, **state) == expect == _outcome(rm.route_state({**rm.DEFAULT, **state}), "ordinary")


ROWS = [  # (kind, state, outcome)
    # the wavefront kernel's forms: plain (tree, list scan), V, T, TM, and their adaptive twins
    ("ordinary", dict(), ("K", 2, 0, 0, "pt_render_wgwf")),
    ("ordinary", dict(vine=2), ("K", 2, 0, 0, "pt_render_wgwf (list scan)")),
    ("ordinary", dict(ext_flags=V, have_volume=1, vol_switch=1), ("K", 2, 0, 0, "pt_render_wgwf (volume)")),
    ("ordinary", dict(tex=2, tex_switch=1), ("K", 2, 0, 0, "pt_render_wgwf (textures)")),
    ("ordinary", dict(tex=2, maps=1, tex_switch=1), ("K", 2, 0, 0, "pt_render_wgwf (textures, maps)")),
    ("adaptive", dict(ext_flags=V, have_volume=1, vol_switch=1), ("K", 2, 0, 0, "pt_render_wgwf (volume, adaptive)")),
    ("adaptive_moments", dict(tex=2, maps=1, tex_switch=1), ("K", 2, 0, 0, "pt_render_wgwf (textures, maps, adaptive)")),
    ("calibration", dict(), ("K", 2, 0, 0, "pt_render_wgwf")),
    # a switch that is on and cannot apply changes nothing: a vine tree under a texture set, the volume beside spheres
    ("ordinary", dict(tex=2, tex_switch=1, vine=2), ("K", 1, 4, 1, P + " (extensions, textures)")),
    ("ordinary", dict(ext_flags=V, have_volume=1, vol_switch=1, spheres=3), ("K", 1, 4, 1, P + " (volume)")),
    # the tile kernel, and the three fallback bits
    ("ordinary", dict(variant=0), ("K", 0, 0, 0, "pt_render_kernel")),
    ("ordinary", dict(params=rm.PARAMS[1]), ("K", 1, 1, 1, P)),
    ("ordinary", dict(params=rm.PARAMS[3]), ("K", 1, 2, 1, P)),
    ("ordinary", dict(params=rm.PARAMS[2]), ("K", 2, 0, 0, "pt_render_wgwf")),
    ("ordinary", dict(ext_flags=V, have_volume=1, vol_switch=1, params=rm.PARAMS[2]), ("K", 1, 2, 1, P + " (volume)")),  # (the V form's narrower range)
    ("ordinary", dict(spheres=3, params=rm.PARAMS[1]), ("K", 1, 5, 1, P + " (extensions)")),
    # one refusal a kind
    ("ordinary", dict(ext_flags=V), ("R", "GLRTX_EXT_VOLUME is set and no volume is uploaded (glrtx_upload_volume)")),
    ("ordinary", dict(ext_flags=V, have_volume=1, tex=2, cut_emit="cut"), ("R", "GLRTX_EXT_VOLUME is set and cutouts are bound (the volume kernels have no cutout form)")),
    ("adaptive", dict(spheres=3), ("R", "spheres are uploaded (only the wavefront kernel has a tile list)")),
    ("adaptive", dict(variant=1), ("R", "variant 1 (only the wavefront kernel, variant 2, has a tile list)")),
    ("moments", dict(ext_flags=V, have_volume=1, vol_switch=1), ("R", "extensions or volume are on")),
    ("moments", dict(tex=2), ("R", "textures are bound and the wavefront kernel does not shade them here: the texture wavefront switch is off "
                                   "(glrtx_set_texture_wavefront) (the megakernel that shades them writes no sample planes)")),
    ("adaptive_moments", dict(params=rm.PARAMS[1]), ("R", "max_depth 256 / n_samples 1 beyond the wavefront kernel's path state")),
    ("cascades", dict(env=1), ("R", "an environment is bound (the megakernel that shades it writes no sample planes)")),
    ("calibration", dict(tex=2, cut_emit="emit"), ("R", "textures are bound and emission maps are bound (wavefront kernel only)")),
    ("calibration", dict(variant=1), ("R", "wavefront kernel only")),
]


@pytest.mark.parametrize("kind,state,expect", ROWS, ids=[f"{k}-{'-'.join(f'{a}={b}' for a, b in s.items()) or 'plain'}" for k, s, _ in ROWS])
def test_rows_spelled_out(matrix, kind, state, expect):
    assert matrix.outcome(kind, **state) == expect
    assert _outcome(rm.route_state({**rm.DEFAULT, **state}), kind) == expect


def test_the_abi():
    text = (ROOT / "include" / "glrt_host.h").read_text()
    assert re.search(r"\bint glrt_launch_route\(const glrt_route_state \*state, int kind, glrt_route \*route_out, char \*msg, size_t cap\);", text)
    for k, name in enumerate(rm.KINDS):
        assert f"#define GLRT_ROUTE_{name.upper()} {k}" in text
    assert host.ROUTE_KINDS == rm.KINDS
    H = C.CDLL(str(PKG / "lib" / "libglrt_host.so"))
    assert hasattr(H, "glrt_launch_route")
    assert C.sizeof(host.RouteState) == 14 * 4 and C.sizeof(host.Route) == 5 * 4 + 96
    L, state, out, msg = host.lib(), host.RouteState(variant=2, max_depth=2, n_samples=1), host.Route(), C.create_string_buffer(8)
    assert L.glrt_launch_route(None, 0, C.byref(out), msg, 8) == -2 and L.glrt_launch_route(C.byref(state), 0, None, msg, 8) == -2
    assert L.glrt_launch_route(C.byref(state), 6, C.byref(out), msg, 8) == -2 and L.glrt_launch_route(C.byref(state), -1, C.byref(out), msg, 8) == -2
    state.variant = 1
    assert L.glrt_launch_route(C.byref(state), 3, C.byref(out), msg, 8) == -1 and msg.value == b"wavefro" and out.kernel == b""  # (a small message buffer)
    assert L.glrt_launch_route(C.byref(state), 3, C.byref(out), None, 0) == -1
    assert L.glrt_launch_route(C.byref(state), 0, C.byref(out), None, 0) == 0 and out.kernel == b"pt_render_persistent"


# ---- sanitizers: the statement in a stand-alone program of its own
def test_the_statement_runs_clean_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx is not None, "the host library's compiler is needed"
    host_dir = PKG / "host"
    exe = tmp_path / "route_sanitize"
    cmd = [cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{ROOT / 'include'}", f"-I{host_dir}", "-o", str(exe),
           str(pathlib.Path(__file__).with_name("route_sanitize.cpp")), str(host_dir / "route.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "route_sanitize ok" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]
