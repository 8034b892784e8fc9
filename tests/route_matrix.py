"""tests/golden/route_matrix.txt for the tests that read it (test_route_host.py, test_gpu_route.py): the recorded route of every context state, per request kind.
The file's header says how it was recorded and in which order its states run; this module repeats that order and nothing of the rule."""
import itertools
import pathlib

EXT_WHITTED, EXT_VOLUME = 2, 4
KINDS = ("ordinary", "adaptive", "moments", "calibration", "adaptive_moments", "cascades")
FUNCTION = {"ordinary": "glrtx_render", "adaptive": "glrtx_render_adaptive", "moments": "glrtx_render_moments", "calibration": "glrtx_hit_histogram",
            "adaptive_moments": "glrtx_render_adaptive_moments", "cascades": "glrtx_render_cascades"}
DEPTH_MAX, SAMPLE_MAX, VOL_SAMPLE_MAX = 255, (1 << 20) - 1, (1 << 16) - 1
PARAMS = ((2, 1), (DEPTH_MAX + 1, 1), (2, VOL_SAMPLE_MAX + 1), (2, SAMPLE_MAX + 1))  # (max_depth, n_samples): within both ranges, then one past each
# outermost first; the last varies fastest
AXES = (("tex", (0, 2)), ("cut_emit", ("none", "cut", "emit")), ("env", (0, 1)), ("tex_switch", (0, 1)),
        ("ext_flags", (0, EXT_WHITTED, EXT_VOLUME, EXT_VOLUME | EXT_WHITTED)), ("spheres", (0, 3)), ("have_volume", (0, 1)), ("variant", (0, 1, 2)),
        ("maps", (0, 1)), ("params", PARAMS), ("vine", (0, 2)), ("vol_switch", (0, 1)))
N_STATES = 36864
DEFAULT = dict(tex=0, cut_emit="none", env=0, tex_switch=0, ext_flags=0, spheres=0, have_volume=0, variant=2, maps=0, params=PARAMS[0], vine=0, vol_switch=0)


def states(both=False):
    """Every state in the file's order, as dicts over AXES' names; both: the states with cutouts AND emission maps bound (cut_emit "both")."""
    axes = [(k, ("both",) if both and k == "cut_emit" else v) for k, v in AXES]
    for values in itertools.product(*(v for _, v in axes)):
        yield dict(zip((k for k, _ in axes), values))


def index(**state):
    """The position of a state of the main enumeration; axes not named take DEFAULT's value."""
    s = {**DEFAULT, **state}
    assert set(s) == set(DEFAULT), sorted(set(s) - set(DEFAULT))
    i = 0
    for k, values in AXES:
        i = i * len(values) + values.index(s[k])
    return i


def route_state(s):
    """A state of the enumeration as glrt_route_state's fields."""
    return dict(variant=s["variant"], ext_flags=s["ext_flags"], n_spheres=s["spheres"], n_tex=s["tex"], n_vine=s["vine"], have_volume=s["have_volume"],
                have_maps=s["maps"], have_cut=int(s["cut_emit"] in ("cut", "both")), have_emit=int(s["cut_emit"] in ("emit", "both")), have_env=s["env"],
                vol_switch=s["vol_switch"], tex_switch=s["tex_switch"], max_depth=s["params"][0], n_samples=s["params"][1])


class Matrix:
    """vocab[i]: ("K", variant_last, fallback_last, counted, kernel name) or ("R", text); rows[kind] / both[kind]: one vocabulary index a state."""

    def __init__(self, path=pathlib.Path(__file__).parent / "golden" / "route_matrix.txt"):
        lines = [ln for ln in path.read_text().splitlines() if ln and not ln.startswith("#")]
        n = int(lines[0].split()[1])
        assert lines[0].split()[0] == "vocab"
        self.vocab = []
        for i, ln in enumerate(lines[1:1 + n]):
            k, what, rest = ln.split(" ", 2)
            assert int(k) == i and what in "KR", ln
            if what == "K":
                variant, fallback, counted, name = rest.split(" ", 3)
                self.vocab.append(("K", int(variant), int(fallback), int(counted), name))
            else:
                self.vocab.append(("R", rest))
        self.rows, self.both = {}, {}
        into = None
        for ln in lines[1 + n:]:
            if ln.startswith(("kind ", "both ")):
                section, kind, count = ln.split()
                into = (self.rows if section == "kind" else self.both).setdefault(kind, [])
                expect = int(count)
                continue
            for run in ln.split():
                k, times = run.split("x")
                into.extend([int(k)] * int(times))
            assert len(into) <= expect
        assert set(self.rows) == set(self.both) == set(KINDS)
        assert all(len(v) == N_STATES for v in self.rows.values()) and all(len(v) == N_STATES // 3 for v in self.both.values())

    def outcome(self, kind, **state):
        return self.vocab[self.rows[kind][index(**state)]]
