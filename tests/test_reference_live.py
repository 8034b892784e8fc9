"""Oracle vs the reference's own shaders on llvmpipe, through records of what the reference made of each input (tests/golden/live/, written by
tests/golden/make_golden_live.py from the reference's unmodified raytrace/screen shaders on Mesa llvmpipe in the build container).  Every input is
stored with its output, so the comparison needs neither the reference checkout nor Mesa."""
import pathlib
import sys

import numpy as np
import pytest

from conftest import assert_bit_equal
from fuzz_scenes import CASES as FUZZ_CASES
from oracle import pt_oracle

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent / "golden"))
from make_golden_live import CASES, N_SHADOW_HOSTILE, load, render_record  # noqa: E402


@pytest.fixture(scope="module")
def live():
    """{group: {key: record}}: the recorded inputs and the reference's outputs."""
    return {g: load(g) for g in ("configs", "fuzz", "hostile", "shadow_hostile", "screen", "screen_hostile")}


def _screen(rec):
    """(accumulator, [(gamma, expected bytes)]) of a resolve-pass record; a NaN gamma is the shader's default, 2.2."""
    acc = np.concatenate([rec["rgb"], rec["count"][..., None]], -1)
    return acc, [(2.2 if np.isnan(gm) else float(gm), out) for gm, out in zip(rec["gammas"], rec["out"])]


@pytest.mark.parametrize("cfg,kw,over", CASES)
def test_oracle_bit_exact_vs_live_reference(live, cfg, kw, over):
    sc, pr, rgb, cnt = render_record(live["configs"][f"case{CASES.index((cfg, kw, over))}"])
    acc, rays = pt_oracle.render(sc, pr)
    assert rays >= pr["width"] * pr["height"] * pr["n_samples"]
    assert_bit_equal(acc[..., :3], rgb, "rgb")
    assert_bit_equal(acc[..., 3], cnt, "count")


def test_random_seeds_sweep(live):
    for j in range(6):
        sc, p, rgb, cnt = render_record(live["configs"][f"seeds{j}"])
        acc, _ = pt_oracle.render(sc, p)
        assert_bit_equal(acc[..., :3], rgb, f"seed {p['seed']}")


@pytest.mark.parametrize("case", FUZZ_CASES, ids=[f"seed{c[0]}" for c in FUZZ_CASES])
def test_oracle_bit_exact_vs_live_reference_on_adversarial_scenes(live, case):
    """The scenes of tests/test_gpu_fuzz.py (ties, degenerate and axis-aligned geometry, large distances, 1-2 triangles)
    through the reference's own shader: pins the oracle where the GPU tests rely on it."""
    sc, pr, rgb, cnt = render_record(live["fuzz"][f"seed{case[0]}"])
    acc, _ = pt_oracle.render(sc, pr)
    assert_bit_equal(acc[..., :3], rgb, "rgb")
    assert_bit_equal(acc[..., 3], cnt, "count")


def test_resolve_restatement_vs_live_screen_shader(live):
    """The reference's screen.frag drawn into RGBA8 and read back against the oracle's resolve on random accumulators
    (power-of-two size, several gammas) and on a rendered image."""
    recs = live["screen"]
    assert sorted(recs) == ["random128x256", "random32x32", "render"]
    for key, rec in recs.items():
        acc, outs = _screen(rec)
        assert len(outs) == (1 if key == "render" else 4)
        for gamma, ref in outs:
            got = pt_oracle.resolve(acc, gamma)
            assert np.array_equal(got, ref), f"{key} gamma {gamma}: {int((got != ref).sum())} bytes differ"


def test_resolve_restatement_vs_live_screen_shader_on_hostile_accumulators(live):
    """Finite but hostile texels (denormals, negatives, 1e-30 .. 3e38, counts of 0 / 3e38 / fractions, values scaled by 2^-140 .. 2^119) and gammas from 1e-45
    to 3e38: llvmpipe runs the pass with denormals flushed, and so does the restatement since round 4 (counts and gammas of 3e38 showed the difference).
    Not generated: NaN / infinite texels and negative zeros -- the GL_LINEAR samplers add the neighbouring texels with weight 0, outside the restatement's domain."""
    recs = live["screen_hostile"]
    assert len(recs) == 12
    for key, rec in recs.items():
        acc, outs = _screen(rec)
        for gamma, ref in outs:
            got = pt_oracle.resolve(acc, gamma)
            assert np.array_equal(got, ref), f"{key}, gamma {gamma}: {int((got != ref).sum())} bytes differ"


def test_oracle_bit_exact_vs_live_reference_on_hostile_inputs(live):
    """The inputs that round 4's device fuzzes throw at the kernels -- determinants beyond 2^126 (the reciprocal is a denormal: llvmpipe flushes it, no hit), scenes
    scaled by 1e-12 .. 1e12, seeds up to 1e20 / inf / NaN, conductors and albedos and emitters of 0 .. 1e30 / inf / NaN, vertices at infinity and NaN -- through the
    reference: the oracle is the reference there too, so the device-against-oracle tests of the same inputs (tests/test_gpu_parity.py) mean what they say."""
    n = 0
    for tag, rec in live["hostile"].items():
        sc, p, rgb, cnt = render_record(rec)
        acc, _ = pt_oracle.render(sc, p)
        a = np.concatenate([rgb, cnt[..., None]], -1)
        same = (a.view(np.uint32) == acc.view(np.uint32)) | (np.isnan(a) & np.isnan(acc))
        assert same.all(), f"{tag}: {int((~same).any(-1).sum())} pixels differ"
        n += 1
    assert n >= 50


@pytest.mark.parametrize("seed", range(N_SHADOW_HOSTILE))
def test_oracle_bit_exact_vs_live_reference_on_shadow_hostile_scenes(live, seed):
    """Lights flush in the faces of their ancestors' boxes, sliver light triangles, receivers that run up to the lights' edges (grazing light samples), distances
    1 .. 100, the scene translated to |coordinates| up to 1e7 (tests/fuzz_scenes.py: shadow_hostile) -- what the shadow rays' search is most sensitive to -- through
    the reference: the oracle is the reference there, so the device tests of the same scenes (tests/test_gpu_fuzz.py) mean what they say."""
    sc, pr, rgb, cnt = render_record(live["shadow_hostile"][f"seed{seed}"])
    acc, _ = pt_oracle.render(sc, pr)
    assert_bit_equal(acc[..., :3], rgb, f"shadow_hostile seed {seed}")
    assert_bit_equal(acc[..., 3], cnt, f"shadow_hostile seed {seed}")
