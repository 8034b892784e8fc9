"""glrt_main --bloom end to end on the GPU: the PNG is what the Python calls predict from the same frames, with and without a tone curve and a denoiser in
front, and without the flag the PNG is what it was."""
import subprocess

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import host, scenes
from test_gpu_facade import _c1_builder

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES = 96, 64, 4, 3


def _run(js, out, *flags):
    r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(DEPTH), "--frames", str(FRAMES), "--out", str(out), *flags],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    from PIL import Image
    return np.asarray(Image.open(out)), r.stdout


def test_glrt_main_bloom_writes_what_the_binding_predicts(tmp_path, gpu_device):
    b = _c1_builder()
    js = scenes.export_json_obj(b, tmp_path, W, H, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)
    plain, text = _run(js, tmp_path / "plain.png")
    assert "Bloom:" not in text
    aces, text = _run(js, tmp_path / "aces.png", "--bloom", "--tonemap", "aces")
    assert "Bloom: threshold 1, strength 0.25, 5 levels" in text
    bare, _ = _run(js, tmp_path / "bare.png", "--bloom", "--bloom-threshold", "0.5", "--bloom-strength", "0.6", "--bloom-levels", "3")
    den, _ = _run(js, tmp_path / "den.png", "--denoise", "--bloom", "--tonemap", "aces", "--auto-exposure")

    b2 = scenes.SceneBuilder()  # (material ids follow shape order in Scene::parse: one material per shape)
    for pos, nrm, mid in zip(b._pos, b._nrm, b._mid):
        b2.add_mesh(pos, nrm, b2.add_material(b.materials[int(mid[0])]))
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, W, H)
    params = dict(scenes.make_params(c2w, s2c, W, H, DEPTH, 1), focal=0.0)
    d = gpu_device
    d.upload_scene(b2.build()); d.set_partition(0, 1, 16); d.resize(W, H); d.exposure_reset()
    d.render_features(params)
    for f in range(FRAMES):
        d.render(dict(params, seed=host.frame_seed(f)))
    assert np.array_equal(plain, d.resolve_rgba8(2.2, True))
    d.bloom()
    assert np.array_equal(aces, d.resolve_bloomed_rgba8(op="aces"))
    assert not np.array_equal(aces, d.resolve_tonemapped_rgba8(op="aces"))  # (the lamp glows)
    d.bloom(threshold=0.5, strength=0.6, levels=3)
    assert np.array_equal(bare, d.resolve_bloomed_rgba8())  # without --tonemap: op 0 at exposure 1
    d.denoise(); d.exposure_reset()
    d.exposure_measure(source=1, op="aces", auto_exposure=1)
    d.bloom(source=1)
    assert np.array_equal(den, d.resolve_bloomed_rgba8(op="aces", auto_exposure=1))


def test_glrt_main_refuses_bloom_options_without_bloom(tmp_path):
    for flags in (["--bloom-levels", "3"], ["--bloom-strength", "1"], ["--bloom", "--bloom-levels", "9"], ["--bloom", "--bloom-threshold", "-1"],
                  ["--bloom", "--save-every-frame"]):
        r = subprocess.run([str(PKG / "lib" / "glrt_main"), "-i", str(tmp_path / "none.json"), *flags], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--bloom" in r.stderr, flags
