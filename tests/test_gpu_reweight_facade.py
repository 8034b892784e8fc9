"""glrt_main --reweight on the GPU: the PNG is the bindings' image -- render_cascades of the same frames, reweight, the resolve of D (or the tone curve and
the bloom over D) -- at 48x32, 4 frames; and the flags it does not compose with are refused with a message."""
import subprocess

import numpy as np
import pytest

from conftest import PKG
from glrt_amd import device, host, scenes
from test_gpu_facade import _c1_builder

pytestmark = pytest.mark.gpu


def test_glrt_main_reweight_writes_the_bindings_image(tmp_path, gpu_device):
    from PIL import Image
    w, h, depth, frames = 48, 32, 4, 4
    b = _c1_builder()
    js = scenes.export_json_obj(b, tmp_path, w, h, (0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0)
    exe = str(PKG / "lib" / "glrt_main")

    def glrt_main(extra, name, in_flight="1"):
        out = tmp_path / name
        r = subprocess.run([exe, "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--frames-in-flight", in_flight, "--out", str(out)] + extra,
                           capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert "Reweight:" in r.stdout
        return np.asarray(Image.open(out))

    b2 = scenes.SceneBuilder()
    for pos, nrm, mid in zip(b._pos, b._nrm, b._mid):
        b2.add_mesh(pos, nrm, b2.add_material(b.materials[int(mid[0])]))
    scene = b2.build()
    c2w, s2c = scenes.camera((0, 3, 9), (0, 1, 0), (0, 1, 0), 40.0, w, h)
    params = dict(scenes.make_params(c2w, s2c, w, h, depth, 1), focal=0.0)  # (absent focalLength parses as 0)
    d = gpu_device
    d.set_variant(2); d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(w, h); d.clear()
    try:
        # start 0.125: at 4 spp the lamp's reflections spread over several cascades, so that the re-weighted image is not the plain one
        d.track_cascades(True, 0.125)
        d.render_cascades(params, [host.frame_seed(f) for f in range(frames)])
        plain = d.resolve_rgba8(2.2, True)
        d.reweight(kappa=2.0)
        ref = d.resolve_denoised_rgba8(2.2, True)
        flags = ["--reweight", "--reweight-kappa", "2", "--reweight-start", "0.125"]
        for in_flight in ("1", "3", "16"):
            img = glrt_main(flags, f"rw{in_flight}.png", in_flight)
            assert np.array_equal(img, ref), (in_flight, int((img != ref).any(-1).sum()))
        assert not np.array_equal(ref, plain)
        assert np.array_equal(glrt_main(flags + ["--tonemap", "aces"], "rw_aces.png"), d.resolve_tonemapped_rgba8(source=1, op=2))
        d.bloom(source=1)
        assert np.array_equal(glrt_main(flags + ["--bloom"], "rw_bloom.png"), d.resolve_bloomed_rgba8(op=0))
        d.track_cascades(True)  # the defaults
        d.clear()
        d.render_cascades(params, [host.frame_seed(f) for f in range(frames)])
        d.reweight()
        assert np.array_equal(glrt_main(["--reweight"], "rw_default.png"), d.resolve_denoised_rgba8(2.2, True))
    finally:
        d.track_cascades(False)
    for extra, word in ((["--denoise"], "--denoise"), (["--denoise-variance"], "--denoise-variance"), (["--adaptive", "0.05"], "--adaptive"),
                        (["--adaptive-variance", "0.05"], "--adaptive-variance"), (["--enable-volume"], "--enable-volume"),
                        (["--save-every-frame"], "--save-every-frame"), (["--reweight-kappa", "0"], "--reweight-kappa"),
                        (["--reweight-start", "0"], "--reweight-start"), (["--frames-in-flight", "1025"], "--frames-in-flight")):
        r = subprocess.run([exe, "-i", str(js), "--reweight"] + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--reweight" in r.stderr and word in r.stderr, (extra, r.stderr)
    r = subprocess.run([exe, "-i", str(js), "--reweight-kappa", "2"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--reweight" in r.stderr
