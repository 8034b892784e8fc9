"""glrt_main --animate end to end on the GPU: the PNG of every step is, byte for byte, the image of the call sequence Window::setAnimation documents, driven
from Python on the scene the facade parsed -- once plain, once with --carry-history --denoise-variance --tonemap aces; without --animate the PNG is what it
was; the combinations --animate does not take are refused with their message."""
import subprocess

import numpy as np
import pytest

import animate_cases as ac
from conftest import PKG
from glrt_amd import device, host, rig
from test_scene_parse import _probe

pytestmark = pytest.mark.gpu

W, H, DEPTH, FRAMES = 64, 48, 4, 2
MAIN = str(PKG / "lib" / "glrt_main")


def _main(js, out, *flags):
    r = subprocess.run([MAIN, "-i", str(js), "--max-depth", str(DEPTH), "--frames", str(FRAMES), "--out", str(out), *flags], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path))


def _parsed(js):
    """The scene as the facade uploads it (the parser's own vertices: file normals are renormalised on load), its shapes' rig, and the scene file's camera."""
    sc = _probe(js)
    scene = dict(vert=sc["vert"], tri=sc["tri"], mat=sc["mat"], light=sc["light"], bvh=sc["nodes"])
    first = ac.probe(js, js.parent / "anim.json")["first_vertex"]
    obj = np.repeat(np.arange(len(first) - 1), np.diff(first)).astype(np.int32)
    params = dict(c2w=host.mat4_inverse(sc["view"]), s2c=host.mat4_inverse(sc["proj"]), width=W, height=H, max_depth=DEPTH, n_samples=1, seed=(0.0, 0.0),
                  aperture=float(sc["lens"][0]), focal=float(sc["lens"][1]))
    return scene, obj, params


def _step_params(params, doc, s):
    cam = doc["steps"][s].get("camera")
    if cam is None:
        return params
    view, proj, ap, fo = ac.camera_params(cam, W, H)
    return dict(params, c2w=host.mat4_inverse(view), s2c=host.mat4_inverse(proj), aperture=float(ap), focal=float(fo))


@pytest.fixture()
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _start(d, scene, obj):
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H)
    bones, weights = rig.rigid(obj)
    d.upload_rig(scene["vert"], bones, weights, int(obj.max()) + 1)


def test_animate_writes_the_documented_call_sequence(tmp_path, dev):
    js, an = ac.write_scene(tmp_path, W, H), ac.write_animation(tmp_path)
    doc = ac.steps_doc()
    scene, obj, params = _parsed(js)
    mats = ac.pose_matrices(doc, int(obj.max()) + 1)
    seeds = [host.frame_seed(f) for f in range(FRAMES * len(doc["steps"]))]  # the frame counter runs on across the steps

    text = _main(js, tmp_path / "plain.png", "--animate", str(an))
    assert text.count("Save:") == 3 and not (tmp_path / "plain.png").exists()
    _start(dev, scene, obj)
    images = []
    for s in range(3):
        p = _step_params(params, doc, s)
        dev.pose(mats[s])
        dev.clear()
        for f in range(FRAMES):
            dev.render(dict(p, seed=seeds[FRAMES * s + f]))
        images.append(dev.resolve_rgba8(2.2, True))
        assert np.array_equal(_png(tmp_path / f"plain_{s:04d}.png"), images[-1]), f"plain, step {s}"
    assert not np.array_equal(images[0], images[1]) and not np.array_equal(images[1], images[2])

    text = _main(js, tmp_path / "carry.png", "--animate", str(an), "--carry-history", "--denoise-variance", "--tonemap", "aces")
    assert text.count("Save:") == 3 and text.count("carries history") == 2
    d = device.Device()
    try:
        _start(d, scene, obj)
        for s in range(3):
            p = _step_params(params, doc, s)
            d.pose(mats[s])
            if s == 0:
                d.track_motion(True); d.track_moments(True); d.render_features(p)
            else:
                d.reproject_motion(p)
                assert d.reproject_last()[0] > 0
            d.render_moments(p, seeds[FRAMES * s:FRAMES * (s + 1)])
            d.denoise_variance()
            want = d.resolve_tonemapped_rgba8(op="aces", source=1)
            assert np.array_equal(_png(tmp_path / f"carry_{s:04d}.png"), want), f"carry, step {s}"
            assert not np.array_equal(want, images[s])
    finally:
        d.close()


def test_without_animate_every_png_is_what_it_was(tmp_path, dev):
    js = ac.write_scene(tmp_path, W, H)
    ac.write_animation(tmp_path)
    scene, obj, params = _parsed(js)
    _main(js, tmp_path / "still.png")
    _main(js, tmp_path / "still_dv.png", "--denoise-variance", "--tonemap", "aces")
    dev.upload_scene(scene); dev.set_partition(0, 1, 16); dev.resize(W, H)
    for f in range(FRAMES):
        dev.render(dict(params, seed=host.frame_seed(f)))
    assert np.array_equal(_png(tmp_path / "still.png"), dev.resolve_rgba8(2.2, True))
    dev.clear()
    dev.render_features(params); dev.track_moments(True)
    dev.render_moments(params, [host.frame_seed(f) for f in range(FRAMES)])
    dev.denoise_variance()
    assert np.array_equal(_png(tmp_path / "still_dv.png"), dev.resolve_tonemapped_rgba8(op="aces", source=1))


REFUSED = [
    (["--gpus", "2"], "--animate: one device"),
    (["--adaptive", "0.05"], "--animate: one device, and not with --adaptive"),
    (["--adaptive-variance", "0.05"], "--animate: one device, and not with --adaptive"),
    (["--reweight"], "--reweight"),
    (["--enable-volume"], "--enable-volume"),
    (["--extensions"], "--extensions"),
    (["--save-every-frame"], "--save-every-frame"),
    (["--carry-history", "--denoise"], "--carry-history: not with --denoise"),
]


@pytest.mark.parametrize("flags,message", REFUSED, ids=[" ".join(r[0]) for r in REFUSED])
def test_refused_combinations(tmp_path, flags, message):
    js, an = ac.write_scene(tmp_path, W, H), ac.write_animation(tmp_path)
    r = subprocess.run([MAIN, "-i", str(js), "--frames", "1", "--out", str(tmp_path / "o.png"), "--animate", str(an), *flags], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and message in r.stderr, (flags, r.stderr[-300:])
    assert not list(tmp_path.glob("o*.png"))


def test_carry_history_needs_animate(tmp_path):
    r = subprocess.run([MAIN, "-i", str(tmp_path / "none.json"), "--carry-history"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "--carry-history needs --animate" in r.stderr
