"""glrt_main --animate with morph targets end to end on the GPU: the PNG of every step is, byte for byte, the image of the same calls driven from Python on the
scene the facade parsed -- upload_rig, upload_morph_targets, then pose_morph a step --, and an animation file without "targets" gives the PNGs of a glrtx_pose
run."""
import numpy as np
import pytest

import animate_cases as ac
import deform_cases as dc
from glrt_amd import device, host, rig
from test_gpu_animate_facade import FRAMES, H, W, _main, _parsed, _png

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(tmp_path, targets):
    js = dc.write_scene(tmp_path, W, H)
    dc.write_target(tmp_path)
    doc = dc.steps_doc(targets)
    # (_parsed reads the shapes' vertex ranges through the animation probe from anim.json beside the scene)
    an = dc.write_animation(tmp_path, doc, name="anim.json")
    scene, obj, params = _parsed(js)
    return js, an, doc, scene, obj, params


def _start(d, scene, obj):
    d.upload_scene(scene); d.set_partition(0, 1, 16); d.resize(W, H)
    bones, weights = rig.rigid(obj)
    d.upload_rig(scene["vert"], bones, weights, int(obj.max()) + 1)


def _render(d, params, s):
    d.clear()
    for f in range(FRAMES):
        d.render(dict(params, seed=host.frame_seed(FRAMES * s + f)))  # the frame counter runs on across the steps
    return d.resolve_rgba8(2.2, True)


def test_animate_with_a_target_is_the_calls_from_python(tmp_path, dev):
    js, an, doc, scene, obj, params = _setup(tmp_path, True)
    morph = dc.probe(js, an)
    assert morph["deltas"].shape[0] == 1 and morph["weights"].tolist() == [[0.5], [1.25]]
    mats = ac.pose_matrices(doc, 2)
    text = _main(js, tmp_path / "morph.png", "--animate", str(an))
    assert text.count("Save:") == 2 and "1 morph targets" in text
    _start(dev, scene, obj)
    dev.upload_morph_targets(morph["deltas"])
    images = []
    for s in range(2):
        dev.pose_morph(mats[s], morph["weights"][s])
        images.append(_render(dev, params, s))
        assert np.array_equal(_png(tmp_path / f"morph_{s:04d}.png"), images[-1]), f"step {s}"
    assert not np.array_equal(images[0], images[1])
    # the target is in the picture: the same matrices without weights give other images
    dev.pose_morph(mats[0], np.zeros(1, np.float32))
    assert not np.array_equal(_render(dev, params, 0), images[0])


def test_a_file_without_targets_gives_the_pose_runs_images(tmp_path, dev):
    js, an, doc, scene, obj, params = _setup(tmp_path, False)
    mats = ac.pose_matrices(doc, 2)
    text = _main(js, tmp_path / "plain.png", "--animate", str(an))
    assert text.count("Save:") == 2 and "morph targets" not in text
    _start(dev, scene, obj)
    for s in range(2):
        dev.pose(mats[s])
        assert np.array_equal(_png(tmp_path / f"plain_{s:04d}.png"), _render(dev, params, s)), f"step {s}"
