"""glrt_main --animate with "sparse_targets": true end to end on the GPU: the PNG of every step is, byte for byte, the image of the same calls driven from Python
on the scene the facade parsed -- upload_rig, upload_morph_targets_sparse with the parser's index, then pose_morph a step; the same file without the key writes
the PNGs of the dense calls from Python."""
import numpy as np
import pytest

import animate_cases as ac
import deform_cases as dc
import deform_sparse_cases as sc
from glrt_amd import device
from test_gpu_animate_facade import H, W, _main, _parsed, _png
from test_gpu_deform_facade import _render, _start

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


def _setup(tmp_path, sparse):
    js = dc.write_scene(tmp_path, W, H)
    sc.write_targets(tmp_path)
    doc = sc.steps_doc(sparse)
    an = dc.write_animation(tmp_path, doc, name="anim.json")  # (_parsed reads the shapes' vertex ranges from anim.json beside the scene)
    scene, obj, params = _parsed(js)
    return js, an, doc, scene, obj, params


def test_animate_with_sparse_targets_is_the_calls_from_python(tmp_path, dev):
    js, an, doc, scene, obj, params = _setup(tmp_path, True)
    morph = sc.probe(js, an)
    assert morph["sparse"] and morph["offsets"].size == 4 and 0 < morph["vertex"].size < 3 * morph["n_vert"]
    mats = ac.pose_matrices(doc, 2)
    text = _main(js, tmp_path / "sparse.png", "--animate", str(an))
    assert text.count("Save:") == 2 and f"3 sparse morph targets, {morph['vertex'].size} entries" in text
    _start(dev, scene, obj)
    dev.upload_morph_targets_sparse(morph["offsets"], morph["vertex"], morph["deltas"])
    images = []
    for s in range(2):
        dev.pose_morph(mats[s], morph["weights"][s])
        images.append(_render(dev, params, s))
        assert np.array_equal(_png(tmp_path / f"sparse_{s:04d}.png"), images[-1]), f"step {s}"
    assert not np.array_equal(images[0], images[1])
    # the targets are in the picture: the same matrices without weights give other images
    dev.pose_morph(mats[0], np.zeros(3, np.float32))
    assert not np.array_equal(_render(dev, params, 0), images[0])


def test_the_same_file_without_the_key_is_the_dense_path(tmp_path, dev):
    js, an, doc, scene, obj, params = _setup(tmp_path, False)
    morph = dc.probe(js, an)
    assert morph["deltas"].shape[0] == 3 and not sc.probe(js, an)["sparse"]
    mats = ac.pose_matrices(doc, 2)
    text = _main(js, tmp_path / "dense.png", "--animate", str(an))
    assert text.count("Save:") == 2 and "3 morph targets" in text and "sparse morph" not in text
    _start(dev, scene, obj)
    dev.upload_morph_targets(morph["deltas"])
    for s in range(2):
        dev.pose_morph(mats[s], morph["weights"][s])
        assert np.array_equal(_png(tmp_path / f"dense_{s:04d}.png"), _render(dev, params, s)), f"step {s}"
