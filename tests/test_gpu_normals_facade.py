"""glrt_main --animate with "rebuild_normals": true end to end on the GPU: the PNG of every step of a two-step morph is, byte for byte, the image of the same
calls driven from Python on the scene the facade parsed -- upload_rig, upload_morph_targets, upload_normal_topology, set_pose_normals, then pose_morph a step;
the rebuilt normals are in the picture."""
import numpy as np
import pytest

import animate_cases as ac
import deform_cases as dc
from glrt_amd import device, host
from test_gpu_animate_facade import _main, _png
from test_gpu_deform_facade import _render, _setup, _start

pytestmark = pytest.mark.gpu


@pytest.fixture()
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


@pytest.mark.parametrize("weld,flags", [(None, 0), ("positions", host.NORMALS_WELD_POSITIONS)], ids=["default", "positions"])
def test_animate_with_rebuilt_normals_is_the_calls_from_python(tmp_path, dev, weld, flags):
    js, an, doc, scene, obj, params = _setup(tmp_path, True)
    doc["rebuild_normals"] = True
    if weld:
        doc["weld"] = weld
    an = dc.write_animation(tmp_path, doc, name="normals.json")
    morph = dc.probe(js, an)
    mats = ac.pose_matrices(doc, 2)
    text = _main(js, tmp_path / "normals.png", "--animate", str(an))
    assert text.count("Save:") == 2 and "normals rebuilt from the moved faces" in text
    _start(dev, scene, obj)
    dev.upload_morph_targets(morph["deltas"])
    dev.upload_normal_topology(scene["vert"], scene["tri"], flags)
    dev.set_pose_normals(True)
    images = []
    for s in range(2):
        dev.pose_morph(mats[s], morph["weights"][s])
        images.append(_render(dev, params, s))
        assert np.array_equal(_png(tmp_path / f"normals_{s:04d}.png"), images[-1]), f"step {s}"
    # the rebuild is in the picture: the same poses with the switch off give other images
    dev.set_pose_normals(False)
    dev.pose_morph(mats[1], morph["weights"][1])
    assert not np.array_equal(_render(dev, params, 1), images[1])
