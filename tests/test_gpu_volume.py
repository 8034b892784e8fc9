"""The volume branch (GLRTX_EXT_VOLUME) on the device, through the C ABI, bit for bit against the reference's shader on llvmpipe
with the branch switched on (tests/golden/make_golden_volume.py; the fixtures' two shader classes are described there), and the
device's log / exp / acos / blackBody / lookup against llvmpipe's own (math_volume.npz)."""
import numpy as np
import pytest

from conftest import GOLDEN, assert_bit_equal, load_golden
from glrt_amd import device
import volume_math as vm

pytestmark = pytest.mark.gpu

VOLUME = GOLDEN / "volume"
FIXTURES = sorted(p.stem for p in VOLUME.glob("vol_*.npz"))
BOTH_INSTANTIATIONS = pytest.mark.parametrize("count_rays", [True, False], ids=["counting", "timed"])


def load_volume(name):
    scene, params, rows, frames, rgb, cnt = load_golden(f"volume/{name}")
    z = np.load(VOLUME / f"{name}.npz")
    vol = dict(density=z["density"], temperature=z["temperature"], bbox_min=z["bbox"][:3], bbox_max=z["bbox"][3:],
               density_max=float(z["density_max"]))
    return scene, params, frames, vol, rgb, cnt


def render(target, scene, params, frames, vol, flags=device.EXT_VOLUME, count_rays=True):
    """Upload, render (the fixture's frames through render_frames), read back; leaves the target without volume and flags."""
    target.upload_scene(scene)
    if vol is not None:
        target.upload_volume(**vol)
    try:
        if isinstance(target, device.Group):
            target.member_call(target.L.glrtx_set_extensions, int(flags))
            target.member_call(target.L.glrtx_count_rays, int(count_rays))
        else:
            target.set_extensions(flags)
            target.set_partition(0, 1, 16)
            target.reset_stats()
            target.count_rays(count_rays)
        target.resize(params["width"], params["height"])
        if frames:
            target.render_frames(params, frames)
        else:
            target.render(params)
        target.sync()
        return target.read_accum(), target.stats()
    finally:
        if isinstance(target, device.Group):
            target.member_call(target.L.glrtx_set_extensions, 0)
        else:
            target.set_extensions(0)
        target.upload_volume(None, None, (0, 0, 0), (1, 1, 1))


@BOTH_INSTANTIATIONS
@pytest.mark.parametrize("name", FIXTURES)
def test_volume_matches_reference_golden(gpu_device, name, count_rays):
    scene, params, frames, vol, rgb, cnt = load_volume(name)
    acc, st = render(gpu_device, scene, params, frames, vol, count_rays=count_rays)
    assert st.variant_last == 1  # the persistent megakernel's volume instantiation
    assert_bit_equal(acc[..., :3], rgb, f"{name} rgb")
    assert_bit_equal(acc[..., 3], cnt, f"{name} count")
    if count_rays:
        assert st.rays > 0


def test_volume_trials_are_counted_as_rays(gpu_device):
    """Every trial ray of the Woodcock tracking is an execution of intersect() (raytrace.frag:439): the same scene renders more rays
    with the branch on than with it off, where a media surface seen from the front only repeats its camera ray's traversal."""
    scene, params, frames, vol, _, _ = load_volume("vol_const_lod")
    _, on = render(gpu_device, scene, params, frames, vol)
    _, off = render(gpu_device, scene, params, frames, vol, flags=0)
    assert on.rays != off.rays and on.rays > 0 and off.rays > 0


@pytest.mark.parametrize("name", ["vol_fire16", "vol_noise_12x7x5", "vol_open", "vol_frames3"])
def test_volume_group_of_two_on_one_device_matches_one_context(gpu_device, name):
    scene, params, frames, vol, rgb, cnt = load_volume(name)
    one, _ = render(gpu_device, scene, params, frames, vol)
    g = device.Group([0, 0])
    try:
        two, _ = render(g, scene, params, frames, vol)
    finally:
        g.close()
    assert_bit_equal(two, one, f"{name}: group vs context")
    assert_bit_equal(two[..., :3], rgb, f"{name}: group vs reference")


def test_volume_flag_off_keeps_media_front(gpu_device):
    """Off by default: with a volume uploaded and GLRTX_EXT_VOLUME clear, a media surface seen from the front leaves the ray unchanged
    (the reference with ENABLE_VOLUME 0), bit for bit the media_front fixture."""
    scene, params, rows, frames, rgb, cnt = load_golden("media_front")
    z = np.load(VOLUME / "vol_fire16.npz")
    vol = dict(density=z["density"], temperature=z["temperature"], bbox_min=(-4, -1, -4), bbox_max=(4, 3, 4))
    acc, st = render(gpu_device, scene, params, frames, vol, flags=0)
    assert not st.fallback_last & device.FALLBACK_EXTENSIONS  # the volume alone does not leave the selected kernel
    assert_bit_equal(acc[..., :3], rgb, "media_front rgb")
    assert_bit_equal(acc[..., 3], cnt, "media_front count")


def test_volume_flag_without_volume_is_an_error(gpu_device):
    scene, params, frames, vol, _, _ = load_volume("vol_const_lod")
    gpu_device.upload_scene(scene)
    gpu_device.resize(params["width"], params["height"])
    gpu_device.set_extensions(device.EXT_VOLUME)
    try:
        with pytest.raises(device.GlrtxError, match="no volume is uploaded") as e:
            gpu_device.render(params)
        assert e.value.code == device.GLRTX_EINVAL
        gpu_device.upload_volume(**vol)
        gpu_device.upload_volume(None, None, (0, 0, 0), (1, 1, 1))  # removed again
        with pytest.raises(device.GlrtxError, match="no volume is uploaded"):
            gpu_device.render(params)
    finally:
        gpu_device.set_extensions(0)
    with pytest.raises(device.GlrtxError, match="zero or non-finite extent"):
        gpu_device.upload_volume(vol["density"], vol["temperature"], (0, 0, 0), (1, 0, 1))


@pytest.fixture(scope="module")
def sweep():
    return np.load(VOLUME / "math_volume.npz")


@pytest.mark.parametrize("fn,op", [("exp", device.VMATH_EXP), ("log", device.VMATH_LOG), ("acos", device.VMATH_ACOS)])
def test_device_math_matches_llvmpipe(gpu_device, sweep, fn, op):
    got = device.volume_math(op, sweep["x"])
    assert_bit_equal(got, sweep[fn], f"device {fn}")
    assert_bit_equal(got, getattr(vm, f"lp_{fn}")(sweep["x"]), f"device {fn} vs numpy statement")


def test_device_blackbody_matches_llvmpipe(gpu_device, sweep):
    assert_bit_equal(device.volume_math(device.VMATH_BLACKBODY, sweep["temp"]), sweep["blackbody"], "device blackBody")


def test_device_lookup_matches_llvmpipe(gpu_device, sweep):
    got = device.volume_lookup(sweep["grid"], sweep["bbox"][:3], sweep["bbox"][3:], sweep["pos"])
    assert_bit_equal(got, sweep["lookup"], "device lookup")


def test_glrt_main_enable_volume_renders_like_the_binding(tmp_path, gpu_device):
    """The façade end to end: a JSON scene whose media shape names two VOL files, rendered by glrt_main --enable-volume, equals the same
    frames through the C ABI (upload_volume with the JSON's bbox and the density file's maximum, EXT_VOLUME); without the switch the
    files are not read and the image is the pass-through one."""
    import subprocess
    from PIL import Image
    from conftest import PKG
    from glrt_amd import host, scenes
    w, h, depth, frames = 64, 48, 8, 3
    lo, hi = (-1.0, 0.05, -1.0), (1.0, 2.05, 1.0)
    dens, temp = scenes.fire_grids((16, 16, 16), 10.0)
    b = scenes.SceneBuilder()
    b.add_mesh(*scenes.box(lo, hi), b.add_material(scenes.media({"density": "d.vol", "temperature": "t.vol", "bboxMin": lo, "bboxMax": hi})))
    b.add_mesh(*scenes.quad((-6, 0, 6), (12, 0, 0), (0, 0, -12)), b.add_material(scenes.diffuse((0.7, 0.7, 0.7))))
    b.add_mesh(*scenes.quad((-1, 4, -1), (2, 0, 0), (0, 0, 2)), b.add_material(scenes.emitter((6.0, 6.0, 6.0))))
    eye = (0.4, 2.4, 5.5)
    js = scenes.export_json_obj(b, tmp_path, w, h, eye, (0, 1, 0), (0, 1, 0), 42.0)
    scenes.write_vol(tmp_path / "d.vol", dens, (0, 0, 0), (1, 1, 1))  # (the files' own bbox is not the one rendered)
    scenes.write_vol(tmp_path / "t.vol", temp, (0, 0, 0), (1, 1, 1))
    pngs = {}
    for flag in (True, False):
        out = tmp_path / f"out_{flag}.png"
        cmd = [str(PKG / "lib" / "glrt_main"), "-i", str(js), "--max-depth", str(depth), "--frames", str(frames), "--out", str(out)]
        r = subprocess.run(cmd + (["--enable-volume"] if flag else []), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        assert ("volume: 16 x 16 x 16" in r.stdout) == flag
        pngs[flag] = np.asarray(Image.open(out))
    assert not np.array_equal(pngs[True], pngs[False])

    c2w, s2c = scenes.camera(eye, (0, 1, 0), (0, 1, 0), 42.0, w, h)
    params = scenes.make_params(c2w, s2c, w, h, depth, 1)
    d = gpu_device
    d.upload_scene(b.build())
    d.upload_volume(dens, temp, lo, hi)
    d.set_extensions(device.EXT_VOLUME)
    try:
        d.set_partition(0, 1, 16)
        d.resize(w, h)
        for f in range(frames):
            d.render(dict(params, seed=host.frame_seed(f), focal=0.0))  # absent focalLength parses as 0 (scene.cpp:71-74)
        d.sync()
        ref = d.resolve_rgba8(2.2, True)
    finally:
        d.set_extensions(0)
        d.upload_volume(None, None, (0, 0, 0), (1, 1, 1))
    assert np.array_equal(pngs[True], ref)
