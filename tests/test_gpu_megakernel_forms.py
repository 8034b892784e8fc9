"""The persistent megakernel's table (csrc/glrtx.hip: kPersistent[form][count_rays]) walked in full: each of the eighteen forms of pt_render_persistent that
are launched, once without ray counting and once with it, under the name the route statement (host.launch_route) gives the form.  The two instantiations of a form differ in nothing but the counting, so the two images are equal bit
for bit, the counter stays at zero in one launch and moves in the other -- a transposed or shifted row of the table shows in one of the three.  What each form
computes is pinned by the texture, maps, cutout, emission, environment, volume and parity tests; here each form gets the least that reaches it."""
import numpy as np
import pytest

from conftest import assert_bit_equal
from glrt_amd import device, host, scenes
from test_gpu_maps import FLAT, _flat_everywhere, _none, _types

pytestmark = pytest.mark.gpu

W, H = 37, 19  # partial 8x8 tiles on both edges
FORMS = {  # what is bound: ext(ension flag), vol(ume), tex(ture set), maps, env(ironment), cut(outs), emit (emission maps)
    "plain": (), "ext": ("ext",), "volume": ("vol",), "tex": ("tex",), "tex+volume": ("tex", "vol"), "tex+maps": ("tex", "maps"),
    "tex+volume+maps": ("tex", "vol", "maps"), "env": ("env",), "env+tex": ("env", "tex"), "env+tex+maps": ("env", "tex", "maps"),
    "tex+cut": ("tex", "cut"), "tex+maps+cut": ("tex", "maps", "cut"), "env+tex+cut": ("env", "tex", "cut"), "env+tex+maps+cut": ("env", "tex", "maps", "cut"),
    "tex+emit": ("tex", "emit"), "tex+maps+emit": ("tex", "maps", "emit"), "env+tex+emit": ("env", "tex", "emit"), "env+tex+maps+emit": ("env", "tex", "maps", "emit"),
}


def _kernel_name(bound):
    """The statement's name for the launch of a variant-1 context with this bound."""
    route, refusal = host.launch_route(dict(variant=1, ext_flags=(device.EXT_WHITTED if "ext" in bound else 0) | (device.EXT_VOLUME if "vol" in bound else 0),
                                            have_volume="vol" in bound, n_tex=2 * ("tex" in bound), have_maps="maps" in bound, have_cut="cut" in bound,
                                            have_emit="emit" in bound, have_env="env" in bound, max_depth=3, n_samples=2))
    assert refusal == "", refusal
    return route.kernel.decode()


@pytest.fixture(scope="module")
def dev(gpu_device):
    d = device.Device()
    yield d
    d.close()


@pytest.mark.parametrize("form", list(FORMS))
def test_each_form_renders_the_same_image_with_and_without_ray_counting(dev, form):
    bound = FORMS[form]
    scene, params = scenes.config_c1(W, H, max_depth=3, n_samples=2, subdiv=1)
    d = dev
    d.set_variant(1); d.track_motion(False)
    d.upload_scene(scene); d.upload_spheres(None); d.resize(W, H)
    try:
        d.set_extensions((device.EXT_WHITTED if "ext" in bound else 0) | (device.EXT_VOLUME if "vol" in bound else 0))
        if "vol" in bound:
            grid = np.linspace(0.5, 1.5, 64, dtype=np.float32).reshape(4, 4, 4)
            d.upload_volume(grid, 1000.0 * grid, (-1, 0, -1), (1, 2, 1))
        if "tex" in bound:
            albedo = _none(scene)
            albedo[int(np.flatnonzero(_types(scene) == 2)[0])] = 1
            d.upload_textures([FLAT, (np.linspace(0.1, 0.9, 48, dtype=np.float32).reshape(4, 4, 3), "rgba32f", "repeat", "bilinear")], albedo)
        if "maps" in bound:
            d.bind_material_maps(normal=_flat_everywhere(scene))
        if "cut" in bound:
            cut = _none(scene)
            cut[int(np.flatnonzero(_types(scene) == 2)[0])] = 0
            d.bind_cutouts(texture=cut)
        if "emit" in bound:
            emit = _none(scene)
            emit[int(np.flatnonzero(_types(scene) == 1)[0])] = 0
            d.bind_emission_maps(emit)
        if "env" in bound:
            d.upload_environment((scenes.env_octant_map(), "rgba32f", "bilinear"), host.env_cfg("escape"))
        images = []
        for count in (False, True):
            d.count_rays(count); d.clear(); d.reset_stats()
            d.render(params); d.sync()
            st = d.stats()
            assert st.variant_last == 1, (form, count, st.variant_last)
            assert d.last_kernel() == _kernel_name(bound), (form, count)
            assert (st.rays > 0) if count else (st.rays == 0), (form, count, st.rays)
            images.append(d.read_accum())
        assert_bit_equal(images[1], images[0], f"{form}: with against without ray counting")
    finally:
        d.upload_environment(None); d.upload_textures(None, None); d.set_extensions(0); d.upload_volume(None, None, (0, 0, 0), (1, 1, 1)); d.count_rays(True)
