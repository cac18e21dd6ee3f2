"""The shading mode of a render (ShadeMode in csrc/pt_types.h, decided by render_mode in csrc/pt_render.cpp): environment importance
sampling, participating media, exact light sampling and spectral dispersion exclude each other. One small scene in which each of the
four can be put in effect; every subset of two or more is refused with the whole message of the first pair the render checks, every
single feature renders. The feature suites match substrings of these messages; this pins the texts and their precedence.

The six texts are written out here, in the order of the checks."""
import itertools

import numpy as np
import pytest

from common import SceneSpec, default_camera

pytestmark = pytest.mark.gpu

FEATURES = ("env", "media", "lights", "dispersion")
REFUSALS = [   # (the pair, pt_render's message), in the order the render checks them
    ({"media", "env"}, "pt_render: environment importance sampling together with participating media is not supported (set one of them off)"),
    ({"lights", "env"}, "pt_render: exact light sampling together with environment importance sampling is not supported (set one of them off)"),
    ({"lights", "media"}, "pt_render: exact light sampling together with participating media is not supported (set light sampling to 0 or take the media out)"),
    ({"dispersion", "env"}, "pt_render: spectral dispersion together with environment importance sampling is not supported (set one of them off)"),
    ({"dispersion", "media"},
     "pt_render: spectral dispersion together with participating media or a glass interior is not supported (clear the dispersion or take the media out)"),
    ({"dispersion", "lights"}, "pt_render: spectral dispersion together with exact light sampling is not supported (set one of them off)"),
]
SUBSETS = [c for n in (1, 2, 3, 4) for c in itertools.combinations(FEATURES, n)]
assert len(SUBSETS) == 15 and sum(len(c) >= 2 for c in SUBSETS) == 11


@pytest.fixture(scope="module")
def scene(pt, ctx):
    """16 x 16 pixels: a glass ball on a floor under a sphere light and a 4 x 2 float environment map; a fog material nothing carries."""
    spec = SceneSpec()
    env = np.array([[[4.0, 3.0, 2.0], [0.5, 0.5, 0.5], [0.25, 0.5, 1.0], [1.0, 1.0, 1.0]],
                    [[0.1, 0.1, 0.1], [0.2, 0.1, 0.0], [0.0, 0.0, 0.0], [0.1, 0.2, 0.1]]], dtype=np.float32)
    tex = spec.add("tex_image_rgbf32", env)
    floor = spec.add("mat_diffuse", spec.add("tex_solid_rgb", 0.6, 0.6, 0.6), -1)
    glass = spec.add("mat_glass", spec.add("tex_solid_rgb", 1.0, 1.0, 1.0), spec.add("tex_solid_f", 0.05), 0.0, 1.5)
    fog = spec.add("mat_medium", 0.05, (0.9, 0.9, 0.9), 0.2)
    spec.add("world_add_object", spec.add("quad", (-8.0, 0.0, -8.0), (0.0, 0.0, 16.0), (16.0, 0.0, 0.0), floor))
    spec.add("world_add_object", spec.add("sphere", 1.0, (0.0, 1.0, 0.0), (0.0, 1.0, 0.0), glass))
    spec.add("world_add_light", spec.add("sphere", 0.3, (2.0, 3.0, 0.0), (2.0, 3.0, 0.0), spec.add("mat_light", spec.add("tex_solid_rgb", 9.0, 8.0, 7.0))))
    spec.add("world_build")
    spec.camera = default_camera(width=16, spp=1, defocus_angle=0.0, env_is_map=1, env_tex=tex)
    gs = pt.Scene(ctx)
    res = spec.replay(gs)
    yield gs, spec.make_camera(pt.Camera, res), res[glass], res[fog]
    gs.close()


def put_in_effect(scene, on):
    gs, _, glass, fog = scene
    gs.set_env_sampling(0.5 if "env" in on else 0.0)
    gs.set_camera_medium(fog if "media" in on else -1)
    gs.set_light_sampling("exact" if "lights" in on else "reference")
    gs.mat_glass_set_dispersion(glass, 30.0 if "dispersion" in on else 0.0)
    gs.world_build()


@pytest.mark.parametrize("on", SUBSETS, ids="+".join)
def test_one_feature_renders_and_two_are_refused_by_name(pt, scene, on):
    gs, cam = scene[:2]
    put_in_effect(scene, on)
    want = next((text for pair, text in REFUSALS if pair <= set(on)), None)
    if want is None:
        assert len(on) == 1
        acc, stats = gs.render(cam, 1, 0, 1)
        assert stats.samples == 16 * 16 and np.isfinite(acc).any()
        return
    with pytest.raises(pt.PtError) as err:
        gs.render(cam, 1, 0, 1)
    assert str(err.value) == "pt_render: " + want   # (the binding puts the entry point's name in front of pt_last_error's text)
    assert pt.lib.pt_last_error().decode() == want
