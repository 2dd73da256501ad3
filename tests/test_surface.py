"""The surface index (rt4.h rt4_scene_surface_count / rt4_scene_surface) on the CPU: the flat numbering of everything
a G-buffer pixel can name, checked against the SceneDesc fields of the seven named scenes."""
import ctypes
from ctypes import byref, c_int32

import pytest

import denoise_ref

SCENES = ["sphere", "room", "tiger", "cylinder4d", "hypercube", "all_primitives", "tiger_two_mirrors"]
ERR_ARG = -1


def expected_surfaces(rt4, d):
    """[(kind, index, part)] in surface order, from the counts alone."""
    out = [(rt4.GROUP_SPACES, i, 0) for i in range(d.n_spaces)]
    out += [(rt4.GROUP_SPHERES, i, 0) for i in range(d.n_spheres)]
    out += [(rt4.GROUP_CYLINDERS, i, 0) for i in range(d.n_cylinders)]
    out += [(rt4.GROUP_CYLINDERS_UNION, i, k) for i in range(d.n_unions) for k in range(2)]
    out += [(rt4.GROUP_HYPERCUBE, i, k) for i in range(d.n_hypercubes) for k in range(8)]
    out += [(rt4.GROUP_TIGER, i, k) for i in range(d.n_tigers) for k in range(4)]
    return out


@pytest.mark.parametrize("name", SCENES)
def test_surface_numbering(rt4, name):
    scene = rt4.Scene.named(name)
    d = scene.desc
    want = expected_surfaces(rt4, d)
    mats = denoise_ref.surface_materials(d)
    assert rt4.lib.rt4_scene_surface_count(byref(d)) == scene.surface_count() == len(want) == len(mats) > 0
    for s, ((kind, index, part), m) in enumerate(zip(want, mats)):
        k, i, p, got = c_int32(-7), c_int32(-7), c_int32(-7), rt4.Material()
        err = ctypes.create_string_buffer(256)
        assert rt4.lib.rt4_scene_surface(byref(d), s, byref(k), byref(i), byref(p), byref(got), err, len(err)) == 0
        assert (k.value, i.value, p.value) == (kind, index, part), s
        assert bytes(got) == bytes(m), s  # the material, byte for byte
        info = scene.surface(s)
        assert (info["kind"], info["index"], info["part"]) == (kind, index, part)
        assert info["color"] == tuple(m.color) and info["glow"] == m.glow and info["refl_prob"] == m.refl_prob


def test_surface_counts_of_named_scenes(rt4):
    # spaces + spheres + cylinders + 2 unions + 8 hypercubes + 4 tigers
    assert rt4.Scene.builtin("sphere").surface_count() == 1 + 2
    assert rt4.Scene.builtin("room").surface_count() == 8 + 2
    assert rt4.Scene.builtin("tiger").surface_count() == 1 + 4
    assert rt4.Scene.builtin("cylinder4d").surface_count() == 1 + 2
    assert rt4.Scene.builtin("hypercube").surface_count() == 1 + 8
    assert rt4.Scene.named("all_primitives").surface_count() == 2 + 3 + 1 + 2 + 8 + 4
    assert rt4.Scene.named("tiger_two_mirrors").surface_count() == 3 + 4


@pytest.mark.parametrize("name", SCENES)
def test_surface_out_of_range(rt4, name):
    d = rt4.Scene.named(name).desc
    n = rt4.lib.rt4_scene_surface_count(byref(d))
    for bad in (-1, n):
        k = c_int32(-7)
        err = ctypes.create_string_buffer(256)
        assert rt4.lib.rt4_scene_surface(byref(d), bad, byref(k), None, None, None, err, len(err)) == ERR_ARG
        assert k.value == -7 and err.value  # nothing written, a message
        with pytest.raises(rt4.RT4Error):
            rt4.Scene(d).surface(bad)


def test_surface_null_outputs_and_untested_objects(rt4):
    d = rt4.Scene.builtin("sphere").desc
    assert rt4.lib.rt4_scene_surface(byref(d), 0, None, None, None, None, None, 0) == 0
    # the numbering follows the arrays, whether or not a group uses the object
    d2 = rt4.SceneDesc.from_buffer_copy(bytes(d))
    d2.n_groups = 1  # only the spaces group is left
    assert rt4.lib.rt4_scene_surface_count(byref(d2)) == rt4.lib.rt4_scene_surface_count(byref(d))
    assert rt4.lib.rt4_scene_surface_count(None) == 0


def test_denoise_params_default(rt4):
    p = rt4.denoise_params()
    assert (p.levels, p.cos_min, p.depth_tol, p.max_refl_prob) == (3, ctypes.c_float(0.9).value, ctypes.c_float(0.1).value, 0.5)
    assert rt4.denoise_params(levels=5, cos_min=1.0).levels == 5
    assert rt4.GBUFFER_DTYPE.itemsize == 32 == ctypes.sizeof(rt4.GBufferPx)
