"""The kernels against shader_f64.py, the independent float64 restatement of executable/shader.frag (run on the GPU
box: pytest -m gpu).

Every other GPU test compares the kernel with the CPU oracle, bit for bit; the oracle was written from the same reading
of the shader as the kernel. Here the hot path itself meets the second reading (test_shader_f64.py has the cases, the
masks, the caps and the bounds, all from the reference alone, and runs the oracle against them on the CPU):

  * rt4_debug_find_intersection on the specialised and on the generic kernel: hit flag, winner, glow and refl_prob
    equal, distance and normal within the case's bound, on the rays the reference keeps;
  * two 36x20 frames (2 spp, 3 bounces; the second with another seed, blended with part = 0.5) with the sampler table,
    the inline sampler, primary reuse and the generic kernel: colour within the case's bound on the kept pixels, and
    the find_intersection count (the kernel reports the image's total);
  * the primary-hit G-buffer against the reference's primary hit.

The new scenes of test_shader_f64.py are in no other GPU test, so they are also compared with the oracle bit for bit.
The references are computed once per case and shared; nothing outside the repository is read.
"""
import numpy as np
import pytest

import scene_builder as sb
import shader_f64 as sf
import test_shader_f64 as cpu
from test_gpu_parity import assert_bits

pytestmark = pytest.mark.gpu

_tracers = {}
_scenes = {}


@pytest.fixture(scope="module")
def tracer_of(rt4):
    """One context per flag word for the whole module (the scene is set per case; setting a scene seen before costs
    only the upload)."""
    def get(flags, scene):
        t = _tracers.get(flags)
        if t is None:
            t = _tracers[flags] = rt4.Tracer(device=0, flags=flags)
        t.set_scene(scene)
        return t

    yield get
    for t in _tracers.values():
        t.close()
    _tracers.clear()


def scene_of(rt4, name):
    if name not in _scenes:
        _scenes[name] = rt4.Scene(cpu.case_of(rt4, name)["desc"])
    return _scenes[name]


def render_modes(rt4):
    return {"lut": rt4.FLAG_SAMPLER_LUT, "inline": 0, "reuse": rt4.FLAG_SAMPLER_LUT | rt4.FLAG_PRIMARY_REUSE,
            "generic": rt4.FLAG_GENERIC_KERNEL}


@pytest.mark.parametrize("name", cpu.RAY_CASES + sb.SIMPLE_CASES)
def test_find_intersection(rt4, oracle, tracer_of, name):
    ref = cpu.ray_reference(rt4, name)
    cpu.check_ray_reference(name, ref)
    rays = cpu.case_of(rt4, name)["rays"]
    for flags in (0, rt4.FLAG_GENERIC_KERNEL):
        t = tracer_of(flags, scene_of(rt4, name))
        if flags:
            assert t.kernel_shape == sb.GENERIC
        got, got_col = t.debug_find_intersection(rays)
        cpu.check_rays(name, ref, got, got_col, f"kernel {t.kernel_shape:#x}")
        if name in cpu.NEW_SCENES:
            want, want_col = oracle.find_intersection(scene_of(rt4, name).desc, rays)
            assert_bits(got, want, f"{name} find_intersection flags={flags}")
            assert_bits(got_col, want_col, f"{name} material colour flags={flags}")


RENDERS = [(n, m) for n in cpu.PIXEL_CASES for m in ("lut", "inline", "reuse", "generic")]


@pytest.mark.parametrize("name,mode", RENDERS, ids=[f"{n}-{m}" for n, m in RENDERS])
def test_render(rt4, tracer_of, name, mode):
    ref = cpu.pixel_reference(rt4, name)
    cpu.check_pixel_reference(name, ref)
    t = tracer_of(render_modes(rt4)[mode], scene_of(rt4, name))
    if mode == "generic":
        assert t.kernel_shape == sb.GENERIC
    reg = rt4.region(cpu.WIDTH, cpu.HEIGHT)
    frame = np.zeros((cpu.HEIGHT, cpu.WIDTH, 4), np.float32)
    for k, u in enumerate(cpu.frame_uniforms(rt4, name)):
        total = t.render_host(u, reg, frame)
        cpu.check_frame(name, ref, k, frame, f"kernel {t.kernel_shape:#x} {mode}", total=total)


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("name", cpu.PIXEL_CASES)
def test_gbuffer(rt4, tracer_of, name, generic):
    ref = cpu.pixel_reference(rt4, name)
    cpu.check_pixel_reference(name, ref)
    f = ref["frames"][0]
    t = tracer_of(rt4.FLAG_GENERIC_KERNEL if generic else 0, scene_of(rt4, name))
    got = t.render_gbuffer_host(cpu.frame_uniforms(rt4, name)[0], rt4.region(cpu.WIDTH, cpu.HEIGHT))
    keep = ~f["primary_ambiguous"]
    hit, miss = keep & f["hit"], keep & ~f["hit"]
    assert hit.sum() >= cpu.MIN_WINS and (name == "room" or miss.sum() >= cpu.MIN_WINS)
    assert np.array_equal(got["surface"][keep], f["surface"][keep]), name
    assert (got["surface"][miss] == -1).all() and (got["depth"][miss] == np.inf).all()
    assert not cpu.bits(got["normal"][miss]).any()  # +0.0 four times
    assert not cpu.bits(got["glow"][miss]).any() and not cpu.bits(got["refl_prob"][miss]).any()
    assert np.array_equal(cpu.bits(got["glow"][hit]), cpu.bits(f["glow"][hit]))
    assert np.array_equal(cpu.bits(got["refl_prob"][hit]), cpu.bits(f["refl_prob"][hit]))
    e_depth = (np.abs(got["depth"][hit].astype(np.float64) - f["depth"][hit]) / np.maximum(1.0, f["depth"][hit])).max()
    well = hit & ~sf.ill_conditioned(f["primary_cond"])
    e_normal = np.abs(got["normal"][well].astype(np.float64) - f["normal"][well]).max()
    print(f"{name}: depth error {e_depth:.2e} (bound {4 * ref['e_depth']:.2e}) normal error {e_normal:.2e} "
          f"(bound {4 * ref['e_normal']:.2e})")
    assert e_depth <= 4 * ref["e_depth"] and e_normal <= 4 * ref["e_normal"]
