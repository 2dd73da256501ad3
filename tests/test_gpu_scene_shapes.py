"""Composed scenes on the kernels the named scenes never reach, against the CPU oracle, bit for bit (run on the
GPU box: pytest -m gpu).

The seven named scenes run on kernels compiled for their exact object counts. A scene with other counts runs on one
of the six runtime-count kernels (rt4_trace.hip kVariants: the for_count<0> loops, prim_bases read from SceneAux,
the LDS table of MAX_PRIMS entries, the pending-sphere mask up to bit 31, the deferred tiger test with runtime
counts, the REFILL_MIN threshold), and a scene whose group list is not shader.frag's canonical one (outer = false,
closest(inter, new), sub-ranges, a kind twice, another order, several composites of a kind, a kind set without a
variant) on the generic find_intersection. scene_builder.CASES holds such scenes; every test here first asserts
the kernel_shape the scene is meant to reach, then compares find_intersection rows, material colours, images and
intersection counts (NaN equal to NaN, as everywhere in the suite). test_scene_shapes.py shows from the oracle
that every tested object of every case wins rays and that the images have hits and sky tiles.
"""
import numpy as np
import pytest

import scene_builder as sb
from test_gpu_parity import assert_bits
from test_gpu_refill_edges import gpu_frames, same_bits

pytestmark = pytest.mark.gpu

SPP, BOUNCES, WIDTH, HEIGHT = 3, 4, 64, 40
FRAMES_REGION = (67, 9)  # 18 tiles: a four-tile claim straddles the frame boundary, partial tiles on the right

_tracers = {}
_cases = {}
_oracle = {}


@pytest.fixture(scope="module")
def tracer_of(rt4):
    """One context per flag word for the whole module (the scene is set per case)."""
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


def case_of(rt4, name):
    """(Scene, rays, expected kernel_shape) of a case, built once."""
    if name not in _cases:
        d, rays = sb.case_scene_and_rays(rt4, name)
        _cases[name] = (rt4.Scene(d), rays, sb.CASES[name][0])
    return _cases[name]


def oracle_once(key, compute):
    if key not in _oracle:
        _oracle[key] = compute()
    return _oracle[key]


def render_modes(rt4):
    return {"lut": rt4.FLAG_SAMPLER_LUT, "inline": 0, "reuse": rt4.FLAG_SAMPLER_LUT | rt4.FLAG_PRIMARY_REUSE,
            "generic": rt4.FLAG_GENERIC_KERNEL}


@pytest.mark.parametrize("name", list(sb.CASES))
def test_find_intersection(rt4, oracle, tracer_of, name):
    """About 20000 aimed and background rays on the scene's own kernel and on the generic one."""
    scene, rays, shape = case_of(rt4, name)
    want, want_col = oracle_once((name, "find"), lambda: oracle.find_intersection(scene.desc, rays))
    for flags, expect in ((0, shape), (rt4.FLAG_GENERIC_KERNEL, sb.GENERIC)):
        t = tracer_of(flags, scene)
        assert t.kernel_shape == expect, f"{name}: kernel_shape {t.kernel_shape:#x}, expected {expect:#x}"
        got, got_col = t.debug_find_intersection(rays)
        assert_bits(got, want, f"{name} find_intersection flags={flags}")
        assert_bits(got_col, want_col, f"{name} material colour flags={flags}")


RENDERS = ([(n, m) for n in sb.RUNTIME_CASES for m in ("lut", "inline", "reuse", "generic")]
           + [(n, m) for n in sb.GENERIC_CASES for m in ("lut", "inline")])


@pytest.mark.parametrize("name,mode", RENDERS, ids=[f"{n}-{m}" for n, m in RENDERS])
def test_render(rt4, oracle, tracer_of, name, mode):
    """A 64x40 image, 3 spp, 4 bounces, into a counter that starts nonzero: sampler table, inline sampler, and for
    the runtime-count kernels primary reuse (evaluated calls = count - (spp - 1) per pixel) and the generic kernel."""
    scene, _, shape = case_of(rt4, name)
    flags = render_modes(rt4)[mode]
    reg = rt4.region(WIDTH, HEIGHT)
    u = sb.case_uniforms(rt4, name, WIDTH, HEIGHT, SPP, BOUNCES, seed=31)
    want, n_want = oracle_once((name, "render"), lambda: oracle.render_fmt(scene.desc, u, reg, rt4.FRAME_RGBA32F, threads=4))
    t = tracer_of(flags, scene)
    expect = sb.GENERIC if mode == "generic" else shape
    assert t.kernel_shape == expect, f"{name}: kernel_shape {t.kernel_shape:#x}, expected {expect:#x}"
    if mode == "reuse":
        t.evaluated()  # reset
    got, n_got = gpu_frames(rt4, t, [u], reg)
    assert n_got == n_want, f"{name} {mode}"
    assert same_bits(got, want), f"{name} {mode} image"
    if mode == "reuse":
        assert t.evaluated() == n_want - (SPP - 1) * WIDTH * HEIGHT


@pytest.mark.parametrize("name", sb.FRAMES_CASES)
def test_pipelined_frames(rt4, oracle, tracer_of, name):
    """Three progressive frames in one rt4_render_frames_device call on the 67x9 region, against the oracle's three
    frames blended in turn; each frame has its own seed and part."""
    scene, _, shape = case_of(rt4, name)
    w, h = FRAMES_REGION
    reg = rt4.region(w, h)
    base = sb.case_uniforms(rt4, name, w, h, SPP, BOUNCES, seed=77)
    us = [rt4.progressive_uniforms(base, n) for n in range(1, 4)]
    want, n_want = np.zeros((h, w, 4), np.float32), 0
    for u in us:
        _, k = oracle.render_fmt(scene.desc, u, reg, rt4.FRAME_RGBA32F, frame=want, threads=4)
        n_want += k
    t = tracer_of(rt4.FLAG_SAMPLER_LUT, scene)
    assert t.kernel_shape == shape, f"{name}: kernel_shape {t.kernel_shape:#x}, expected {shape:#x}"
    got, n_got = gpu_frames(rt4, t, us, reg)
    assert n_got == n_want, name
    assert same_bits(got, want), f"{name} three pipelined frames"
