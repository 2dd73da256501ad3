"""The trace kernels' final_light (rt4_trace.hip) on the MI355X against the oracle's, bit for bit, on directions aimed at
the boundaries of its three shortcuts (final_light_cases.py; the CPU side is test_final_light.py).

a. rt4_debug_final_light, which calls the kernels' own device function, on every sun and every direction set.
b. rt4_debug_sky_threshold against the sweep of the oracle's acos: c* is the CPU's definition, not only the device's.
c. Renders whose 512 columns cross the sun's rim in steps of 2e-6 rad, through the real trace kernels: the debug kernel
   shares the device function, not the inlining context.
d. The argument errors of the new entry point write nothing.

Branches the inputs of (a) take, of 917 546 directions per sun (from the oracle's output and the fp32 predicates of
final_light_cases.py; the tables NO_PRETEST, NO_THRESHOLD_ONLY and NO_IN_SUN name the suns whose scene empties one):
  sun            pre-test  threshold only   in sun      sun            pre-test  threshold only   in sun
  ref_sphere      488376       154624       273694      drct_0110       474143       184482       258023
  ref_tiger       488616       153814       274212      drct_1234       494297       193242       229060
  ref_hypercube   488685       153858       274167      drct_3040       486161       185374       245086
  ang_1e-3        629756       213399        73650      len_2^-22       180158       466156       270321
  ang_0.02        558071       192905       165676      len_2^22        180177       465695       270752
  ang_0.3         479766       172541       264270      k_low_in        484049       199727       232831
  ang_1.0         433000       162772       321100      k_high_in       485999       163915       266700
  ang_1.5         457615       118887       340449      sharp_0         474719       184376       257622
  ang_pio2_dn     396654       160658       359816      sharp_0.7       474209       184526       257921
  ang_pio2_up     492238        56534       368496      sharp_1.0       474481       184544       257629
  ang_3.2              0          686       916856      sharp_1.5       473974       183831       258926
Divisors: of the 366 candidates the device refuses all but 1/32, 1/16, 1/8, 1/4, 1/2, 1, 1.25, 1.5 and 2 (the 3-op form
misses quotients in the subnormal range), so every sun above but ang_1.5 divides by its size in IEEE form, and by its
length unless that is 1; test_slow_divisor_suns uses 3/64 (refused) and 1.25 (accepted) as size and as length.

Hand mutations of rt4_trace.hip on scratch builds, the whole gpu suite against each (MI355X):
  1. sky_pre_k with (1 + 1e-5): 32 tests of this file fail (a on every sun with a sky_pre_k, the slow divisors, every
     render of c through the mutated library); of the earlier suite the four 1080p frames of test_gpu_configs,
     test_render_bitwise_config3_rows (one pixel) and test_gpu_scene_shapes test_render[unions_2-*].
  2. sky_c_star without nextafter: 16 tests of (a) and the slow divisors fail (where a v_cos equals the smallest c); of
     the earlier suite the four 1080p frames of test_gpu_configs.
  3. no guard on l2: nothing fails, here or elsewhere: the guard changes no result (test_final_light.py, b).
  4. deviation * (1 / ang) for the verified quotient: 30 tests of this file and 201 of the earlier suite fail.
"""
import ctypes
import os

import numpy as np
import pytest

import final_light_cases as fc
import shader_f64 as sf
from test_gpu_codegen import BUILDS

pytestmark = pytest.mark.gpu

f32 = np.float32
MIN_BRANCH = 1000
GENERIC_SUNS = ("ref_sphere", "ang_1.5", "k_low_in")


@pytest.fixture(scope="module")
def tracer_generic(rt4):
    t = rt4.Tracer(device=0, flags=rt4.FLAG_GENERIC_KERNEL)
    yield t
    t.close()


def _compare(rt4, oracle, t, scene, name, sets):
    """debug_final_light == oracle on every set; the branch counts (pre-test, threshold only, in sun) of the inputs."""
    d = scene.desc
    t.set_scene(scene)
    ax = fc.aux(oracle, d)
    counts = np.zeros(3, np.int64)
    for what, v in sets.items():
        want = oracle.final_light(d, v)
        got = t.debug_final_light(v)
        same = fc.same_bits(got, want).all(axis=1)
        assert same.all(), (name, what, int((~same).sum()), v[~same][0], got[~same][0], want[~same][0])
        if d.final_light_mode == rt4.FINAL_LIGHT_SUN_SKY:
            counts += [int(b.sum()) for b in fc.branches(d, ax, v, want)]
    return counts


def _assert_branches(name, counts):
    for q, (what, empty) in enumerate((("pre-test", fc.NO_PRETEST), ("threshold only", fc.NO_THRESHOLD_ONLY),
                                       ("in sun", fc.NO_IN_SUN))):
        if name not in empty:
            assert counts[q] >= MIN_BRANCH, (name, what, counts.tolist())


@pytest.mark.parametrize("name", fc.SUN_NAMES)
def test_final_light_matches_oracle(rt4, oracle, tracer, name):
    scene = fc.scene(rt4, name)
    counts = _compare(rt4, oracle, tracer, scene, name, fc.directions(scene.desc, name))
    print(f"  {name}: pre-test / threshold only / in sun = {counts.tolist()}")
    _assert_branches(name, counts)


@pytest.mark.parametrize("name", GENERIC_SUNS)
def test_final_light_matches_oracle_generic_kernel(rt4, oracle, tracer_generic, name):
    scene = fc.scene(rt4, name)
    _assert_branches(name, _compare(rt4, oracle, tracer_generic, scene, name, fc.directions(scene.desc, name)))


def test_slow_divisor_suns(rt4, oracle, tracer):
    """Suns whose angular size or length is refused as a verified divisor (the IEEE quotient runs instead of the 3-op
    form), next to accepted ones, both found on the device in the committed candidate list."""
    bad = [tracer.debug_verify_div(b) != 0 for b in fc.DIV_CANDIDATES]
    refused = [b for b, x in zip(fc.DIV_CANDIDATES, bad) if x]
    accepted = [b for b, x in zip(fc.DIV_CANDIDATES, bad) if not x]
    print(f"  divisors refused: {len(refused)} of {len(bad)}; accepted: {accepted}")
    assert refused and accepted
    # an accepted divisor that is no power of two, if there is one: its reciprocal is rounded
    refused, accepted = refused[0], ([b for b in accepted if np.frexp(b)[0] != 0.5] or accepted)[0]
    print(f"  suns from the refused {refused!r} and the accepted {accepted!r}")
    for tag, ang, ln in (("slow_ang", refused, accepted), ("slow_len", accepted, refused), ("slow_both", refused, refused),
                         ("fast_both", accepted, accepted)):
        scene = fc.scene(rt4, tag, ang=ang, drct=(ln, 0.0, 0.0, 0.0))
        sets = fc.directions(scene.desc, tag, ("rim", "pretest", "circle", "specials"))
        _assert_branches(tag, _compare(rt4, oracle, tracer, scene, tag, sets))


@pytest.mark.parametrize("name", [n for n in fc.SUN_NAMES if n not in fc.CONSTANT_MODE])
def test_sky_threshold_is_the_oracles(rt4, oracle, tracer, name):
    ang = fc.scene(rt4, name).desc.sun.angular_size
    want = fc.c_min_sweep(oracle, ang)
    got = f32(tracer.debug_sky_threshold(ang, full=ang > 1.0))
    assert got.view(np.uint32) == want.view(np.uint32), (name, ang, got, want)


# ------------------------------------------------------------------------------ renders across the rim
W, H, STEP = 512, 8, 2e-6
_render_cache = {}


def _rim_view(rt4, oracle, name):
    """(scene, uniforms, region, oracle frame, oracle count) of a camera high above the scene that looks at the sun's
    rim: vec_to_mtr is the unit vector at angle ang from the sun, right_drct points at the sun's centre."""
    if name in _render_cache:
        return _render_cache[name]
    scene = fc.scene(rt4, name)
    d = scene.desc
    s = np.array(list(d.sun.drct), np.float64)
    s /= np.linalg.norm(s)
    p = np.array([1.0, 0.0, 0.0, 0.0])
    p -= (p @ s) * s
    p /= np.linalg.norm(p)
    ang = float(d.sun.angular_size)
    fwd = np.cos(ang) * s + np.sin(ang) * p
    right = np.sin(ang) * s - np.cos(ang) * p
    top = np.array([0.0, 0.0, 0.0, 1.0]) - (np.array([0.0, 0.0, 0.0, 1.0]) @ s) * s
    top -= (top @ p) * p
    top /= np.linalg.norm(top)
    u = rt4.make_uniforms(W, H, samples=1, reflections=0, seed=99, k=1.0 / 64.0, focus=(0.0, 0.0, 1000.0, 0.0))
    u.mtr_sizes[0], u.mtr_sizes[1] = W * STEP, H * STEP
    for q in range(4):
        u.vec_to_mtr[q], u.top_drct[q], u.right_drct[q] = fwd[q], top[q], right[q]
    reg = rt4.region(W, H)
    # conditions, from the oracle and the float64 reference alone
    sx = (np.arange(W) + 0.5) / W
    sy = (np.arange(H) + 0.5) / H
    mx, my = (sx - 0.5) * (W * STEP), (0.5 - sy) * (H * STEP)
    dirs = (np.array(list(u.right_drct), np.float64)[None, None] * mx[None, :, None]
            + np.array(list(u.top_drct), np.float64)[None, None] * my[:, None, None]
            + np.array(list(u.vec_to_mtr), np.float64)[None, None]).reshape(-1, 4)
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    rays = np.concatenate([np.tile(np.array(list(u.focus), np.float64), (len(dirs), 1)), dirs], axis=1).astype(f32)
    hit, _ = oracle.find_intersection(d, rays)
    assert not hit[:, 0].any()
    _, in_sun = sf.final_light(d, dirs, np.float64)
    cols = in_sun.reshape(H, W)
    assert cols.all(axis=0).mean() >= 0.40 and (~cols).all(axis=0).mean() >= 0.40
    frame, n, _, _ = oracle.render(d, u, reg, np.full((H, W, 4), 0.25, f32))
    assert n == W * H
    assert len(np.unique(frame.reshape(-1, 4).view(np.uint32), axis=0)) >= 100
    _render_cache[name] = (scene, u, reg, frame, n)
    return _render_cache[name]


def _equal(fg, ng, fc_, nc):
    assert ng == nc
    assert np.array_equal(fg.view(np.uint32), fc_.view(np.uint32)), f"{int(np.sum(np.any(fg != fc_, axis=2)))} pixels differ"


@pytest.mark.parametrize("how", ["lut", "inline", "generic", "reuse"])
@pytest.mark.parametrize("name", ["ref_sphere", "ang_1.0"])
def test_rim_render_bitwise(rt4, oracle, name, how):
    scene, u, reg, want, n = _rim_view(rt4, oracle, name)
    flags = {"lut": rt4.FLAG_SAMPLER_LUT, "inline": 0, "generic": rt4.FLAG_GENERIC_KERNEL,
             "reuse": rt4.FLAG_SAMPLER_LUT | rt4.FLAG_PRIMARY_REUSE}[how]
    t = rt4.Tracer(device=0, flags=flags, scene=scene)
    try:
        fg = np.full((H, W, 4), 0.25, f32)
        ng = t.render_host(u, reg, fg)
    finally:
        t.close()
    _equal(fg, ng, want, n)


@pytest.mark.parametrize("build", sorted(BUILDS))
@pytest.mark.parametrize("name", ["ref_sphere", "ang_1.0"])
def test_rim_render_stress_builds(rt4, oracle, name, build):
    if not os.path.exists(BUILDS[build]):
        pytest.fail(f"{BUILDS[build]} not built (make -C 4d_ray_tracing_amd/csrc all)")
    scene, u, reg, want, n = _rim_view(rt4, oracle, name)
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=scene, library=rt4.load_variant(BUILDS[build]))
    try:
        fg = np.full((H, W, 4), 0.25, f32)
        ng = t.render_host(u, reg, fg)
    finally:
        t.close()
    _equal(fg, ng, want, n)


@pytest.mark.parametrize("name", ["ref_sphere", "ang_1.0"])
def test_rim_render_two_frames(rt4, oracle, name):
    import torch

    scene, u, reg, _, _ = _rim_view(rt4, oracle, name)
    us = [rt4.progressive_uniforms(u, f + 1) for f in range(2)]
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=scene)
    try:
        frame = torch.full((H, W, 4), 0.25, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        t.render_frames_device(us, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, cnt.data_ptr())
        torch.cuda.synchronize()
        fg, ng = frame.cpu().numpy(), int(cnt.item())
    finally:
        t.close()
    want, n = np.full((H, W, 4), 0.25, f32), 0
    for uf in us:
        want, k, _, _ = oracle.render(scene.desc, uf, reg, want)
        n += k
    _equal(fg, ng, want, n)


def test_rim_render_half_frame(rt4, oracle):
    scene, u, reg, _, n = _rim_view(rt4, oracle, "ref_sphere")
    want, nc = oracle.render_fmt(scene.desc, u, reg, rt4.FRAME_RGBA16F, frame=np.full((H, W, 4), 0.25, np.float16))
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=scene)
    try:
        fg = np.full((H, W, 4), 0.25, np.float16)
        ng = t.render_host_ex(u, reg, fg, rt4.FRAME_RGBA16F)
    finally:
        t.close()
    assert ng == nc == n
    assert np.array_equal(fg.view(np.uint16), want.view(np.uint16))
    assert len(np.unique(want.reshape(-1, 4).view(np.uint16), axis=0)) >= 100


# ------------------------------------------------------------------------------ argument errors
def test_argument_errors_write_nothing(rt4, tracer):
    tracer.set_scene(fc.scene(rt4, "ref_sphere"))
    v = np.ones((4, 4), f32)
    out = np.full((4, 3), 7.0, f32)
    err = ctypes.create_string_buffer(256)
    call = rt4.lib.rt4_debug_final_light
    vp, op = ctypes.c_void_p(v.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    assert call(None, vp, op, 4, err, len(err)) == -1
    assert call(tracer._h, None, op, 4, err, len(err)) == -1
    assert call(tracer._h, vp, None, 4, err, len(err)) == -1
    assert call(tracer._h, vp, op, -1, err, len(err)) == -1 and err.value
    empty = rt4.Tracer(device=0)
    try:
        assert call(empty._h, vp, op, 4, err, len(err)) == -1 and b"scene" in err.value
        assert call(empty._h, vp, op, 4, None, 0) == -1
    finally:
        empty.close()
    assert (out == 7.0).all()
    assert call(tracer._h, vp, op, 0, err, len(err)) == 0 and (out == 7.0).all()
    assert tracer.debug_final_light(v).shape == (4, 3)
