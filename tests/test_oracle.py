"""The CPU oracle against the known answers it can be pinned to (no GPU needed).

Pins: the reference ships no tests or golden data, and its GLSL cannot run here,
so against the GL reference itself images are "parity unpinned". What is pinned here:
  * integer RNG: hash() and the first rand() values of two pixels (tests/golden/kat.json)
  * S^3 sampler: w_by_volume known answers + the exhaustive 2^23-input sweep statistics
  * intersectors: closed-form geometry (distances, normals) for every primitive kind
  * image invariants: sky-only pixels, emissive direct hits, colour range, alpha
and in test_shader_f64.py, against an independent float64 restatement of the shader (shader_f64.py):
  * find_intersection of every kind, composites and their quirks included: hit flag, winner, glow and refl_prob
    equal, distance and normal within four times the restatement's own fp32-against-float64 difference
  * whole pixels: the random path (per-pixel find_intersection counts: the rand() order, the seed carried over
    bounces and samples, the row orientation) equal and the colour within the same kind of bound, over two
    blended frames
"""
import json
import math
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
KAT = json.load(open(os.path.join(GOLDEN, "kat.json")))


def test_hash_kat(oracle):
    for x, h in KAT["hash"].items():
        assert oracle.hash_u32(int(x)) == int(h, 16)


def test_first_rands_kat(oracle):
    r = KAT["rand_first4"]
    for key, (x, y) in (("pixel_0_0", (0, 0)), ("pixel_128_128", (128, 128))):
        got = oracle.rand_first(r["W"], r["H"], r["seed"], x, y, 4)
        np.testing.assert_array_equal(got, np.array(r[key], np.float32))


def test_w_by_volume_kat(rt4, oracle):
    for v, (w, iters) in KAT["w_by_volume"].items():
        got, it = oracle.eval_array(rt4.EVAL_W_BY_VOLUME, np.array([float(v)], np.float32))
        # the survey's values used glibc acosf; at v = 0 (w -> -1, where dv/dw -> 0) the Newton
        # inverse stops wherever |dw| < SMALL_FLOAT, so one ulp of acos moves w by ~4e-6 there
        tol = 1e-5 if float(v) == 0.0 else 2e-7
        assert abs(float(got[0]) - w) <= tol, (v, got)
        assert int(it[0]) == iters
    for w, vol in KAT["volume_by_w"].items():
        got, _ = oracle.eval_array(rt4.EVAL_VOLUME_BY_W, np.array([float(w)], np.float32))
        assert abs(float(got[0]) - vol) <= 1e-7


def test_sampler_exhaustive_sweep(rt4, oracle):
    """All 2^23 values rand() can return: no NaN, |w| <= 1, iterations as committed (and close to the
    survey's glibc-acosf sweep: a handful of inputs move between neighbouring bins)."""
    v = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(0x3F800000)).view(np.float32) - np.float32(1.0)
    w, it = oracle.eval_array(rt4.EVAL_W_BY_VOLUME, v)
    assert not np.isnan(w).any()
    assert np.abs(w).max() <= 1.0
    # Newton stops once a step is < SMALL_FLOAT, so w is only nearly monotone in v, but it inverts
    # volume_by_w closely: volume_by_w(w_by_volume(v)) = v within 2e-6 everywhere
    assert np.diff(w).min() > -1e-4
    vb, _ = oracle.eval_array(rt4.EVAL_VOLUME_BY_W, w)
    assert np.abs(vb - v).max() < 2e-6
    hist = np.bincount(it)
    golden = json.load(open(os.path.join(GOLDEN, "sampler.json")))
    assert hist.tolist() == golden["histogram"]
    survey = KAT["sampler_sweep_glibc"]
    assert it.max() == survey["max_iterations"]
    assert abs(it.mean() - survey["mean_iterations"]) < 1e-3
    assert np.abs(hist[1:] - np.array(survey["histogram_1_to_8"])).max() <= 100


def test_rand_drct_uniform_on_s3(oracle):
    import ctypes

    lib = oracle.lib()
    state = (ctypes.c_uint32 * 4)(12345, 12345, 0x3A000000, 0x3B000000)
    out = (ctypes.c_float * 4)()
    dirs = np.empty((100000, 4), np.float64)
    for i in range(dirs.shape[0]):
        lib.oracle_rand_drct(state, out)
        dirs[i] = out[:]
    norms = np.linalg.norm(dirs, axis=1)
    assert np.abs(norms - 1).max() < 2e-6
    second = (dirs ** 2).mean(axis=0)
    np.testing.assert_allclose(second, 0.25, atol=0.005)  # E[x_i^2] = 1/4 on S^3
    np.testing.assert_allclose(dirs.mean(axis=0), 0.0, atol=0.01)


def test_math_definitions_accuracy(rt4, oracle):
    """The oracle's acos/asin/sin/cos definitions are within a few ulp of the true functions."""
    x = np.linspace(-1, 1, 200001, dtype=np.float32)
    for fn, ref in ((rt4.EVAL_ACOS, np.arccos), (rt4.EVAL_ASIN, np.arcsin)):
        got, _ = oracle.eval_array(fn, x)
        exact = ref(x.astype(np.float64))
        ulp = np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)
        assert (np.abs(got - exact) / ulp).max() < 4
    a = np.linspace(-10, 10, 200001, dtype=np.float32)
    for fn, ref in ((rt4.EVAL_SIN, np.sin), (rt4.EVAL_COS, np.cos)):
        got, _ = oracle.eval_array(fn, a)
        assert np.abs(got - ref(a.astype(np.float64))).max() < 3e-7
    got, _ = oracle.eval_array(rt4.EVAL_ACOS, np.array([1.0000001, -1.0000001, np.nan], np.float32))
    assert np.isnan(got).all()  # angle() is unclamped (shader.frag:50): NaN outside [-1, 1]


# ------------------------------------------------------------------------------ intersectors
SCENE_HEAD = """const vec3 sky_light = vec3(0.2, 0.6, 1.2);
const sun_properties sun = sun_properties(vec4(0, 1, 1, 0), PI * 0.09, vec3(500, 500, 10), 0.0);
"""


def one_hit(rt4, oracle, body, find, origin, drct):
    scene = rt4.Scene.parse(SCENE_HEAD + body + "\nintersection find_intersection(ray ray) {\n"
                            "  intersection inter = NOT_INTERSECT;\n" + find + "\n  return inter;\n}\n")
    ray = np.array([list(origin) + list(drct)], np.float32)
    out, col = oracle.find_intersection(scene.desc, ray)
    return out[0], col[0]


def test_sphere_distance_and_normal(rt4, oracle):
    body = "const visible_sphere[1] spheres = visible_sphere[1](visible_sphere(sphere(vec4(0, 0, 0, 0), 1.0), material(0, 0.5, vec3(1, 0.5, 0.25))));"
    find = "for (int i = 0; i < spheres.length(); i++) inter = closest(sphere_intersection(spheres[i], ray, true), inter);"
    o, col = one_hit(rt4, oracle, body, find, (0, -5, 0, 0), (0, 1, 0, 0))
    assert o[0] == 1 and abs(o[1] - 4.0) < 2e-6
    np.testing.assert_allclose(o[2:6], [0, -1, 0, 0], atol=2e-6)  # outward, towards the ray origin
    assert o[7] == np.float32(0.5) and col.tolist() == [1.0, 0.5, 0.25]
    o, _ = one_hit(rt4, oracle, body, find, (0, -5, 0, 0), (0, -1, 0, 0))  # pointing away
    assert o[0] == 0
    o, _ = one_hit(rt4, oracle, body, find, (0, 0, 0, 0.5), (0, 1, 0, 0))  # from inside: far wall
    assert o[0] == 1 and abs(o[1] - math.sqrt(1 - 0.25)) < 2e-6


def test_space_distance_and_normal(rt4, oracle):
    body = "const visible_space[1] spaces = visible_space[1](visible_space(space(vec4(0, 0, -1.5, 0), vec4(0, 0, 1, 0)), material(0, 0, vec3(1))));"
    find = "for (int i = 0; i < spaces.length(); i++) inter = closest(space_intersection(spaces[i], ray), inter);"
    o, _ = one_hit(rt4, oracle, body, find, (0, 0, 0, 0), (0, 0, -1, 0))
    assert o[0] == 1 and abs(o[1] - 1.5) < 1e-6
    np.testing.assert_array_equal(o[2:6], np.array([0, 0, 1, 0], np.float32) * 1)  # faces the origin
    d = np.array([0, 0.6, -0.8, 0], np.float32)
    o, _ = one_hit(rt4, oracle, body, find, (0, 0, 0, 0), d)
    assert abs(o[1] - 1.5 / 0.8) < 2e-6
    o, _ = one_hit(rt4, oracle, body, find, (0, 0, 0, 0), (1, 0, 0, 0))  # parallel: cos < SMALL_FLOAT
    assert o[0] == 0


def test_hypercube_first_cell(rt4, oracle):
    body = """visible_hypercube hypercube = init_hypercube(vec4(0, 0, 0, 0), vec4(1, 0, 0, 0), vec4(0, 1, 0, 0),
  vec4(0, 0, 1, 0), vec4(0, 0, 0, 1), 1, material(0, 0, vec3(1, 0, 0)), material(0, 0, vec3(0, 1, 0)),
  material(0, 0, vec3(0, 0, 1)), material(0, 0, vec3(1, 1, 0)), material(0, 0, vec3(1, 0, 1)),
  material(0, 0, vec3(0, 1, 1)), material(0, 0, vec3(0.5)), material(0, 0, vec3(0.25)));"""
    find = "inter = closest(hypercube_intersection(hypercube, ray), inter);"
    o, col = one_hit(rt4, oracle, body, find, (-5, 0.2, 0.1, 0), (1, 0, 0, 0))
    assert o[0] == 1 and abs(o[1] - 4.0) < 1e-6
    np.testing.assert_array_equal(o[2:6], [-1, 0, 0, 0])
    assert col.tolist() == [1.0, 0.0, 1.0]  # the -x cell (material mxn)
    d = np.array([0.99, 0.1, 0, 0], np.float32)
    o, _ = one_hit(rt4, oracle, body, find, (-5, 3, 0, 0), d / np.linalg.norm(d))  # passes beside the cube
    assert o[0] == 0
    # reference quirk, kept: cube_intersection rejects only cos_dn < 0 (shader.frag:357-358), so a ray
    # exactly parallel to a cell, outside that cell's slab, divides by zero: dist = +inf, the extent
    # tests see NaN and pass, and the cell "hits" at infinity (the +y cell here)
    o, col = one_hit(rt4, oracle, body, find, (-5, 3, 0, 0), (1, 0, 0, 0))
    assert o[0] == 1 and np.isinf(o[1]) and col.tolist() == [0.0, 1.0, 0.0]


def test_cylinder_union_and_tiger(rt4, oracle):
    body = """visible_cylinders_union cylinders_union = visible_cylinders_union(
  visible_cylinder(vec4(0, 2, 0, 0), vec4(1, 0, 0, 0), vec4(0, 0, 0, 1), 1.0, material(0, 0, vec3(1, 0, 0))),
  visible_cylinder(vec4(0, 2, 0, 0), vec4(0, 0, 1, 0), vec4(0, 1, 0, 0), 1.0, material(0, 0, vec3(0, 1, 0))));"""
    find = "inter = closest(cylinders_union_intersection(cylinders_union, ray), inter);"
    o, col = one_hit(rt4, oracle, body, find, (0.5, -5, 0, 0), (0, 1, 0, 0))
    assert o[0] == 1 and abs(o[1] - 6.0) < 2e-6 and col.tolist() == [1, 0, 0]
    np.testing.assert_allclose(o[2:6], [0, -1, 0, 0], atol=2e-6)
    body = """visible_tiger tiger = init_tiger(vec4(0, 2, 0, 0), vec4(1, 0, 0, 0), vec4(0, 0, 0, 1),
  vec4(0, 0, 1, 0), vec4(0, 1, 0, 0), 0.9, 1.4, material(0, 0, vec3(1, 0, 0)), material(0, 0, vec3(0, 1, 0)));"""
    find = "inter = closest(tiger_intersection(tiger, ray), inter);"
    o, col = one_hit(rt4, oracle, body, find, (1.1, -5, 0, 0), (0, 1, 0, 0))
    assert o[0] == 1 and abs(o[1] - 5.6) < 2e-6 and col.tolist() == [1, 0, 0]  # outer cylinder of pair 1
    np.testing.assert_allclose(o[2:6], [0, -1, 0, 0], atol=2e-6)
    o, _ = one_hit(rt4, oracle, body, find, (0.0, -5, 0, 0), (0, 1, 0, 0))  # axis of pair 2: outside band
    assert o[0] == 0


# ------------------------------------------------------------------------------ image invariants
@pytest.mark.parametrize("name", ["sphere", "room", "tiger", "cylinder4d", "hypercube"])
def test_image_range(rt4, oracle, name):
    u = rt4.make_uniforms(40, 24, samples=2, reflections=3, seed=5)
    f, n, _, _ = oracle.render(rt4.Scene.builtin(name).desc, u, rt4.region(40, 24), threads=4)
    assert np.all(f[..., 3] == 1.0)
    assert np.all(f[..., :3] >= 0) and np.all(f[..., :3] < 1)
    assert 40 * 24 * 2 <= n <= 40 * 24 * 2 * 4


def test_sky_only_pixel_closed_form(rt4, oracle):
    """A primary ray that leaves the scene: colour = 1 - 1/(k*sky + 1) (sun away from the top row)."""
    scene = rt4.Scene.builtin("hypercube")
    u = rt4.make_uniforms(64, 40, samples=3, reflections=4, seed=7)
    f, _, _, _ = oracle.render(scene.desc, u, rt4.region(64, 1))  # top row looks up, away from objects
    sky = np.array(scene.desc.sky_light[:], np.float32)
    expect = np.float32(1) - np.float32(1) / (sky + np.float32(1))
    np.testing.assert_allclose(f[0, 0, :3], expect, rtol=1e-6)


def test_emissive_direct_hit(rt4, oracle):
    """reflections_amount = 0: a hit on the glowing sphere returns color*glow, no sky (shader.frag:494)."""
    scene = rt4.Scene.builtin("sphere")
    u = rt4.make_uniforms(96, 60, samples=2, reflections=0, seed=3)
    f, _, _, counts = oracle.render(scene.desc, u, rt4.region(96, 60), pixel_counts=True)
    assert counts.max() == 2  # one find_intersection per sample
    glow = np.float32(90)
    expect = np.float32(1) - np.float32(1) / (glow + np.float32(1))
    assert np.isclose(f[..., 0], expect, rtol=1e-6).any()  # the lamp sphere is in view


def test_op_count_per_unit(rt4, oracle):
    """Algorithmic fp32 ops per find_intersection+shading (the roofline numerator)."""
    u = rt4.make_uniforms(1920, 1080, samples=16, reflections=8, seed=12345)
    reg = rt4.region(1920, 4, y0=100, band_rows=1, band_step=250)
    _, n, ops, _ = oracle.render(rt4.Scene.builtin("sphere").desc, u, reg, count_ops=True)
    assert 200 < ops / n < 320
