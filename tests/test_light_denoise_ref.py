"""What the variance-guided filter of rt4.h (rt4_light_denoise_device) buys, measured on the CPU: its numpy restatement
(light_denoise_ref) on light accumulators folded from oracle frames, against one 4096-spp oracle frame, and the unit
properties of the definition. No GPU: the HIP kernels are held to this definition bit for bit in
test_gpu_light_denoise.py.

Every figure is MSE(filtered) / MSE(plain resolve) of the RGBA32F images over the filterable pixels, at 96 x 64,
4 bounces, k = 1, seeds 777, 991 and 31337; `4 x 16` is 16 frames of 4 spp.

Asserted without a number: (a) the filter beats the plain resolve on all six scenes at 4 x 16, 4 x 256 and 1 x 8;
(b) at 4 x 256 it beats the same filter with sigma = +inf (geometry only); (c) on all_primitives at 4 x 256 the
geometry-only filter is worse than not filtering while the default is better.

Asserted with a measured bound, the largest of the three seeds times 1.5 (measured range -> bound):
  scene        4 x 16                     4 x 256
  sphere       0.0450-0.0514 -> 0.0771    0.2313-0.2470 -> 0.3705
  tiger        0.1077-0.1212 -> 0.1818    0.2345-0.2501 -> 0.3752
  room         0.0303-0.0315 -> 0.0473    0.2122-0.2156 -> 0.3234
  hypercube    0.0510-0.0630 -> 0.0945    0.1957-0.2108 -> 0.3162
  cylinder4d   0.0838-0.1113 -> 0.1670    0.2283-0.2432 -> 0.3648
all_primitives (0.32-0.37 and 0.52-0.54) and the 1 x 8 split (0.10-0.47; the geometry-only filter 0.05-0.59) are
printed, not bounded."""
import functools

import numpy as np
import pytest

import denoise_ref
import light_denoise_ref as ldr
import light_ref

W, H, BOUNCES, K = 96, 64, 4, 1.0
SEEDS = (777, 991, 31337)
BOUNDED = ["sphere", "tiger", "room", "hypercube", "cylinder4d"]
SCENES = BOUNDED + ["all_primitives"]
SPLITS = ["4x16", "4x256", "1x8"]
# the largest of the three seeds' ratios times 1.5 (the module docstring has the measured ranges)
BOUNDS = {
    "sphere": {"4x16": 0.0771, "4x256": 0.3705},
    "tiger": {"4x16": 0.1818, "4x256": 0.3752},
    "room": {"4x16": 0.0473, "4x256": 0.3234},
    "hypercube": {"4x16": 0.0945, "4x256": 0.3162},
    "cylinder4d": {"4x16": 0.1670, "4x256": 0.3648},
}
_ctx = {}


def oracle_light(name, spp, frames, seed):
    """(light, colours), each (frames, H, W, 3) float32, of `frames` progressive oracle frames; the light is the tone
    map of each frame's colour inverted in float64, x = c / (k (1 - c))."""
    rt4, oracle = _ctx["rt4"], _ctx["oracle"]
    scene = rt4.Scene.named(name)
    base = rt4.make_uniforms(W, H, samples=spp, reflections=BOUNCES, seed=seed, k=K)
    reg = rt4.region(W, H)
    out, colours = np.empty((frames, H, W, 3), np.float32), np.empty((frames, H, W, 3), np.float32)
    for f in range(frames):
        u = rt4.progressive_uniforms(base, f + 1)
        u.part = 1.0
        colours[f] = oracle.render(scene.desc, u, reg)[0][..., :3]
        c = colours[f].astype(np.float64)
        assert (c < 1).all()
        out[f] = (c / (K * (1.0 - c))).astype(np.float32)
    return out, colours


def oracle_gbuffer(name):
    """The G-buffer of the view: numpy rays through the oracle's find_intersection, surfaces named by unique colours."""
    rt4, oracle = _ctx["rt4"], _ctx["oracle"]
    scene = rt4.Scene.named(name)
    marked = rt4.SceneDesc.from_buffer_copy(scene.to_bytes())
    table = denoise_ref.unique_colors(rt4, marked)
    g, hit, col = denoise_ref.gbuffer_reference(rt4, oracle, marked, rt4.make_uniforms(W, H, samples=1, reflections=BOUNCES),
                                                rt4.region(W, H))
    g["surface"] = denoise_ref.surfaces_from_colors(table, hit, col)
    return g


@functools.lru_cache(maxsize=None)
def measure(name):
    """{(split, seed): {"default": ratio, "geometry": sigma = +inf (4x256, 1x8), "geometry3": that at 3 levels (4x256),
    "colour_atrous": the colour average through denoise_ref.atrous (4x256)}}
    of one scene; computed once and printed."""
    rt4, oracle = _ctx["rt4"], _ctx["oracle"]
    ref = oracle.render(rt4.Scene.named(name).desc,
                        rt4.make_uniforms(W, H, samples=4096, reflections=BOUNCES, seed=4242, k=K, part=1.0),
                        rt4.region(W, H))[0][..., :3].astype(np.float64)
    g = oracle_gbuffer(name)
    filt = denoise_ref.filterable(g, ldr.DEFAULTS["max_refl_prob"])
    assert filt.sum() > W * H // 8, "too few filterable pixels for the ratio to mean anything"

    def mse(frame):
        return float(((frame[..., :3].astype(np.float64) - ref)[filt] ** 2).mean())

    out = {}
    for seed in SEEDS:
        accs = {}
        acc = np.zeros((H, W), light_ref.LIGHT_DTYPE)
        xs, colours = oracle_light(name, 4, 256, seed)
        for f, x in enumerate(xs):
            acc = light_ref.apply(acc, x)
            if f + 1 == 16:
                accs["4x16"] = acc
        accs["4x256"] = acc
        accs["1x8"] = light_ref.fold(np.zeros((H, W), light_ref.LIGHT_DTYPE), list(oracle_light(name, 1, 8, seed)[0]))
        # today's other path, printed only: the average of the tone-mapped colours through the colour filter (3 levels)
        average = np.ones((H, W, 4), np.float32)
        average[..., :3] = colours.astype(np.float64).mean(axis=0)
        for split, a in accs.items():
            plain = mse(light_ref.resolve(a, K))
            frame, _ = ldr.light_denoise(a, g, K)
            assert np.array_equal(frame[~filt].view(np.uint32), light_ref.resolve(a, K)[~filt].view(np.uint32))
            r = {"default": mse(frame) / plain}
            if split in ("4x256", "1x8"):
                r["geometry"] = mse(ldr.light_denoise(a, g, K, sigma=np.inf)[0]) / plain
            if split == "4x256":
                r["colour_atrous"] = mse(denoise_ref.atrous(average, g)) / plain
                r["geometry3"] = mse(ldr.light_denoise(a, g, K, sigma=np.inf, levels=3)[0]) / plain
            out[split, seed] = r
    for split in SPLITS:
        for kind in ("default", "geometry", "geometry3", "colour_atrous"):
            vals = [out[split, s][kind] for s in SEEDS if kind in out[split, s]]
            if vals:
                print(f"{name} {split} {kind}: " + " ".join(f"{v:.4f}" for v in vals) + f"  (range {min(vals):.4f}-{max(vals):.4f})")
    return out


@pytest.fixture
def measured(rt4, oracle):
    _ctx.update(rt4=rt4, oracle=oracle)
    return measure


@pytest.mark.slow
@pytest.mark.parametrize("name", SCENES)
def test_filter_beats_the_plain_resolve(measured, name):
    """(a): all six scenes, the three splits, the three seeds."""
    m = measured(name)
    for split in SPLITS:
        for seed in SEEDS:
            assert m[split, seed]["default"] < 1.0, (name, split, seed, m[split, seed])


@pytest.mark.slow
@pytest.mark.parametrize("name", SCENES)
def test_variance_beats_geometry_only_once_converged(measured, name):
    """(b): at 4 x 256 the default is below sigma = +inf at the same five levels."""
    m = measured(name)
    for seed in SEEDS:
        assert m["4x256", seed]["default"] < m["4x256", seed]["geometry"], (name, seed, m["4x256", seed])


@pytest.mark.slow
def test_geometry_only_hurts_all_primitives(measured):
    """(c): the reason the variance is used at all."""
    m = measured("all_primitives")
    for seed in SEEDS:
        r = m["4x256", seed]
        assert r["geometry"] > 1.0 > r["default"], (seed, r)


@pytest.mark.slow
@pytest.mark.parametrize("split", ["4x16", "4x256"])
@pytest.mark.parametrize("name", BOUNDED)
def test_ratio_within_its_measured_bound(measured, name, split):
    m = measured(name)
    for seed in SEEDS:
        assert m[split, seed]["default"] <= BOUNDS[name][split], (name, split, seed, m[split, seed])


# ------------------------------------------------------------------------------------------ unit properties
GB = np.dtype([("normal", "<f4", (4,)), ("depth", "<f4"), ("surface", "<i4"), ("refl_prob", "<f4"), ("glow", "<f4")])


def flat_gbuffer(h, w, surface=0):
    g = np.zeros((h, w), GB)
    g["normal"] = (0, 0, 1, 0)
    g["depth"] = 3.0
    g["surface"] = surface
    return g


def random_acc(seed, h=9, w=13, n=8):
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    a["mean"] = (rng.random((h, w, 3)) * 2).astype(np.float32)
    a["mean_y"] = light_ref.luminance(a["mean"])
    a["m2"] = (rng.random((h, w)) * 3).astype(np.float32)
    a["n"] = n
    return a


def raw(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8])
def test_no_levels_and_all_misses_are_the_plain_resolve(dtype):
    a = random_acc(1)
    a["n"][0, :4] = [0, 1, 2, 3]
    want = light_ref.resolve(a, 0.7, dtype)
    frame, fl = ldr.light_denoise(a, flat_gbuffer(9, 13), 0.7, dtype, levels=0)
    assert frame.dtype == want.dtype and raw(frame) == raw(want)
    assert raw(fl[..., :3]) == raw(a["mean"]) and np.isposinf(fl[0, :2, 3]).all() and np.isfinite(fl[0, 2:, 3]).all()
    assert raw(fl[0, 2:, 3]) == raw(ldr.variance0(a)[0, 2:])
    frame, fl0 = ldr.light_denoise(a, flat_gbuffer(9, 13, surface=-1), 0.7, dtype)
    assert raw(frame) == raw(want) and raw(fl0) == raw(fl)
    # reflective above the threshold: the same
    g = flat_gbuffer(9, 13)
    g["refl_prob"] = np.float32(0.50000006)
    assert raw(ldr.light_denoise(a, g, 0.7, dtype)[0]) == raw(want)


def test_constant_accumulator_comes_back_unchanged():
    a = np.zeros((9, 13), light_ref.LIGHT_DTYPE)
    a["mean"] = (0.25, 0.5, 0.75)  # dyadic: every weighted sum is exact enough to divide back
    a["mean_y"] = 0.5
    a["n"] = 4
    frame, fl = ldr.light_denoise(a, flat_gbuffer(9, 13), 1.0)
    assert raw(frame) == raw(light_ref.resolve(a, 1.0))
    assert raw(fl[..., :3]) == raw(a["mean"]) and not fl[..., 3].any()


def test_variance_after_one_level_on_a_flat_surface():
    """Equal variances, equal luminances: every tap has wl = 1, so V' = V * sum(k^2) / sum(k)^2 over the taps inside."""
    h, w = 9, 13
    a = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    a["mean"] = 0.5
    a["mean_y"] = 0.5
    a["n"] = 2
    a["m2"] = 4.0  # V_0 = 4 / 1 / 2 = 2
    _, fl = ldr.light_denoise(a, flat_gbuffer(h, w), 1.0, levels=1)
    k = np.outer(denoise_ref.H5, denoise_ref.H5).astype(np.float64)
    inner = 2.0 * (k ** 2).sum() / k.sum() ** 2
    assert np.allclose(fl[2:-2, 2:-2, 3], inner, rtol=1e-6) and inner < 0.15 * 2.0
    kc = k[2:, 2:]  # the corner pixel: the taps with dy, dx >= 0
    assert np.isclose(fl[0, 0, 3], 2.0 * (kc ** 2).sum() / kc.sum() ** 2, rtol=1e-6)


def test_pixels_with_fewer_than_two_frames_are_neither_filtered_nor_tapped():
    a = random_acc(3)
    young = np.zeros(a.shape, bool)
    young[::2, 1::3] = True
    a["n"][young] = 1
    a["mean"][young] = 1e6  # would show in every neighbour
    a["mean_y"][young] = 1e6
    g = flat_gbuffer(*a.shape)
    _, fl = ldr.light_denoise(a, g, 1.0, sigma=np.inf)
    assert raw(fl[young][:, :3]) == raw(a["mean"][young]) and np.isposinf(fl[young][:, 3]).all()
    assert (fl[~young][:, :3] < 3).all()
    # the same result with those pixels turned into misses
    g2 = g.copy()
    g2["surface"][young] = -1
    assert raw(ldr.light_denoise(a, g2, 1.0, sigma=np.inf)[1][~young]) == raw(fl[~young])


def test_an_isolated_bright_pixel_is_reduced_and_its_neighbours_move_less():
    h, w = 9, 13
    a = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    a["mean"] = 0.5
    a["mean_y"] = 0.5
    a["n"] = 16
    a["mean"][4, 6] = 50.0
    a["mean_y"][4, 6] = 50.0
    a["m2"][4, 6] = 16 * 15 * 49.5 ** 2  # one bright frame among 16: se about the excess
    _, fl = ldr.light_denoise(a, flat_gbuffer(h, w), 1.0)
    moved = np.abs(fl[..., 0] - a["mean"][..., 0])
    assert fl[4, 6, 0] < 50.0
    others = np.ones((h, w), bool)
    others[4, 6] = False
    assert moved[others].max() < moved[4, 6]
