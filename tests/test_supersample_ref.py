"""The supersampled light accumulator's definition (include/rt4.h rt4_light_downsample_device, restated in
supersample_ref) on the CPU, no GPU: the unit properties of the definition, then against the CPU oracle that the
anti-aliased image is closer to the truth at equal rays where outlines matter, and that its standard error is
calibrated against two independent runs while a merge of the strata as frames is not."""
import numpy as np
import pytest

import light_merge_ref
import light_ref
import supersample_ref

W, H, BOUNCES, K = 48, 30, 4, 1.0
F32 = np.float32


# ------------------------------------------------------------------------------------------ unit properties
def random_fine(seed, h, w, s, n_choices=(2, 3, 7, 40)):
    rng = np.random.default_rng(seed)
    a = np.zeros((h * s, w * s), light_ref.LIGHT_DTYPE)
    a["mean"] = (rng.random((h * s, w * s, 3)) * 3).astype(F32)
    a["mean_y"] = light_ref.luminance(a["mean"])
    a["m2"] = (rng.random((h * s, w * s)) * 5).astype(F32)
    a["n"] = rng.choice(np.array(n_choices, np.int32), (h * s, w * s))
    return a


@pytest.mark.parametrize("s", [1, 2, 3, 8])
def test_an_empty_stratum_empties_the_pixel(s):
    fine = random_fine(1, 3, 4, s)
    fine["n"][1 * s + s - 1, 2 * s + s - 1] = 0  # the last stratum of pixel (2, 1)
    fine["n"][0, 0] = -5  # a negative count is no sample either: pixel (0, 0)
    out = supersample_ref.downsample(fine, s)
    empty = np.zeros((), light_ref.LIGHT_DTYPE).tobytes()
    assert out[1, 2].tobytes() == empty and out[0, 0].tobytes() == empty
    assert (out["n"] > 0).sum() == 3 * 4 - 2


@pytest.mark.parametrize("s", [1, 2, 4])
def test_one_frame_in_a_stratum_is_unmeasured(s):
    """n = 1 in one stratum: n' = 1 and m2' = 0, the means still averaged."""
    fine = random_fine(2, 2, 2, s)
    fine["n"][0, 0] = 1
    out = supersample_ref.downsample(fine, s)
    assert out["n"][0, 0] == 1 and out["m2"][0, 0] == 0 and out["mean_y"][0, 0] > 0
    assert (out["n"][0, 1:] >= 2).all() and (out["m2"][0, 1:] > 0).all()
    se, _, _, stats = light_ref.noise(out, K, 1.0 / 255.0)
    assert np.isinf(se[0, 0]) and stats["measured"] == 3


@pytest.mark.parametrize("s", [1, 2, 3])
def test_constant_input_has_no_noise(s):
    x = np.full((2 * s, 3 * s, 3), 0.25, F32)
    fine = light_ref.fold(np.zeros((2 * s, 3 * s), light_ref.LIGHT_DTYPE), [x] * 5)
    out = supersample_ref.downsample(fine, s)
    se, _, _, _ = light_ref.noise(out, K, 1.0 / 255.0)
    assert (out["n"] == 5).all() and (out["m2"] == 0).all() and (se == 0).all()
    assert np.allclose(out["mean"], 0.25, rtol=1e-6, atol=0) and np.allclose(out["mean_y"], fine["mean_y"][0, 0], rtol=1e-6, atol=0)


def test_s1_keeps_mean_and_n_bit_for_bit():
    fine = random_fine(3, 5, 7, 1, n_choices=(1, 2, 3, 1000, 2 ** 31 - 1))
    out = supersample_ref.downsample(fine, 1)
    assert np.array_equal(out["n"], fine["n"])
    assert light_ref.same_floats(out["mean"], fine["mean"]) and light_ref.same_floats(out["mean_y"], fine["mean_y"])
    measured = fine["n"] >= 2
    assert (out["m2"][~measured] == 0).all()
    # m2 comes back through four roundings: (m2 / (n-1)) / n, then * n * (n-1)
    rel = np.abs(out["m2"][measured].astype(np.float64) / fine["m2"][measured].astype(np.float64) - 1.0)
    assert rel.max() < 4 * 2.0 ** -23, rel.max()


@pytest.mark.parametrize("s", [1, 2, 3, 4, 8])
def test_downstream_standard_error_is_the_root_of_the_variance(s):
    """The noise map's se of the output is sqrt(sum se_i^2 / s^4) of the strata, float64, to within 1e-6 relative."""
    fine = random_fine(10 + s, 6, 5, s, n_choices=(2, 3, 7, 40, 100000))
    out = supersample_ref.downsample(fine, s)
    se, _, _, _ = light_ref.noise(out, K, 1.0 / 255.0)
    want = np.sqrt(supersample_ref.variance(fine, s))
    rel = np.abs(se.astype(np.float64) / want - 1.0)
    print(f"s {s}: downstream se against sqrt(var), largest relative error {rel.max():.3g}")
    assert rel.max() < 1e-6, (s, rel.max())


# ------------------------------------------------------------------------------------------ against the oracle
def light_from_colour(c):
    """x = c / (k (1 - c)) in float64: the tone map inverted (as test_light_ref)."""
    assert (c < 1).all(), c.max()
    c = c.astype(np.float64)
    return c / (K * (1.0 - c))


def oracle_light(rt4, oracle, name, s, spp, frames, seed):
    """The light (frames, H*s, W*s, 3) float64 of `frames` progressive frames of the view at s times the resolution,
    rt4.upscale_uniforms of the W x H view."""
    scene = rt4.Scene.named(name)
    base = rt4.upscale_uniforms(rt4.make_uniforms(W, H, samples=spp, reflections=BOUNCES, seed=seed, k=K), s)
    reg = rt4.region(W * s, H * s)
    out = np.empty((frames, H * s, W * s, 3), np.float64)
    for f in range(frames):
        u = rt4.progressive_uniforms(base, f + 1)
        u.part = 1.0
        out[f] = light_from_colour(oracle.render(scene.desc, u, reg)[0][..., :3])
    return out


def accumulate(xs):
    return light_ref.fold(np.zeros(xs.shape[1:3], light_ref.LIGHT_DTYPE), list(xs.astype(F32)))


def supersampled(rt4, oracle, name, s, spp, frames, seed):
    """(fine accumulator, its downsample): the pipeline of rt4_render --light --supersample s, in the references."""
    fine = accumulate(oracle_light(rt4, oracle, name, s, spp, frames, seed))
    return fine, supersample_ref.downsample(fine, s)


_truth = {}


def truth(rt4, oracle, name):
    """S = 4, 256 samples per sub-pixel, seed 4242, box-averaged as light, then tone-mapped: (H, W, 3) float64."""
    if name not in _truth:
        x = oracle_light(rt4, oracle, name, 4, 256, 1, 4242)[0]
        x = x.reshape(H, 4, W, 4, 3).mean(axis=(1, 3))
        _truth[name] = 1.0 - 1.0 / (K * x + 1.0)
    return _truth[name]


def rmse_pair(rt4, oracle, name):
    """RMSE in display units against the truth at 256 samples per pixel, seed 777: S = 1, 4 spp x 64 frames and
    S = 2, 4 spp x 16 frames. The same number of rays."""
    ref = truth(rt4, oracle, name)
    out = []
    for s, frames in ((1, 64), (2, 16)):
        _, acc = supersampled(rt4, oracle, name, s, 4, frames, 777)
        image = light_ref.resolve(acc, K)[..., :3].astype(np.float64)
        out.append(float(np.sqrt(((image - ref) ** 2).mean())))
    return out


def test_supersampling_beats_more_frames_on_an_outline(rt4, oracle):
    """Sphere: at equal rays the anti-aliased image is closer to the truth (float64 prototype: 0.0684 against 0.1038)."""
    plain, anti = rmse_pair(rt4, oracle, "sphere")
    print(f"sphere: RMSE S=1 4 spp x 64 {plain:.4f}, S=2 4 spp x 16 {anti:.4f}")
    assert anti < plain, (plain, anti)


@pytest.mark.parametrize("name", ["tiger", "hypercube", "cylinder4d", "room"])
def test_supersampling_elsewhere_is_within_the_noise(rt4, oracle, name):
    """Printed, not asserted: on these scenes noise dominates and the two differ by a few percent either way."""
    plain, anti = rmse_pair(rt4, oracle, name)
    print(f"{name}: RMSE S=1 4 spp x 64 {plain:.4f}, S=2 4 spp x 16 {anti:.4f}")
    assert np.isfinite(plain) and np.isfinite(anti)


def calibration(runs):
    """sum (y_a - y_b)^2 / sum (se_a^2 + se_b^2) over the pixels of two independent runs: expected value 1."""
    (ya, sa), (yb, sb) = runs
    return float(((ya - yb) ** 2).sum() / (sa ** 2 + sb ** 2).sum())


def mean_and_se(acc):
    se, _, _, stats = light_ref.noise(acc, K, 1.0 / 255.0)
    assert stats["measured"] == acc.size
    return acc["mean_y"].astype(np.float64), se.astype(np.float64)


@pytest.mark.parametrize("s, spp, frames", [(2, 4, 32), (3, 2, 16)])
@pytest.mark.parametrize("name", ["sphere", "tiger", "room", "hypercube"])
def test_standard_error_is_calibrated(rt4, oracle, name, s, spp, frames):
    """[0.5, 2] is the margin test_light_ref uses for this heavy-tailed statistic (0.79 .. 1.09 in the float64 prototype).
    On sphere at S = 2 the same statistic with the strata folded as frames of one variable (light_merge_ref) is below
    0.5: the error estimate would be many times too large, which is why the downsample is a kernel of its own."""
    strat, merged = [], []
    for seed in (777, 991):
        fine, acc = supersampled(rt4, oracle, name, s, spp, frames, seed)
        strat.append(mean_and_se(acc))
        if name == "sphere" and s == 2:
            parts = [np.ascontiguousarray(p) for p in supersample_ref.strata(fine, s)]
            merged.append(mean_and_se(light_merge_ref.merge_all(np.zeros((H, W), light_ref.LIGHT_DTYPE), parts)))
    ratio = calibration(strat)
    print(f"{name} S={s} {spp} spp x {frames}: calibration ratio {ratio:.3f}")
    assert 0.5 <= ratio <= 2.0, (name, s, ratio)
    if merged:
        as_frames = calibration(merged)
        print(f"{name} S={s} {spp} spp x {frames}: strata merged as frames, calibration ratio {as_frames:.3f}")
        assert as_frames < 0.5, as_frames
