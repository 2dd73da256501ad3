"""The light accumulator's definition (include/rt4.h rt4_light_px, restated in light_ref) against the CPU oracle, no
GPU: the light average is less biased than the colour average and does not depend on how the samples are split into
frames, its standard error is calibrated against two independent runs, and the unit properties of the definition."""
import numpy as np
import pytest

import light_ref

W, H, BOUNCES, K = 48, 30, 4, 1.0
SPLITS = [(1, 64), (4, 16), (16, 4)]  # samples per frame x frames: 64 samples per pixel each


def oracle_frames(rt4, oracle, name, spp, frames, seed):
    """The tone-mapped colours (frames, H, W, 3) float32 of `frames` progressive frames (part = 1 each)."""
    scene = rt4.Scene.named(name)
    base = rt4.make_uniforms(W, H, samples=spp, reflections=BOUNCES, seed=seed, k=K)
    reg = rt4.region(W, H)
    out = np.empty((frames, H, W, 3), np.float32)
    for f in range(frames):
        u = rt4.progressive_uniforms(base, f + 1)
        u.part = 1.0
        out[f] = oracle.render(scene.desc, u, reg)[0][..., :3]
    return out


def light_from_colour(c):
    """x = c / (k (1 - c)) in float64: the tone map inverted."""
    assert (c < 1).all(), c.max()  # the largest colour seen was 0.99945
    c = c.astype(np.float64)
    return c / (K * (1.0 - c))


def accumulate(colours):
    """light_ref.fold of the frames' light into an empty accumulator."""
    xs = light_from_colour(colours).astype(np.float32)
    return light_ref.fold(np.zeros((H, W), light_ref.LIGHT_DTYPE), list(xs))


@pytest.mark.parametrize("name", ["sphere", "room", "tiger"])
def test_light_average_is_less_biased_and_split_independent(rt4, oracle, name):
    ref = oracle_frames(rt4, oracle, name, 4096, 1, 4242)[0].astype(np.float64)
    bias_colour, bias_light = [], []
    for spp, frames in SPLITS:
        c = oracle_frames(rt4, oracle, name, spp, frames, 777)
        bias_colour.append(float((c.astype(np.float64).mean(axis=0) - ref).mean()))
        image = light_ref.resolve(accumulate(c), K)[..., :3].astype(np.float64)
        bias_light.append(float((image - ref).mean()))
    print(f"{name}: bias colour {bias_colour}, bias light {bias_light}")
    for bc, bl in zip(bias_colour, bias_light):
        assert abs(bl) < abs(bc), (name, bias_colour, bias_light)
    assert max(bias_light) - min(bias_light) < max(bias_colour) - min(bias_colour), (name, bias_colour, bias_light)


@pytest.mark.parametrize("spp", [4, 1])
@pytest.mark.parametrize("name", ["sphere", "tiger", "room", "hypercube"])
def test_standard_error_is_calibrated(rt4, oracle, name, spp):
    """Two independent runs of 32 frames: sum (mean_a - mean_b)^2 / sum (se_a^2 + se_b^2) over the pixels has the
    expected value 1; [0.5, 2] is the margin for a heavy-tailed statistic at 1440 pixels (0.87 .. 1.21 measured)."""
    runs = []
    for seed in (777, 991):
        acc = accumulate(oracle_frames(rt4, oracle, name, spp, 32, seed))
        se, _, _, stats = light_ref.noise(acc, K, 1.0 / 255.0)
        assert stats["measured"] == W * H
        runs.append((acc["mean_y"].astype(np.float64), se.astype(np.float64)))
    (ya, sa), (yb, sb) = runs
    ratio = ((ya - yb) ** 2).sum() / (sa ** 2 + sb ** 2).sum()
    print(f"{name} {spp} spp x 32: calibration ratio {ratio:.3f}")
    assert 0.5 <= ratio <= 2.0, (name, spp, ratio)


# ------------------------------------------------------------------------------------------ unit properties
def random_light(seed, h=5, w=7):
    rng = np.random.default_rng(seed)
    return (rng.random((h, w, 3)) * rng.choice([0.0, 0.1, 1.0, 50.0], (h, w, 1))).astype(np.float32)


def test_one_frame_is_the_frame():
    x = random_light(1)
    acc = light_ref.apply(np.zeros(x.shape[:2], light_ref.LIGHT_DTYPE), x)
    assert acc["mean"].tobytes() == x.tobytes()
    assert acc["mean_y"].tobytes() == light_ref.luminance(x).tobytes()
    assert (acc["n"] == 1).all() and not acc["m2"].any() and not acc["reserved"].any()
    # and its resolve is the tone map of the frame
    want = np.float32(1) - np.float32(1) / light_ref.fma32(np.float32(K), x, np.float32(1))
    assert light_ref.resolve(acc, K)[..., :3].tobytes() == want.astype(np.float32).tobytes()


def test_n_saturates():
    acc = np.zeros((1, 2), light_ref.LIGHT_DTYPE)
    acc["n"] = [[light_ref.INT32_MAX - 1, light_ref.INT32_MAX]]
    out = light_ref.apply(acc, np.ones((1, 2, 3), np.float32))
    assert out["n"].tolist() == [[light_ref.INT32_MAX, light_ref.INT32_MAX]]
    assert (out["mean"] == np.float32(1.0) / np.float32(2.0 ** 31)).all()  # inv = 1 / (float)INT32_MAX for both


def test_constant_input_has_no_noise():
    x = random_light(2)
    acc = light_ref.fold(np.zeros(x.shape[:2], light_ref.LIGHT_DTYPE), [x] * 5)
    assert (acc["n"] == 5).all() and not acc["m2"].any()
    assert acc["mean"].tobytes() == x.tobytes()
    se, q, tiles, stats = light_ref.noise(acc, K, 0.0)
    assert not se.any() and not q.any() and not tiles.any()
    assert stats == {"pixels": 35, "measured": 35, "above": 0, "max_q": 0.0, "max_se": 0.0}


def test_fewer_than_two_frames_is_unmeasured():
    acc = np.zeros((3, 9), light_ref.LIGHT_DTYPE)
    acc["n"][:, 3:] = 1
    acc["m2"] = 4.0
    acc["n"][2, 8] = 2
    se, q, tiles, stats = light_ref.noise(acc, K, 0.5)
    assert np.isposinf(se).sum() == 26 and np.isposinf(q).sum() == 26
    assert se[2, 8] == np.float32(np.sqrt(2.0)) and stats["measured"] == 1 and stats["above"] == 1
    assert tiles.tolist() == [[0, 1]] and stats["max_se"] == float(se[2, 8]) and stats["max_q"] == float(q[2, 8])
    assert (light_ref.resolve(acc, K)[:, :3, :3] == 0).all() and (light_ref.resolve(acc, K)[..., 3] == 1).all()


def test_nan_is_counted_nowhere():
    xs = [random_light(s, 2, 3) for s in (3, 4, 5)]
    xs[1][0, 1, 1] = np.nan
    acc = light_ref.fold(np.zeros((2, 3), light_ref.LIGHT_DTYPE), xs)
    assert np.isnan(acc["mean_y"][0, 1]) and np.isnan(acc["m2"][0, 1]) and np.isnan(acc["mean"][0, 1, 1])
    assert not np.isnan(acc["mean"][0, 1, 0])  # the other channels go on
    se, q, tiles, stats = light_ref.noise(acc, K, -1.0)  # every number is above -1; NaN is not
    assert np.isnan(q[0, 1]) and np.isnan(se[0, 1])
    assert stats["measured"] == 6 and stats["above"] == 5 and tiles.tolist() == [[5]]
    clean = np.ones((2, 3), bool)
    clean[0, 1] = False
    assert stats["max_q"] == float(q[clean].max()) and stats["max_se"] == float(se[clean].max())
