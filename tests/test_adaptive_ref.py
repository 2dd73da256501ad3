"""Adaptive light sampling (include/rt4.h rt4_light_select_tiles_device and the loop of DESIGN.md §4.39, restated in
adaptive_ref) on the CPU, no GPU: the unit properties of the selection's definition, and the study behind the defaults:
the loop against the same budget of uniform frames on the CPU oracle."""
import numpy as np
import pytest

import adaptive_ref
import light_ref
from adaptive_ref import Params

K = 1.0


# ------------------------------------------------------------------------------------------ unit properties
def quiet(h, w, n=16):
    """An accumulator whose pixels are all measured and noiseless."""
    acc = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    acc["n"] = n
    acc["mean_y"] = 0.5
    acc["mean"] = 0.5
    return acc


def make_hot(acc, ys, xs):
    acc["m2"][ys, xs] = 100.0


def test_strict_greater_at_the_threshold():
    acc = quiet(8, 16)
    make_hot(acc, 0, 0)
    make_hot(acc, 0, 8)
    acc["m2"][0, 8] = 1.0
    q = light_ref.noise(acc, K, 0.0)[1]
    assert q[0, 0] > q[0, 8] > 0
    p = Params(threshold=float(q[0, 8]), min_above=1, min_frames=0, dilate=0)
    assert adaptive_ref.select_tiles(acc, K, p)[0].tolist() == [0]  # q == threshold is not above it
    p.threshold = float(np.nextafter(q[0, 8], np.float32(0)))
    assert adaptive_ref.select_tiles(acc, K, p)[0].tolist() == [0, 1]


@pytest.mark.parametrize("min_above", [1, 3, 64])
def test_min_above_reached_exactly_and_missed_by_one(min_above):
    acc = quiet(8, 16)
    idx = np.arange(64)
    make_hot(acc, idx[:min_above] // 8, idx[:min_above] % 8)  # tile 0: exactly min_above hot pixels
    make_hot(acc, idx[:min_above - 1] // 8, 8 + idx[:min_above - 1] % 8)  # tile 1: one fewer
    tiles, state = adaptive_ref.select_tiles(acc, K, Params(threshold=0.01, min_above=min_above, min_frames=0, dilate=0))
    assert tiles.tolist() == [0] and state.tolist() == [[2, 0]]


def test_a_young_pixel_in_a_quiet_tile():
    acc = quiet(8, 24)
    acc["n"][7, 23] = 4
    for min_frames, want in ((0, []), (4, []), (5, [2]), (16, [2]), (17, [0, 1, 2])):
        assert adaptive_ref.select_tiles(acc, K, Params(0.01, 1, min_frames, 0))[0].tolist() == want, min_frames
    acc["n"][0, 0] = 1  # unmeasured: not hot whatever its m2, young below min_frames 2
    acc["m2"][0, 0] = 1e30
    assert adaptive_ref.select_tiles(acc, K, Params(0.0, 1, 1, 0))[0].tolist() == []
    assert adaptive_ref.select_tiles(acc, K, Params(0.0, 1, 2, 0))[0].tolist() == [0]


def test_pixels_outside_a_partial_edge_tile_never_count():
    wide = quiet(9, 12)
    make_hot(wide, slice(None), slice(9, 12))  # columns 9.. are padding for a 9 x 9 image
    wide["n"][:, 9:] = 0
    img = np.ascontiguousarray(wide[:, :9])
    tiles, state = adaptive_ref.select_tiles(img, K, Params(0.01, 1, 8, 0))
    assert tiles.tolist() == [] and state.shape == (2, 2)
    make_hot(img, 8, 8)  # the one pixel of the corner tile
    assert adaptive_ref.select_tiles(img, K, Params(0.01, 1, 8, 0))[0].tolist() == [3]
    assert adaptive_ref.select_tiles(img, K, Params(0.01, 2, 8, 0))[0].tolist() == []


def test_no_dilation_wrap_around_and_ascending_output():
    acc = quiet(24, 32)  # 4 x 3 tiles
    make_hot(acc, 0, 31)  # tile 3: the end of tile row 0
    tiles, state = adaptive_ref.select_tiles(acc, K, Params(0.01, 1, 0, 1))
    assert tiles.tolist() == [2, 3, 6, 7]  # not tile 4, the start of the next row
    assert state.tolist() == [[0, 0, 1, 2], [0, 0, 1, 1], [0, 0, 0, 0]]
    make_hot(acc, 23, 0)  # tile 8: a corner
    tiles, state = adaptive_ref.select_tiles(acc, K, Params(0.01, 1, 0, 2))
    assert tiles.tolist() == sorted(tiles.tolist()) == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11]
    tiles, _ = adaptive_ref.select_tiles(acc, K, Params(0.01, 1, 0, 1))
    assert tiles.tolist() == [2, 3, 4, 5, 6, 7, 8, 9]
    assert adaptive_ref.tile_mask([3, 8, 12, 0xFFFFFFFF], 32, 24).sum() == 128


def test_the_loop_spends_its_budget_and_numbers_frames_globally():
    """A scene whose left tile is noisy and whose right tile is constant: the loop's log, budget and frame numbers."""
    w, h = 16, 8
    seen = []

    def frame(g):
        seen.append(g)
        x = np.full((h, w, 3), 0.25, np.float32)
        x[:, :8] = np.float32(g % 3)
        return x

    acc, log, frames = adaptive_ref.adaptive(frame, w, h, K, 16, Params(0.01, 1, 0, 0), warmup=4, pass_frames=4, full_every=3)
    assert seen == list(range(1, frames + 1))
    assert log[0] == ("warmup", 2, 4) and log[1] == ("tiles", 1, 4) and log[3] == ("full", 2, 4)
    assert sum(t * f for _, t, f in log) == 16 * 2
    assert (acc["n"][:, 8:] == acc["n"][0, 8]).all() and acc["n"][0, 0] > acc["n"][0, 8] >= 4
    # nothing noisy: every pass is a whole-frame pass and the loop does not stop early
    acc, log, frames = adaptive_ref.adaptive(lambda g: np.ones((h, w, 3), np.float32), w, h, K, 9, Params(0.01, 1, 0, 0),
                                             warmup=2, pass_frames=4, full_every=0)
    assert log == [("warmup", 2, 2), ("empty", 2, 4), ("empty", 2, 3)] and frames == 9 and (acc["n"] == 9).all()


# ------------------------------------------------------------------------------------------ the study
W, H, SPP, BOUNCES, BUDGET = 96, 60, 4, 4, 64
SEEDS = [101, 202, 303, 404, 505, 606, 707, 808]
SCENES = ["sphere", "room", "tiger", "hypercube"]


def oracle_colour(rt4, oracle, name, spp, seed, g):
    """The tone-mapped colour (H, W, 3) float32 of progressive frame g (part = 1), as tests/test_light_ref.py."""
    base = rt4.make_uniforms(W, H, samples=spp, reflections=BOUNCES, seed=seed, k=K)
    u = rt4.progressive_uniforms(base, g)
    u.part = 1.0
    return oracle.render(rt4.Scene.named(name).desc, u, rt4.region(W, H))[0][..., :3]


def light_from_colour(c):
    """x = c / (k (1 - c)) in float64: the tone map inverted."""
    assert (c < 1).all(), c.max()
    c = c.astype(np.float64)
    return (c / (K * (1.0 - c))).astype(np.float32)


def errors(acc, ref):
    """(RMSE, mean absolute error, mean signed error) of the resolved image against ref, in display units."""
    d = light_ref.resolve(acc, K)[..., :3].astype(np.float64) - ref
    return np.sqrt((d ** 2).mean()), np.abs(d).mean(), d.mean()


def study(rt4, oracle, name, params=None, seeds=SEEDS, **loop):
    """{"uniform" | "adaptive": (len(seeds), 3) errors, "logs": [...], "n": [the adaptive runs' n images]}."""
    ref = oracle_colour(rt4, oracle, name, 4096, 4242, 1).astype(np.float64)
    out = {"uniform": [], "adaptive": [], "logs": [], "n": []}
    for seed in seeds:
        cache = {}

        def frame(g):
            if g not in cache:
                cache[g] = light_from_colour(oracle_colour(rt4, oracle, name, SPP, seed, g))
            return cache[g]

        uni = light_ref.fold(np.zeros((H, W), light_ref.LIGHT_DTYPE), [frame(g) for g in range(1, BUDGET + 1)])
        acc, log, _ = adaptive_ref.adaptive(frame, W, H, K, BUDGET, params, **loop)
        out["uniform"].append(errors(uni, ref))
        out["adaptive"].append(errors(acc, ref))
        out["logs"].append(log)
        out["n"].append(acc["n"].copy())
    out["uniform"], out["adaptive"] = np.array(out["uniform"]), np.array(out["adaptive"])
    return out


def mean_se(x):
    return float(np.mean(x)), float(np.std(x, ddof=1) / np.sqrt(len(x)))


@pytest.mark.parametrize("name", SCENES)
def test_adaptive_against_uniform_at_the_same_budget(rt4, oracle, name):
    """The defaults (adaptive_ref.Params(), WARMUP, PASS_FRAMES, FULL_EVERY) at a budget of 64 frames against 64 uniform
    frames, 8 base seeds, reference one 4096-spp frame. Prints the table of DESIGN.md §4.39. Asserts that the budget is
    spent to within one pass, that every pixel got the warm-up, and adaptive RMSE < uniform RMSE where the two means
    differ by more than twice the standard error of their (paired) difference; where they do not, nothing."""
    r = study(rt4, oracle, name)
    tiles = ((W + 7) // 8) * ((H + 7) // 8)
    for log, n in zip(r["logs"], r["n"]):
        spent = sum(t * f for _, t, f in log)
        assert BUDGET * tiles - tiles < spent <= BUDGET * tiles, (name, spent)  # less than one frame of the last pass left
        assert n.min() >= adaptive_ref.WARMUP
    for col, what in enumerate(("RMSE", "MAE", "bias")):
        (mu, su), (ma, sa) = mean_se(r["uniform"][:, col]), mean_se(r["adaptive"][:, col])
        md, sd = mean_se(r["adaptive"][:, col] - r["uniform"][:, col])
        print(f"{name} {what}: uniform {mu:.6f} +- {su:.6f}, adaptive {ma:.6f} +- {sa:.6f}, difference {md:+.6f} +- {sd:.6f}")
    ns = np.array(r["n"])
    print(f"{name} n: min {ns.min()}, median {int(np.median(ns))}, max {ns.max()}; passes {[len(g) for g in r['logs']]}")
    md, sd = mean_se(r["adaptive"][:, 0] - r["uniform"][:, 0])
    if abs(md) > 2 * sd:
        assert md < 0, (name, md, sd)
    else:
        print(f"{name}: RMSE difference within twice its standard error: nothing asserted")
