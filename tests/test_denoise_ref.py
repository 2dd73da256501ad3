"""What the filter definition of rt4.h buys, measured on the CPU: the numpy restatement (denoise_ref.atrous) on oracle
renders of the reference scenes, against the image the same settings converge to. No GPU: the HIP kernel is held to
this definition bit for bit in test_gpu_denoise.py."""
import numpy as np
import pytest

import denoise_ref

W, H, SPP, BOUNCES = 96, 64, 4, 4
TARGET_FRAMES = 256
ASSERTED = ["sphere", "room", "tiger", "cylinder4d", "hypercube"]
REPORTED = ["all_primitives", "tiger_two_mirrors"]  # glossy surfaces under the pass-through threshold: 0.155, 0.097


def mse_ratio(rt4, oracle, name):
    scene = rt4.Scene.named(name)
    reg = rt4.region(W, H)
    noisy, _, _, _ = oracle.render(scene.desc, rt4.make_uniforms(W, H, samples=SPP, reflections=BOUNCES, seed=12345), reg)
    base = rt4.make_uniforms(W, H, samples=SPP, reflections=BOUNCES, seed=777)
    target = np.zeros((H, W, 4), np.float32)
    for n in range(1, TARGET_FRAMES + 1):  # the reference's accumulation: mix(old, new, 1 / n)
        oracle.render(scene.desc, rt4.progressive_uniforms(base, n), reg, frame=target)
    # the G-buffer: numpy rays through the oracle's find_intersection, surfaces named by unique colours
    marked = rt4.SceneDesc.from_buffer_copy(scene.to_bytes())
    table = denoise_ref.unique_colors(rt4, marked)
    g, hit, col = denoise_ref.gbuffer_reference(rt4, oracle, marked, base, reg)
    g["surface"] = denoise_ref.surfaces_from_colors(table, hit, col)
    p = rt4.denoise_params()
    out = denoise_ref.atrous(noisy, g, p.levels, p.cos_min, p.depth_tol, p.max_refl_prob)
    filt = denoise_ref.filterable(g, p.max_refl_prob)
    assert filt.sum() > W * H // 8, "too few filterable pixels for the ratio to mean anything"
    assert np.array_equal(out[~filt].view(np.uint32), noisy[~filt].view(np.uint32))  # pass-through pixels keep their bits
    assert np.array_equal(out[..., 3].view(np.uint32), noisy[..., 3].view(np.uint32))  # alpha as stored
    t = target[..., :3].astype(np.float64)
    err_f = ((out[..., :3].astype(np.float64) - t)[filt] ** 2).mean()
    err_n = ((noisy[..., :3].astype(np.float64) - t)[filt] ** 2).mean()
    return err_f / err_n


@pytest.mark.parametrize("name", ASSERTED)
def test_filter_reduces_error(rt4, oracle, name):
    ratio = mse_ratio(rt4, oracle, name)
    print(f"{name}: filtered MSE / noisy MSE = {ratio:.4f}")
    assert ratio <= 0.1


@pytest.mark.parametrize("name", REPORTED)
def test_filter_on_glossy_scenes_reported(rt4, oracle, name):
    ratio = mse_ratio(rt4, oracle, name)
    print(f"{name}: filtered MSE / noisy MSE = {ratio:.4f} (reported, not bounded)")
    assert np.isfinite(ratio)


def test_fma32_is_single_rounded():
    a, b = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23)  # a*b = 1 + 2^-22 + 2^-46
    c = np.float32(2.0 ** -24)  # sum = 1 + 2^-22 + 2^-24 + 2^-46: just above the tie between two float32
    assert denoise_ref.fma32(a, b, c)[0] == np.float32(1 + 2.0 ** -22 + 2.0 ** -23)
    # an exact tie goes to the even neighbour: 2^30 + 2^7 + 2^6 with ulp 2^7
    x = denoise_ref.fma32(np.float32(2.0 ** 30), np.float32(1 + 2.0 ** -23), np.float32(2.0 ** 6))[0]
    assert x == np.float32(2.0 ** 30 + 2.0 ** 8)
    # (2^40 + 2^17) * 1.5 is a float32 tie (ulp 2^17, + 2^16); - 2^-30 puts the sum just under it, which float64
    # cannot hold (71 bits): rounding the float64 sum again would take the tie to the even neighbour above
    lo = np.float32(2.0 ** 40 + 2.0 ** 39 + 2.0 ** 17)
    y = denoise_ref.fma32(np.float32(2.0 ** 40 + 2.0 ** 17), np.float32(1.5), np.float32(-(2.0 ** -30)))[0]
    assert y == lo
    assert np.float32(np.float64(2.0 ** 40 + 2.0 ** 17) * 1.5 - 2.0 ** -30) != lo  # the shortcut is wrong here
    z = denoise_ref.fma32(np.float32(3.0), np.float32(-0.0), np.float32(-0.0))[0]
    assert z == 0 and np.signbit(z)
