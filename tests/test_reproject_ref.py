"""What the reprojection definition of rt4.h does, on the CPU: the numpy restatement (reproject_ref.reproject) on
G-buffers made from numpy rays through the oracle's find_intersection (sphere scene, 61 x 37). No GPU: the HIP kernel is
held to this definition bit for bit in test_gpu_reproject.py.

The bounds on the kept share of eligible pixels are conditions on the definition, not measurements: moves inside the
camera's 3D slice must keep at least 0.9 of the history, moves that leave the slice at most 0.15."""
import numpy as np
import pytest

import denoise_ref
import reproject_ref

W, H = 61, 37


@pytest.fixture(scope="module")
def views(rt4, oracle):
    """{pose name: (uniforms, G-buffer)} and the default camera's, surfaces named by unique colours."""
    marked = rt4.SceneDesc.from_buffer_copy(rt4.Scene.named("sphere").to_bytes())
    table = denoise_ref.unique_colors(rt4, marked)
    reg = rt4.region(W, H)

    def view(u):
        g, hit, col = denoise_ref.gbuffer_reference(rt4, oracle, marked, u, reg)
        g["surface"] = denoise_ref.surfaces_from_colors(table, hit, col)
        g.setflags(write=False)
        return u, g

    out = {"prev": view(rt4.make_uniforms(W, H, samples=4, reflections=4))}
    for name, kind, amount in reproject_ref.POSES:
        out[name] = view(reproject_ref.pose_uniforms(rt4, W, H, kind, amount))
    return out


@pytest.fixture(scope="module")
def results(views):
    """{pose name: (acc_out, hist_out, details)}: a random old image, history 3 everywhere, default parameters."""
    u_prev, g_prev = views["prev"]
    acc = np.random.default_rng(5).random((H, W, 4)).astype(np.float32)
    hist = np.full((H, W), 3, np.int32)
    return {name: reproject_ref.reproject(views[name][0], views[name][1], u_prev, g_prev, acc, hist, details=True)
            for name, _, _ in reproject_ref.POSES}


def kept_share(res):
    d = res[2]
    assert d["eligible"].sum() > W * H // 4, "too few eligible pixels for the share to mean anything"
    assert not (d["kept"] & ~d["eligible"]).any()
    return d["kept"].sum() / d["eligible"].sum()


@pytest.mark.parametrize("name", reproject_ref.KEPT)
def test_moves_inside_the_slice_keep_history(results, name):
    share = kept_share(results[name])
    print(f"{name}: kept {share:.3f} of the eligible pixels")
    assert share >= 0.9


@pytest.mark.parametrize("name", reproject_ref.DROPPED)
def test_moves_out_of_the_slice_drop_history(results, name):
    share = kept_share(results[name])
    print(f"{name}: kept {share:.3f} of the eligible pixels")
    assert share <= 0.15


@pytest.mark.parametrize("name", reproject_ref.PARTIAL)
def test_small_w_move_keeps_some_and_drops_some(results, name):
    share = kept_share(results[name])
    print(f"{name}: kept {share:.3f} of the eligible pixels")
    assert 0.15 < share < 0.9


def test_identity_pose_returns_the_image(views, results):
    """At the identity pose fx, fy are the pixel's own coordinates up to rounding: every kept pixel's history is 3, and
    where all weight fell on the pixel itself the colour is the old one."""
    acc_out, hist_out, d = results["identity"]
    assert (hist_out[d["kept"]] == 3).all() and (hist_out[~d["kept"]] == 0).all()
    ys, xs = np.mgrid[0:H, 0:W]
    assert np.abs(d["fx"] - xs)[d["kept"]].max() < 1e-3 and np.abs(d["fy"] - ys)[d["kept"]].max() < 1e-3


@pytest.mark.parametrize("name", [n for n, _, _ in reproject_ref.POSES])
def test_screen_position_against_float64(views, results, name):
    """For eligible pixels whose four taps all count, (fx, fy) agrees with the projection computed in float64 from
    the float32 depth: to well under a pixel."""
    u_cur, g = views[name]
    u_prev, _ = views["prev"]
    d = results[name][2]
    sel = d["all4"]
    if name in reproject_ref.KEPT and name != "identity":  # identity: fx, fy sit on integers, most weights are 0
        assert sel.sum() > 100
    if not sel.any():
        return
    f64 = lambda v: np.array(list(v), np.float64)  # noqa: E731
    ys, xs = np.mgrid[0:H, 0:W]
    mx = ((xs + 0.5) / W - 0.5) * u_cur.mtr_sizes[0]
    my = (0.5 - (ys + 0.5) / H) * u_cur.mtr_sizes[1]
    dd = mx[..., None] * f64(u_cur.right_drct) + my[..., None] * f64(u_cur.top_drct) + f64(u_cur.vec_to_mtr)
    dd /= np.linalg.norm(dd, axis=2, keepdims=True)
    with np.errstate(all="ignore"):
        X = f64(u_cur.focus) + dd * g["depth"].astype(np.float64)[..., None]
        v = X - f64(u_prev.focus)
        F = f64(u_prev.vec_to_mtr)
        a = v @ F / (F @ F)
        fx = ((v @ f64(u_prev.right_drct)) / a / u_prev.mtr_sizes[0] + 0.5) * W - 0.5
        fy = (0.5 - (v @ f64(u_prev.top_drct)) / a / u_prev.mtr_sizes[1]) * H - 0.5
    err = max(np.abs(fx - d["fx"])[sel].max(), np.abs(fy - d["fy"])[sel].max())
    print(f"{name}: {sel.sum()} pixels with four taps, largest |f32 - f64| screen position {err:.2e} pixels")
    assert err < 1e-2


def test_reflective_pixels_and_misses_restart(views, results):
    _, g = views["x+0.05"]
    _, hist_out, d = results["x+0.05"]
    mirror = g["refl_prob"] > 0.5
    miss = g["surface"] < 0
    assert mirror.any() and miss.any()  # the mirror sphere (refl_prob 0.7) and the sky
    assert np.isclose(g["refl_prob"][mirror], 0.7).all()
    assert (hist_out[mirror | miss] == 0).all() and not d["eligible"][mirror | miss].any()


def test_history_takes_the_minimum_and_the_cap(views):
    u_prev, g_prev = views["prev"]
    u_cur, g_cur = views["x+0.05"]
    acc = np.zeros((H, W, 4), np.float32)
    hist = (np.arange(H * W, dtype=np.int32).reshape(H, W) % 7) * 100  # 0 .. 600, zeros included
    _, out, d = reproject_ref.reproject(u_cur, g_cur, u_prev, g_prev, acc, hist, details=True)
    assert out.max() == 255 and (out[d["kept"]] >= 100).all()
    _, out1 = reproject_ref.reproject(u_cur, g_cur, u_prev, g_prev, acc, hist, max_history=1)
    assert set(np.unique(out1)) == {0, 1}


def test_blend_reference_is_the_progressive_mix():
    rng = np.random.default_rng(11)
    new = rng.random((5, 7, 4)).astype(np.float32)
    acc = rng.random((5, 7, 4)).astype(np.float32)
    out, n = reproject_ref.blend(new, acc, np.zeros((5, 7), np.int32))
    assert (n == 1).all() and np.array_equal(out[..., :3], new[..., :3]) and (out[..., 3] == 1).all()  # part = 1
    out, n = reproject_ref.blend(new, acc, np.full((5, 7), 2 ** 31 - 1, np.int32))
    assert (n == 2 ** 31 - 1).all()  # saturates
    out8, _ = reproject_ref.blend(new, (acc * 255).astype(np.uint8), np.full((5, 7), 1, np.int32))
    assert out8.dtype == np.uint8 and (out8[..., 3] == 255).all()
