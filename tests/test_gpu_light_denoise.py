"""The HIP variance-guided filter of a light accumulator (rt4.h rt4_light_denoise_device) against its definition
restated in numpy (light_denoise_ref), bit for bit: rendered accumulators at every level count and in every format,
degenerate sizes with padded and poisoned strides, a synthetic accumulator and guide with the awkward values, host
against device, the argument errors, the neighbours on the same context, one end-to-end reason and the --light-denoise
switch of the host program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import denoise_ref
import light_denoise_ref as ldr
import light_ref

pytestmark = pytest.mark.gpu

ERR_ARG = -1
DT = {0: np.float32, 1: np.float16, 2: np.uint8}
FMT_IDS = ["f32", "f16", "rgba8"]
W, H = 33, 17
POISON = 0xAB


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def params_kw(p):
    return dict(levels=p.levels, cos_min=p.cos_min, depth_tol=p.depth_tol, max_refl_prob=p.max_refl_prob, sigma=p.sigma,
                eps=p.eps)


def as_ref(acc):
    return np.ascontiguousarray(acc).view(light_ref.LIGHT_DTYPE)


def same_frame(got, want):
    """Equal stored frames; in the float formats any NaN matches any NaN (rt4.h leaves the payload undefined)."""
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype == np.uint8:
        return raw(got) == raw(want)
    return light_ref.same_floats(got.astype(np.float32), want.astype(np.float32))


def check(rt4, tracer, acc, g, k, p, what, fmts=(0, 1, 2)):
    """Device against reference: the frame in every format of fmts, with d_filtered given and NULL."""
    acc_rt = np.ascontiguousarray(acc).view(rt4.LIGHT_DTYPE)
    out = None
    for fmt in fmts:
        want, want_fl = ldr.light_denoise(as_ref(acc), g, k, DT[fmt], **params_kw(p))
        got, got_fl = tracer.light_denoise_host(acc_rt, g, k, p, fmt, filtered=True)
        assert same_frame(got, want), (what, FMT_IDS[fmt])
        assert light_ref.same_floats(got_fl, want_fl), (what, FMT_IDS[fmt], "filtered")
        alone = tracer.light_denoise_host(acc_rt, g, k, p, fmt)
        assert same_frame(alone, want), (what, FMT_IDS[fmt], "no filtered output")
        out = out if out is not None else (got, got_fl)
    return out


# ------------------------------------------------------------------------------------------ 1. rendered accumulators
@pytest.fixture(scope="module")
def rendered(rt4, tracer_lut):
    """{scene: (G-buffer, {frames: accumulator}, k)} at 33 x 17, 4 spp, rendered on the GPU once; read-only."""
    out = {}
    reg = rt4.region(W, H)
    for name in ("sphere", "all_primitives"):
        tracer_lut.set_scene(rt4.Scene.named(name))
        us = [rt4.make_uniforms(W, H, samples=4, reflections=4, seed=s) for s in range(1, 17)]
        g = tracer_lut.render_gbuffer_host(us[0], reg)
        acc3, _ = tracer_lut.render_light_host(us[:3], reg)
        acc16 = acc3.copy()
        tracer_lut.render_light_host(us[3:], reg, acc16)
        for a in (g, acc3, acc16):
            a.setflags(write=False)
        out[name] = (g, {3: acc3, 16: acc16}, us[0].light_to_color_conversion_coefficient)
    return out


@pytest.mark.parametrize("frames", [3, 16])
@pytest.mark.parametrize("name", ["sphere", "all_primitives"])
def test_rendered_accumulators_every_level(rt4, tracer_lut, rendered, name, frames):
    """Levels 0, 1, 2 (the LDS strides), 3, 5 and 6 (the gather strides; from level 5 on only the centre row counts in
    y at 17 rows), the three formats, d_filtered NULL and given."""
    g, accs, k = rendered[name]
    acc = accs[frames]
    ids = ldr.state0(as_ref(acc), g, 0.5)[0]
    filt = ids >= 0
    assert filt.any() and (~filt).any() and (acc["n"] == frames).all()
    if name == "all_primitives":
        assert ((g["surface"] >= 0) & ~filt).any()  # reflective pixels pass through
    plain = {fmt: tracer_lut.light_resolve_host(np.ascontiguousarray(acc), k, fmt) for fmt in (0, 1, 2)}
    for levels in (0, 1, 2, 3, 5, 6):
        for fmt in (0, 1, 2):
            got, got_fl = check(rt4, tracer_lut, acc, g, k, rt4.light_denoise_params(levels=levels), (name, frames, levels),
                                fmts=(fmt,))
            assert raw(got[~filt]) == raw(plain[fmt][~filt])
            if levels == 0:
                assert raw(got) == raw(plain[fmt])
            elif fmt == 0:
                assert raw(got) != raw(plain[fmt])  # the filter did something
    assert tracer_lut.light_denoise_bytes() >= W * H * 64


# ------------------------------------------------------------------------------------------ 2. sizes and strides
def random_gbuffer(rt4, h, w, seed):
    """Two surfaces in blocks, a few misses, normals and depths scattered around the defaults' thresholds."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), rt4.GBUFFER_DTYPE)
    sid = (xs // 3 + ys // 2) % 2
    sid[rng.random((h, w)) < 0.1] = -1
    n = np.array([0.0, 0.0, 1.0, 0.0]) + rng.normal(0, 0.2, (h, w, 4))
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    g["normal"] = np.where((sid >= 0)[..., None], n, 0).astype(np.float32)
    g["depth"] = np.where(sid >= 0, 3.0 + rng.normal(0, 0.15, (h, w)), np.inf).astype(np.float32)
    g["surface"] = sid
    g["refl_prob"] = np.where(sid >= 0, rng.choice(np.array([0.0, 0.3, 0.7], np.float32), (h, w), p=[0.6, 0.3, 0.1]), 0)
    return g


def random_acc(rt4, h, w, seed):
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w), rt4.LIGHT_DTYPE)
    a["mean"] = (rng.random((h, w, 3)) * rng.choice([0.1, 1.0, 20.0], (h, w, 1))).astype(np.float32)
    a["mean_y"] = light_ref.luminance(a["mean"])
    a["m2"] = (rng.random((h, w)) * rng.choice([0.0, 0.01, 1.0, 100.0], (h, w))).astype(np.float32)
    a["n"] = rng.choice(np.array([0, 1, 2, 5, 40], np.int32), (h, w), p=[0.05, 0.05, 0.3, 0.3, 0.3])
    a["reserved"] = 7.0
    return a


def _pad(a, w, extra, item):
    """a's rows padded by `extra` elements of `item` bytes that hold other bytes."""
    wide = np.zeros((a.shape[0], w + extra) + a.shape[2:], a.dtype)
    wide.view(np.uint8).reshape(a.shape[0], w + extra, item)[:, w:] = POISON
    wide[:, :w] = a
    return wide


def padding_kept(wide, w):
    item = wide.dtype.itemsize * int(np.prod(wide.shape[2:], dtype=np.int64))
    return (wide.view(np.uint8).reshape(wide.shape[0], wide.shape[1], item)[:, w:] == POISON).all()


@pytest.mark.parametrize("w, h, pads", [(1, 1, (1, 2, 3, 4)), (5, 3, (2, 0, 1, 3)), (8, 8, (0, 1, 0, 2)), (64, 1, (3, 1, 2, 0)),
                                        (3, 40, (1, 3, 0, 2)), (33, 17, (0, 0, 0, 0)), (33, 17, (7, 0, 0, 0)),
                                        (33, 17, (0, 5, 3, 0)), (33, 17, (1, 2, 3, 4))])
def test_sizes_and_padded_strides(rt4, tracer_lut, w, h, pads):
    """Accumulator, G-buffer, frame and filtered light each with its own row padding, poisoned: the image is the
    reference's and every output's padding keeps its bytes."""
    acc, g = random_acc(rt4, h, w, 10 + w), random_gbuffer(rt4, h, w, 20 + h)
    for fmt, levels in ((0, 1), (1, 3), (2, 6), (0, 4)):
        p = rt4.light_denoise_params(levels=levels, cos_min=0.8, depth_tol=0.08)
        want, want_fl = ldr.light_denoise(as_ref(acc), g, 0.9, DT[fmt], **params_kw(p))
        acc_w, g_w = _pad(acc, w, pads[0], 32), _pad(g, w, pads[1], 32)
        out = _pad(np.zeros((h, w, 4), DT[fmt]), w, pads[2], 4 * np.dtype(DT[fmt]).itemsize)
        fl = _pad(np.zeros((h, w, 4), np.float32), w, pads[3], 16)
        tracer_lut.light_denoise_host(acc_w, g_w, 0.9, p, fmt, out=out, filtered=fl, w=w)
        assert same_frame(out[:, :w], want), (w, h, pads, fmt, levels)
        assert light_ref.same_floats(fl[:, :w], want_fl), (w, h, pads, fmt, levels)
        assert padding_kept(out, w) and padding_kept(fl, w)


# ------------------------------------------------------------------------------------------ 3. the awkward values
COS_MIN, DEPTH_TOL = np.float32(0.9), np.float32(0.25)


def awkward(rt4):
    """An 11 x 5 accumulator and guide no renderer made (see test_awkward_values)."""
    h, w = 5, 11
    rng = np.random.default_rng(42)
    a = np.zeros((h, w), rt4.LIGHT_DTYPE)
    a["mean"] = (rng.random((h, w, 3)) * 2).astype(np.float32)
    a["mean_y"] = light_ref.luminance(a["mean"])
    a["m2"] = (rng.random((h, w)) * 0.5).astype(np.float32)
    a["n"] = 4
    g = np.zeros((h, w), rt4.GBUFFER_DTYPE)
    g["normal"] = (0, 0, 1, 0)
    g["depth"] = 2.0
    g["surface"] = 0
    g["refl_prob"] = 0.3
    # row 0: n of 0, 1, 2 and INT32_MAX; m2 of 0, 1e30, inf, NaN and negative
    a["n"][0, 0:4] = [0, 1, 2, light_ref.INT32_MAX]
    a["m2"][0, 4:9] = [0.0, 1e30, np.inf, np.nan, -1.0]
    # row 1: mean_y of inf and NaN; misses next to hits; refl_prob on both sides of a threshold
    a["mean_y"][1, 0:2] = [np.inf, np.nan]
    g["surface"][1, 3] = g["surface"][1, 5] = -1
    g["normal"][1, 3] = g["normal"][1, 5] = 0
    g["depth"][1, 3] = g["depth"][1, 5] = np.inf
    g["refl_prob"][1, 7:10] = [0.5, 0.50000006, 0.7]
    # rows 2-4, columns 0-1: a surface one pixel wide (column 1)
    g["surface"][2:, 1] = 3
    # row 2, columns 3-6: normals whose dot with (0, 0, 1, 0) is exactly cos_min and one ulp below
    for x, c in ((4, COS_MIN), (6, np.nextafter(COS_MIN, np.float32(0)))):
        g["normal"][2, x] = (np.sqrt(np.float32(1) - c * c), 0, c, 0)
    # row 3, columns 3-6: a depth difference exactly at the tolerance of z_p = 2 and one ulp beyond
    g["depth"][3, 4] = np.float32(2.5)
    g["depth"][3, 6] = np.nextafter(np.float32(2.5), np.float32(np.inf))
    # row 4, columns 3-10: zero variance and equal luminance (t = 0/0 when eps = 0), next to unequal luminance
    a["m2"][3:, 7:] = 0.0
    a["mean_y"][4, 7:10] = 0.75
    return a, g


def test_awkward_values(rt4, tracer_lut):
    """n of 0, 1, 2 and INT32_MAX; m2 of 0, 1e30, inf, NaN and negative; mean_y of inf and NaN; misses next to hits; a
    surface one pixel wide; normals whose dot is exactly cos_min and one ulp below; a depth difference exactly at the
    tolerance and one ulp beyond; eps = 0 with zero variance; sigma 0 and +inf; max_refl_prob at a pixel's own value."""
    a, g = awkward(rt4)
    up = np.array([0, 0, 1, 0], np.float32)
    assert denoise_ref.dot4(up, g["normal"][2, 4])[0] == COS_MIN and denoise_ref.dot4(up, g["normal"][2, 6])[0] < COS_MIN
    tol = DEPTH_TOL * g["depth"][3, 3]
    assert abs(g["depth"][3, 4] - g["depth"][3, 3]) == tol and abs(g["depth"][3, 6] - g["depth"][3, 5]) > tol
    base = dict(cos_min=float(COS_MIN), depth_tol=float(DEPTH_TOL))
    variants = {"plain": {}, "eps 0": dict(eps=0.0), "sigma 0": dict(sigma=0.0), "sigma 0, eps 0": dict(sigma=0.0, eps=0.0),
                "sigma inf": dict(sigma=float("inf")), "refl at 0.3": dict(max_refl_prob=float(np.float32(0.3))),
                "refl at 0.5": dict(max_refl_prob=0.5), "refl below": dict(max_refl_prob=0.29)}
    for what, kw in variants.items():
        for levels in (1, 2, 3, 4):
            p = rt4.light_denoise_params(levels=levels, **base, **kw)
            _, fl = check(rt4, tracer_lut, a, g, 0.8, p, (what, levels), fmts=(0, 1, 2) if what == "plain" else (0,))
        if what == "plain":
            assert np.isnan(fl[..., 3]).any() and np.isposinf(fl[..., 3]).any()  # the NaN and inf m2 got somewhere
    ids = ldr.state0(as_ref(a), g, 0.3)[0]
    assert (ids[1, 7:10] == -1).all() and ids[2, 2] == 0 and (ids[0, :4] == [-1, -1, 0, 0]).all()
    assert (ldr.state0(as_ref(a), g, 0.29)[0] == -1).all()


# ------------------------------------------------------------------------------------------ 4. device entry point
def test_device_call_host_call_and_scratch(rt4, tracer_lut, rendered):
    """rt4_light_denoise_device on device buffers equals rt4_light_denoise_host; the accumulator and the G-buffer are
    only read; rt4_context_denoise_bytes does not move; the scratch grows with the image."""
    import torch

    g, accs, k = rendered["sphere"]
    acc = accs[16]
    stream = torch.cuda.current_stream().cuda_stream
    d_acc = torch.from_numpy(acc.view(np.uint8).reshape(H, W * 32).copy()).cuda()
    d_g = torch.from_numpy(g.view(np.uint8).reshape(H, W * 32).copy()).cuda()
    d_frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    d_fl = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    colour_bytes, before = tracer_lut.denoise_bytes(), tracer_lut.light_denoise_bytes()
    p = rt4.light_denoise_params()
    tracer_lut.light_denoise_device(d_acc.data_ptr(), W, d_g.data_ptr(), W, k, d_frame.data_ptr(), 0, W, W, H, p,
                                    d_fl.data_ptr(), W, stream)
    torch.cuda.synchronize()
    want, want_fl = tracer_lut.light_denoise_host(np.ascontiguousarray(acc), np.ascontiguousarray(g), k, p, filtered=True)
    assert raw(d_frame.cpu().numpy()) == raw(want) and raw(d_fl.cpu().numpy()) == raw(want_fl)
    assert raw(d_acc.cpu().numpy()) == raw(acc) and raw(d_g.cpu().numpy()) == raw(g)
    assert tracer_lut.denoise_bytes() == colour_bytes
    assert tracer_lut.light_denoise_bytes() == max(before, W * H * 64)
    big = (48, 40)
    a2, g2 = random_acc(rt4, big[1], big[0], 1), random_gbuffer(rt4, big[1], big[0], 2)
    tracer_lut.light_denoise_host(a2, g2, k, rt4.light_denoise_params(levels=0))  # no levels: no scratch
    assert tracer_lut.light_denoise_bytes() == max(before, W * H * 64)
    tracer_lut.light_denoise_host(a2, g2, k, p)
    assert tracer_lut.light_denoise_bytes() == max(before, big[0] * big[1] * 64) and tracer_lut.denoise_bytes() == colour_bytes
    # the smaller image again, in the larger scratch
    again = tracer_lut.light_denoise_host(np.ascontiguousarray(acc), np.ascontiguousarray(g), k, p)
    assert raw(again) == raw(want)


def test_argument_errors_write_nothing(rt4, tracer_lut):
    import torch

    w, h = 16, 8
    row = w * 32
    # rows of w 32-B records: accumulator rows 0..7, G-buffer rows 8..15, an fp32 frame rows 16..19, filtered rows 20..23
    buf = torch.full((24 * w, 8), 0.25, dtype=torch.float32, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    p0 = buf.data_ptr()
    light, gbuf, frame, filt = p0, p0 + 8 * row, p0 + 16 * row, p0 + 20 * row
    ok = rt4.light_denoise_params()

    def status(light=light, ls=w, gbuf=gbuf, gs=w, frame=frame, fmt=0, fs=w, filt=filt, fls=w, ww=w, hh=h, p=ok):
        try:
            tracer_lut.light_denoise_device(light, ls, gbuf, gs, 1.0, frame, fmt, fs, ww, hh, p, filt, fls, stream)
        except rt4.RT4Error as e:
            return e.status
        return 0

    assert status(light=0) == ERR_ARG and status(gbuf=0) == ERR_ARG and status(frame=0) == ERR_ARG
    err = ctypes.create_string_buffer(256)
    assert rt4.lib.rt4_light_denoise_device(tracer_lut._h, light, w, gbuf, w, 1.0, None, frame, 0, w, filt, w, w, h, stream,
                                            err, len(err)) == ERR_ARG  # no parameters
    assert status(fmt=9) == ERR_ARG
    assert status(ww=0) == ERR_ARG and status(hh=0) == ERR_ARG and status(ww=65536, ls=65536, gs=65536, fs=65536, fls=65536) == ERR_ARG
    assert status(ls=w - 1) == ERR_ARG and status(gs=w - 1) == ERR_ARG and status(fs=w - 1) == ERR_ARG and status(fls=w - 1) == ERR_ARG
    assert status(light=light + 8) == ERR_ARG and status(gbuf=gbuf + 8) == ERR_ARG and status(filt=filt + 8) == ERR_ARG
    assert status(frame=frame + 8) == ERR_ARG and status(frame=frame + 2, fmt=2) == ERR_ARG and status(frame=frame + 4, fmt=1) == ERR_ARG
    for levels in (-1, 7):
        assert status(p=rt4.light_denoise_params(levels=levels)) == ERR_ARG
    for kw in (dict(sigma=-1.0), dict(sigma=float("nan")), dict(eps=-1e-9), dict(eps=float("nan"))):
        assert status(p=rt4.light_denoise_params(**kw)) == ERR_ARG, kw
    assert status(frame=light + 8 * row - 16) == ERR_ARG  # the frame's first pixel is the accumulator's last half record
    assert status(frame=gbuf + 16) == ERR_ARG and status(filt=gbuf) == ERR_ARG and status(filt=light + 16) == ERR_ARG
    assert status(filt=frame) == ERR_ARG and status(filt=frame + 4 * row - 16) == ERR_ARG  # the two outputs
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)
    # adjacent, not overlapping: accepted; the inputs keep their bytes
    assert status() == 0 and status(filt=0, fls=0) == 0 and status(p=rt4.light_denoise_params(sigma=float("inf"), eps=0.0)) == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:16 * w]) == raw(before[:16 * w])
    acc = before[:8 * w].view(rt4.LIGHT_DTYPE).reshape(h, w)
    g = before[8 * w:16 * w].view(rt4.GBUFFER_DTYPE).reshape(h, w)
    want, want_fl = ldr.light_denoise(as_ref(acc), g, 1.0, sigma=float("inf"), eps=0.0)
    assert raw(after[16 * w:20 * w]) == raw(want)
    assert light_ref.same_floats(after[20 * w:24 * w].reshape(h, w, 4), want_fl)


def test_neighbours_on_the_same_context_afterwards(rt4, tracer_lut, rendered, oracle):
    """rt4_denoise_device, rt4_light_resolve_device and rt4_render_device_ex after light-denoise calls on the same
    context still equal their references."""
    g, accs, k = rendered["sphere"]
    acc = np.ascontiguousarray(accs[16])
    tracer_lut.light_denoise_host(acc, np.ascontiguousarray(g), k)
    scene = rt4.Scene.named("sphere")
    tracer_lut.set_scene(scene)
    reg = rt4.region(W, H)
    u = rt4.make_uniforms(W, H, samples=2, reflections=3, seed=99, part=1.0)
    frame = np.zeros((H, W, 4), np.float32)
    tracer_lut.render_host_ex(u, reg, frame, 0)
    want, _ = oracle.render_fmt(scene.desc, u, reg, 0)
    assert raw(frame) == raw(want)
    assert raw(tracer_lut.light_resolve_host(acc, k)) == raw(light_ref.resolve(as_ref(acc), k))
    gb = tracer_lut.render_gbuffer_host(u, reg)
    assert raw(tracer_lut.denoise_host(frame, gb)) == raw(denoise_ref.atrous(frame, gb))
    tracer_lut.light_denoise_host(acc, np.ascontiguousarray(g), k, rt4.light_denoise_params(levels=2))
    assert raw(tracer_lut.denoise_host(frame, gb)) == raw(denoise_ref.atrous(frame, gb))


# ------------------------------------------------------------------------------------------ 5. the reason
def test_filtered_image_is_closer_to_the_converged_one(rt4, tracer_lut):
    """Sphere at 96 x 64: 16 light frames of 4 spp, filtered, against one 4096-spp frame, all on the GPU. The filtered
    MSE over the filterable pixels is below the plain resolve's (test_light_denoise_ref.py has the table)."""
    w, h = 96, 64
    reg = rt4.region(w, h)
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    base = rt4.make_uniforms(w, h, samples=4, reflections=4, seed=777)
    us = [rt4.progressive_uniforms(base, n) for n in range(1, 17)]
    acc, _ = tracer_lut.render_light_host(us, reg)
    k = base.light_to_color_conversion_coefficient
    g = tracer_lut.render_gbuffer_host(base, reg)
    ref = np.zeros((h, w, 4), np.float32)
    tracer_lut.render_host_ex(rt4.make_uniforms(w, h, samples=4096, reflections=4, seed=4242, part=1.0), reg, ref, 0)
    plain = tracer_lut.light_resolve_host(acc, k)
    got = tracer_lut.light_denoise_host(acc, g, k)
    filt = ldr.state0(as_ref(acc), g, 0.5)[0] >= 0
    assert filt.sum() > w * h // 8
    t = ref[..., :3].astype(np.float64)
    mse_f = ((got[..., :3].astype(np.float64) - t)[filt] ** 2).mean()
    mse_p = ((plain[..., :3].astype(np.float64) - t)[filt] ** 2).mean()
    print(f"sphere 96 x 64, 4 spp x 16: filtered MSE / plain MSE = {mse_f / mse_p:.4f}")
    assert mse_f < mse_p


# ------------------------------------------------------------------------------------------ 6. rt4_render --light-denoise
def render_paths(rt4):
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    return os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")


def frame_seed(seed, n):
    return seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)


def test_cpp_host_light_denoise_sections_and_window(rt4, tracer_lut, tmp_path):
    """rt4_render -3 --light --light-denoise 3 --window 2 on tiger: every section's plain resolve, _ldn image and _win
    image (the filtered frame upscaled) equal the same steps from Python."""
    import torch

    exe, props_path = render_paths(rt4)
    pre, seed, frames, levels, s = str(tmp_path / "s"), 99, 3, 3, 2
    r = subprocess.run([exe, "-p", props_path, "-s", "tiger", "-n", str(frames), "-3", "--seed", str(seed), "--light",
                        "--light-denoise", str(levels), "--window", str(s), "-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    tracer_lut.set_scene(rt4.Scene.builtin("tiger"))
    sections = [(rt4.SECTION_YXZ, "yxz", "main"), (rt4.SECTION_YWZ, "ywz", "additional"), (rt4.SECTION_YXW, "yxw", "additional")]
    for sec, tag, window in sections:
        w, h = rt4.window_cells(props, window)
        base = rt4.uniforms_from_properties(props, w, h, sec)
        cam = rt4.Camera(props)
        us = [cam.frame_uniforms(base, sec, frame_seed(seed, n)) for n in range(1, frames + 1)]
        k = base.light_to_color_conversion_coefficient
        acc, _ = tracer_lut.render_light_host(us, rt4.region(w, h))
        g = tracer_lut.render_gbuffer_host(us[-1], rt4.region(w, h))
        ldn = tracer_lut.light_denoise_host(acc, g, k, rt4.light_denoise_params(levels=levels))
        d_ldn = torch.from_numpy(ldn).cuda()
        win = rt4.Window(tracer_lut, w, h, s, 0)
        try:
            win.present(us[-1], d_ldn.data_ptr())
            images = (("", tracer_lut.light_resolve_host(acc, k)), ("_ldn", ldn), ("_win", win.image()))
            for suffix, image in images:
                path = str(tmp_path / f"py_{tag}{suffix}.ppm")
                rt4.write_ppm(path, image)
                assert open(path, "rb").read() == open(f"{pre}_{tag}{suffix}.ppm", "rb").read(), (tag, suffix)
        finally:
            win.close()
        assert not os.path.exists(f"{pre}_{tag}_dn.ppm")
    assert raw(ldn) == raw(ldr.light_denoise(as_ref(acc), g, k, levels=levels)[0])


def test_cpp_host_light_denoise_default_levels_and_refusals(rt4, tracer_lut, tmp_path):
    exe, props_path = render_paths(rt4)
    w, h, seed, frames = 40, 24, 5, 4
    common = [exe, "-p", props_path, "-s", "sphere", "-W", str(w), "-H", str(h), "-n", str(frames), "--seed", str(seed)]
    pre = str(tmp_path / "d")
    r = subprocess.run(common + ["--light", "--light-denoise", "-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, w, h)
    cam = rt4.Camera(props)
    us = [cam.frame_uniforms(base, rt4.SECTION_YXZ, frame_seed(seed, n)) for n in range(1, frames + 1)]
    tracer_lut.set_scene(rt4.Scene.builtin("sphere"))
    acc, _ = tracer_lut.render_light_host(us, rt4.region(w, h))
    g = tracer_lut.render_gbuffer_host(us[-1], rt4.region(w, h))
    rt4.write_ppm(str(tmp_path / "py.ppm"), tracer_lut.light_denoise_host(acc, g, base.light_to_color_conversion_coefficient))
    assert open(str(tmp_path / "py.ppm"), "rb").read() == open(pre + "_yxz_ldn.ppm", "rb").read()
    assert open(pre + "_yxz_ldn.ppm", "rb").read() != open(pre + "_yxz.ppm", "rb").read()
    # --light --denoise without the new flag: the colour filter on the resolved image, as before
    r = subprocess.run(common + ["--light", "--denoise", "2", "-o", str(tmp_path / "c")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    dn = tracer_lut.denoise_host(tracer_lut.light_resolve_host(acc, base.light_to_color_conversion_coefficient), g,
                                 rt4.denoise_params(levels=2))
    rt4.write_ppm(str(tmp_path / "py_dn.ppm"), dn)
    assert open(str(tmp_path / "py_dn.ppm"), "rb").read() == open(str(tmp_path / "c_yxz_dn.ppm"), "rb").read()
    assert not os.path.exists(str(tmp_path / "c_yxz_ldn.ppm"))
    # refused: without --light, together with --denoise, a level count out of range; --gpus stays refused with --light
    for extra in (["--light-denoise"], ["--light", "--light-denoise", "--denoise"], ["--light", "--light-denoise", "7"]):
        r = subprocess.run(common + extra + ["-o", str(tmp_path / "x")], capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--light-denoise" in r.stderr, (extra, r.stderr)
    r = subprocess.run(common + ["--light", "--light-denoise", "--gpus", "2", "-o", str(tmp_path / "x")], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode != 0 and "--light" in r.stderr
