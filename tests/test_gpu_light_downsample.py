"""The HIP downsample of supersampled light accumulators (rt4.h rt4_light_downsample_device / _host) on
the GPU: against its definition restated in numpy (supersample_ref) bit for bit on real renders, on an accumulator
with unequal n and on synthetic edge cases, the device entry against the host entry, the argument errors, and
rt4_render --supersample against the same steps from Python."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import light_ref
import supersample_ref

pytestmark = pytest.mark.gpu

ERR_ARG = -1
W, H, PAD = 33, 17, 3  # a partial 32 x 8 block both ways; both strides padded by 3 pixels
SS = [1, 2, 3, 4, 8]  # the unrolled sub-rows (1, 2), the rolled ones with a partial batch (3), a full one (4) and two (8)
INT32_MAX = 2 ** 31 - 1


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def as_ref(acc):
    return np.ascontiguousarray(acc).view(light_ref.LIGHT_DTYPE)


def poison(rt4, shape, seed):
    """Random bytes as accumulators: what padding holds."""
    n = int(np.prod(shape))
    return np.frombuffer(np.random.default_rng(seed).bytes(n * 32), rt4.LIGHT_DTYPE).reshape(shape).copy()


def padded(rt4, image, seed):
    out = poison(rt4, (image.shape[0], image.shape[1] + PAD), seed)
    out[:, :image.shape[1]] = image
    return out


@pytest.fixture(scope="module")
def tracer(rt4):
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT)
    yield t
    t.close()


def check(rt4, tracer, fine_img, s):
    """The host entry on padded, poisoned buffers against the reference; returns the output image."""
    fine = padded(rt4, fine_img, seed=1)
    out = poison(rt4, (H, W + PAD), seed=2)
    before_out, before_fine = out.copy(), raw(fine)
    got = tracer.light_downsample_host(fine, s, out=out, w=W, h=H)
    want = supersample_ref.downsample(as_ref(fine_img), s)
    assert light_ref.same_acc(as_ref(got[:, :W]), want), s
    assert raw(got[:, W:]) == raw(before_out[:, W:])  # the padding keeps its bytes
    assert raw(fine) == before_fine
    return got[:, :W]


@pytest.fixture(scope="module")
def renders(rt4, tracer):
    """{(scene, s): the (17 s) x (33 s) accumulator of 3 frames of the view at s times the resolution}, read-only."""
    out = {}
    for name in ("sphere", "tiger"):
        tracer.set_scene(rt4.Scene.named(name))
        for s in (2, 3):
            base = rt4.upscale_uniforms(rt4.make_uniforms(W, H, samples=2, reflections=3, seed=77), s)
            us = [rt4.progressive_uniforms(base, n) for n in range(1, 4)]
            acc = tracer.render_light_host(us, rt4.region(W * s, H * s))[0]
            acc.setflags(write=False)
            out[name, s] = acc
    return out


@pytest.mark.parametrize("s", [2, 3])
@pytest.mark.parametrize("name", ["sphere", "tiger"])
def test_downsample_of_real_renders_against_the_reference(rt4, tracer, renders, name, s):
    got = check(rt4, tracer, renders[name, s], s)
    assert (got["n"] == 3).all() and (got["m2"] > 0).any() and not got["reserved"].any()


def test_unequal_n_keeps_equal_weights(rt4, tracer, renders):
    """A second render over a banded region of the fine image, bands of 3 rows every 7: strata of one output pixel
    with n = 3 and n = 5 (a band of 3 fine rows cuts through an output row), the output's n their minimum."""
    s = 2
    tracer.set_scene(rt4.Scene.named("sphere"))
    base = rt4.upscale_uniforms(rt4.make_uniforms(W, H, samples=2, reflections=3, seed=77), s)
    fine = renders["sphere", s].copy()
    rows = [2, 3, 4, 9, 10, 11, 16, 17, 18]  # local row i of the region is image row 2 + (i // 3) * 7 + i % 3
    band = np.ascontiguousarray(fine[rows])
    tracer.render_light_host([rt4.progressive_uniforms(base, n) for n in (4, 5)], rt4.region(W * s, 9, y0=2, band_rows=3, band_step=7),
                             band)
    fine[rows] = band
    assert (fine["n"][rows] == 5).all() and (fine["n"].sum() == 3 * fine.size + 2 * 9 * W * s)
    got = check(rt4, tracer, fine, s)
    assert (got["n"][1] == 5).all() and (got["n"][2] == 3).all() and (got["n"][4] == 3).all() and (got["n"][5] == 5).all()
    assert (got["n"][9] == 3).all() and (got["n"] == 5).sum() == 3 * W


def synthetic(rt4, s, seed):
    """Edge cases in every stratum position: n = 0, 1 and INT32_MAX, inf and NaN means and m2, -0.0f and denormals."""
    rng = np.random.default_rng(seed)
    h, w = H * s, W * s
    a = np.zeros((h, w), rt4.LIGHT_DTYPE)
    a["mean"] = (rng.random((h, w, 3)) * rng.choice([0.0, 0.1, 1.0, 50.0], (h, w, 1))).astype(np.float32)
    a["mean_y"] = light_ref.luminance(a["mean"])
    a["m2"] = (rng.random((h, w)) * rng.choice([0.0, 1.0, 1e6], (h, w))).astype(np.float32)
    a["n"] = rng.choice(np.array([2, 3, 5, 1000, 2 ** 30, INT32_MAX - 1, INT32_MAX], np.int32), (h, w))
    rare = 0.3 / (s * s)  # so that most output pixels hold at most one special stratum
    for n_special in (0, 1):
        a["n"][rng.random((h, w)) < rare] = n_special
    specials = np.array([np.inf, -np.inf, np.nan, -0.0, 1e-45, 3e-39, -2e-40], np.float32)
    for field in ("mean_y", "m2"):
        hit = rng.random((h, w)) < rare
        a[field][hit] = rng.choice(specials, int(hit.sum()))
    hit = rng.random((h, w)) < rare
    a["mean"][hit, 1] = rng.choice(specials, int(hit.sum()))
    # whatever the draw: pixel (0, 0) all -0.0f with n = INT32_MAX, pixel (1, 0) denormal means and m2, pixel (2, 0)
    # only its last stratum empty, pixel (3, 0) only its first stratum with one frame
    a[0:s, 0:s] = np.zeros((), rt4.LIGHT_DTYPE)
    for field in ("mean", "mean_y", "m2"):
        a[field][0:s, 0:s] = -0.0
        a[field][0:s, s:2 * s] = 1e-41
    a["n"][0:s, 0:s] = INT32_MAX
    a["n"][0:s, s:2 * s] = 2
    a["n"][0:s, 2 * s:4 * s] = 7
    a["n"][s - 1, 3 * s - 1] = 0
    a["n"][0, 3 * s] = 1
    return a


@pytest.mark.parametrize("s", SS)
def test_downsample_of_edge_cases_against_the_reference(rt4, tracer, s):
    fine = synthetic(rt4, s, seed=300 + s)
    got = check(rt4, tracer, fine, s)
    empty = np.zeros((), rt4.LIGHT_DTYPE).tobytes()
    assert got[0, 2].tobytes() == empty and (got["n"] == 0).sum() > 1
    assert got["n"][0, 3] == 1 and got["m2"][0, 3] == 0
    assert got["n"][0, 0] == INT32_MAX and raw(got["mean"][0, 0]) == raw(np.zeros(3, np.float32))  # -0.0f sums to +0.0f
    assert got["mean_y"][0, 1] > 0  # denormals are kept
    assert np.isnan(got["mean_y"]).any() and np.isinf(got["m2"]).any() and (got["n"] >= 2).any()
    assert not got["reserved"].any()


def test_s1_is_the_identity_on_mean_and_n(rt4, tracer, renders):
    fine = np.ascontiguousarray(renders["tiger", 2][:H, :W])
    got = check(rt4, tracer, fine, 1)
    assert raw(got["mean"]) == raw(fine["mean"]) and raw(got["mean_y"]) == raw(fine["mean_y"]) and raw(got["n"]) == raw(fine["n"])


@pytest.mark.parametrize("s", SS)
def test_device_entry_on_a_stream(rt4, tracer, s):
    """Tracer.light_downsample_device on torch buffers and a torch stream equals the host entry byte for byte (no NaN in
    the input: a NaN's payload is not defined)."""
    import torch

    rng = np.random.default_rng(40 + s)
    fine_img = np.zeros((H * s, W * s), rt4.LIGHT_DTYPE)
    fine_img["mean"] = rng.random((H * s, W * s, 3)).astype(np.float32)
    fine_img["mean_y"] = light_ref.luminance(fine_img["mean"])
    fine_img["m2"] = rng.random((H * s, W * s)).astype(np.float32)
    fine_img["n"] = rng.choice(np.array([0, 1, 2, 9, INT32_MAX], np.int32), (H * s, W * s), p=[0.02, 0.02, 0.3, 0.36, 0.3])
    fine, out = padded(rt4, fine_img, seed=3), poison(rt4, (H, W + PAD), seed=4)
    want = tracer.light_downsample_host(fine, s, out=out.copy(), w=W, h=H)
    d_fine = torch.from_numpy(fine.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.from_numpy(out.view(np.uint8).reshape(-1).copy()).cuda()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tracer.light_downsample_device(d_fine.data_ptr(), W * s + PAD, d_out.data_ptr(), W + PAD, W, H, s,
                                       stream=stream.cuda_stream)
    stream.synchronize()
    assert d_out.cpu().numpy().tobytes() == raw(want)
    assert d_fine.cpu().numpy().tobytes() == raw(fine)


def test_argument_errors_leave_the_output_untouched(rt4, tracer):
    import torch

    lib, h = rt4.lib, tracer._h
    err = ctypes.create_string_buffer(512)
    s = 2
    fs, os_ = W * s + PAD, W + PAD
    fine, out = poison(rt4, (H * s, fs), seed=5), poison(rt4, (H, os_), seed=6)
    before, fine_before = raw(out), raw(fine)
    pf, po = ctypes.c_void_p(fine.ctypes.data), ctypes.c_void_p(out.ctypes.data)
    inside = ctypes.c_void_p(fine.ctypes.data + 5 * 32)  # an output inside the input
    big = rt4.SUPERSAMPLE_MAX + 1
    host_cases = {
        "NULL ctx": (None, pf, fs, po, os_, W, H, s), "NULL fine": (h, None, fs, po, os_, W, H, s),
        "NULL out": (h, pf, fs, None, os_, W, H, s), "s 0": (h, pf, fs, po, os_, W, H, 0), "s 9": (h, pf, fs, po, os_, W, H, big),
        "s -1": (h, pf, fs, po, os_, W, H, -1), "w 0": (h, pf, fs, po, os_, 0, H, s), "h 0": (h, pf, fs, po, os_, W, 0, s),
        "w -1": (h, pf, fs, po, os_, -1, H, s), "w 65536": (h, pf, 65536, po, 65536, 65536, 1, 1),
        "h 65536": (h, pf, 1, po, 1, 1, 65536, 1), "w*s 65536": (h, pf, 65536, po, 32768, 32768, 1, 2),
        "h*s 65536": (h, pf, 8, po, 1, 1, 8192, 8), "fine stride": (h, pf, W * s - 1, po, os_, W, H, s),
        "out stride": (h, pf, fs, po, W - 1, W, H, s), "out is the input": (h, pf, fs, pf, os_, W, H, s),
        "out inside the input": (h, pf, fs, inside, os_, W, H, s),
    }
    for name, args in host_cases.items():
        assert lib.rt4_light_downsample_host(*args, err, len(err)) == ERR_ARG and err.value, name
        assert raw(out) == before and raw(fine) == fine_before, name
    # the same through the device entry, and what only it checks: pointers aligned to 16 B
    d_fine = torch.from_numpy(fine.view(np.uint8).reshape(-1).copy()).cuda()
    d_out = torch.from_numpy(out.view(np.uint8).reshape(-1).copy()).cuda()
    df, do = d_fine.data_ptr(), d_out.data_ptr()
    device_cases = {
        "out + 8": (h, df, fs, do + 8, os_ - 1, W, H, s), "fine + 8": (h, df + 8, fs - 1, do, os_, W, H, s),
        "fine + 4": (h, df + 4, fs - 1, do, os_, W, H, s), "s 9": (h, df, fs, do, os_, W, H, big),
        "w*s 65536": (h, df, 65536, do, 32768, 32768, 1, 2), "fine stride": (h, df, W * s - 1, do, os_, W, H, s),
        "out stride": (h, df, fs, do, W - 1, W, H, s), "out inside the input": (h, df, fs, df + 64, os_, W, H, s),
        "NULL out": (h, df, fs, None, os_, W, H, s), "NULL fine": (h, None, fs, do, os_, W, H, s),
    }
    for name, args in device_cases.items():
        args = tuple(ctypes.c_void_p(a) if i in (1, 3) and a is not None else a for i, a in enumerate(args))
        assert lib.rt4_light_downsample_device(*args, None, err, len(err)) == ERR_ARG and err.value, name
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == before and d_fine.cpu().numpy().tobytes() == fine_before
    with pytest.raises(rt4.RT4Error) as ei:
        tracer.light_downsample_host(fine, 0, out=out, w=W, h=H)
    assert ei.value.status == ERR_ARG and raw(out) == before


def test_cpp_host_supersample(rt4, tracer, tmp_path):
    """rt4_render -s sphere -W 16 -H 8 -n 4 --light --supersample 2 --raw: the image's bytes are the Python pipeline's,
    upscale_uniforms, render_light_host at 32 x 16, the downsample, the resolve; so are the accumulator's."""
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    exe, props_path = os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")
    w, h, s, frames, seed = 16, 8, 2, 4, 12345  # the program's default seed
    pre = str(tmp_path / "ss")
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", str(w), "-H", str(h), "-n", str(frames), "--light",
                        "--supersample", str(s), "--raw", "-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, w, h)
    fine_base = rt4.upscale_uniforms(base, s)
    cam = rt4.Camera(props)
    us = [cam.frame_uniforms(fine_base, rt4.SECTION_YXZ, seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) for n in range(1, frames + 1)]
    tracer.set_scene(rt4.Scene.builtin("sphere"))
    fine, _ = tracer.render_light_host(us, rt4.region(w * s, h * s))
    acc = tracer.light_downsample_host(fine, s)
    image = tracer.light_resolve_host(acc, base.light_to_color_conversion_coefficient)
    assert open(pre + "_yxz.raw", "rb").read() == raw(image)
    assert open(pre + "_yxz_light.raw", "rb").read() == raw(acc)
    assert f"wrote {pre}_yxz.ppm ({w} x {h})" in r.stdout and f"noise yxz: pixels {w * h}," in r.stdout
    # and it is not the image of the same frames at the output resolution
    r1 = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", str(w), "-H", str(h), "-n", str(frames), "--light", "--raw",
                         "-o", str(tmp_path / "plain")], capture_output=True, text=True, timeout=120)
    assert r1.returncode == 0, r1.stderr
    assert open(str(tmp_path / "plain_yxz.raw"), "rb").read() != raw(image)


def test_cpp_host_supersample_resume_and_adaptive(rt4, tmp_path):
    """--light-checkpoint saves the fine accumulator: 2 frames, then 2 more with --light-resume, leave the bytes of 4
    unbroken frames; a checkpoint is refused at another S; --adaptive runs at the fine resolution and its _n picture
    is the output's size."""
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    exe, props_path = os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")
    common = [exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8", "--light", "--raw"]
    ck = str(tmp_path / "c.rt4l")

    def run(args):
        return subprocess.run(common + args, capture_output=True, text=True, timeout=120)

    whole = run(["--supersample", "2", "-n", "4", "-o", str(tmp_path / "whole")])
    first = run(["--supersample", "2", "-n", "2", "--light-checkpoint", ck, "-o", str(tmp_path / "first")])
    assert whole.returncode == 0 and first.returncode == 0, (whole.stderr, first.stderr)
    info = rt4.light_info(ck)
    assert (info["w"], info["h"], info["frames_issued"]) == (32, 16, 2)
    second = run(["--supersample", "2", "-n", "2", "--light-resume", ck, "-o", str(tmp_path / "second")])
    assert second.returncode == 0, second.stderr
    for suffix in ("_yxz.raw", "_yxz_light.raw"):
        assert open(str(tmp_path / "second") + suffix, "rb").read() == open(str(tmp_path / "whole") + suffix, "rb").read(), suffix
    other = run(["--supersample", "4", "-n", "2", "--light-resume", ck, "-o", str(tmp_path / "other")])
    assert other.returncode == 1 and other.stderr == "rt4_render: --light-resume: the checkpoint holds a 32x16 accumulator, not 64x32\n"
    ad = run(["--supersample", "2", "-n", "12", "--adaptive", "--png", "-o", str(tmp_path / "ad")])
    assert ad.returncode == 0, ad.stderr
    assert "adaptive yxz: warmup tiles 8 frames 8" in ad.stdout  # 32 x 16 fine pixels: 4 x 2 tiles
    assert f"wrote {tmp_path / 'ad'}_yxz_n.png (16 x 8, frames per pixel)" in ad.stdout
