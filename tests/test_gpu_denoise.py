"""The HIP edge-stopping filter (rt4.h rt4_denoise_device) against its definition restated in numpy
(denoise_ref.atrous), bit for bit: rendered frames in every format and at every level count, degenerate sizes with
padded strides, a synthetic G-buffer with the awkward values, the parameter edges, the argument errors and the
--denoise switch of the host program."""
import os
import subprocess

import numpy as np
import pytest

import denoise_ref

pytestmark = pytest.mark.gpu

W, H = 61, 37
DT = {0: np.float32, 1: np.float16, 2: np.uint8}
ERR_ARG = -1


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def params_kw(p):
    return dict(levels=p.levels, cos_min=p.cos_min, depth_tol=p.depth_tol, max_refl_prob=p.max_refl_prob)


def synthetic_gbuffer(rt4, h, w, seed):
    """A G-buffer no renderer made: surface ids in blocks and stripes, misses, NaN and +inf depths, zero normals and
    refl_prob on both sides of the default threshold 0.5."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    g = np.zeros((h, w), rt4.GBUFFER_DTYPE)
    sid = (xs // 5 + 3 * (ys // 4)) % 5  # blocks
    sid[:, w // 2:] = np.where(ys[:, w // 2:] % 3 == 0, 5 + xs[:, w // 2:] % 2, sid[:, w // 2:])  # stripes one pixel wide
    sid[rng.random((h, w)) < 0.08] = -1
    base = rng.normal(size=(8, 4))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    n = base[np.maximum(sid, 0)] + rng.normal(0, 0.15, (h, w, 4))  # some pairs fall under cos_min = 0.9
    n /= np.linalg.norm(n, axis=2, keepdims=True)
    n[rng.random((h, w)) < 0.05] = 0.0  # zero normals: every dot is 0
    z = 3.0 + 0.2 * np.maximum(sid, 0) + rng.normal(0, 0.2, (h, w))  # some pairs fall outside depth_tol = 0.1
    z[rng.random((h, w)) < 0.04] = np.nan
    z[rng.random((h, w)) < 0.04] = np.inf
    g["normal"] = np.where((sid >= 0)[..., None], n, 0).astype(np.float32)
    g["depth"] = np.where(sid >= 0, z, np.inf).astype(np.float32)
    g["surface"] = sid
    g["refl_prob"] = np.where(sid >= 0, rng.choice(np.array([0.0, 0.3, 0.5, 0.50000006, 0.7], np.float32), (h, w)), 0)
    g["glow"] = 0.0
    return g


def synthetic_frame(h, w, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    return (rng.random((h, w, 4)) * 1.5).astype(DT[fmt])  # alpha is not 1: it must come out as stored


def check(tracer, frame, g, p, what):
    got = tracer.denoise_host(frame, g, p)
    want = denoise_ref.atrous(frame, g, **params_kw(p))
    assert got.dtype == frame.dtype and raw(got) == raw(want), what
    return got


# ------------------------------------------------------------------------------------------ 5. rendered input
@pytest.fixture(scope="module")
def rendered(rt4, tracer_lut):
    """{(scene, format): (frame as rendered on the GPU, its G-buffer)} at 61 x 37, 4 spp; rendered once."""
    out = {}
    u = rt4.make_uniforms(W, H, samples=4, reflections=4, seed=12345)
    reg = rt4.region(W, H)
    for name in ("sphere", "all_primitives"):
        tracer_lut.set_scene(rt4.Scene.named(name))
        g = tracer_lut.render_gbuffer_host(u, reg)
        for fmt in (0, 1, 2):
            frame = np.zeros((H, W, 4), DT[fmt])
            tracer_lut.render_host_ex(u, reg, frame, fmt)
            frame.setflags(write=False)
            out[name, fmt] = (frame, g)
        g.setflags(write=False)
    return out


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["f32", "f16", "rgba8"])
@pytest.mark.parametrize("name", ["sphere", "all_primitives"])
def test_rendered_input_every_level(rt4, tracer_lut, rendered, name, fmt):
    frame, g = rendered[name, fmt]
    filt = denoise_ref.filterable(g, 0.5)
    assert filt.any() and (~filt).any()  # sphere: misses; all_primitives: reflective pixels pass through
    if name == "all_primitives":
        assert ((g["surface"] >= 0) & ~filt).any()
    for levels in range(1, rt4.DENOISE_MAX_LEVELS + 1):  # level 5: stride 32, most taps outside the image
        got = check(tracer_lut, frame, g, rt4.denoise_params(levels=levels), (name, fmt, levels))
        assert raw(got[~filt]) == raw(frame[~filt])
    assert raw(got) != raw(frame)  # and the filter did something
    assert tracer_lut.denoise_bytes() >= W * H * 56


# ------------------------------------------------------------------------------------------ 6. degenerate sizes
@pytest.mark.parametrize("w, h", [(1, 1), (5, 3), (8, 8), (64, 1)])
def test_degenerate_sizes_and_strides(rt4, tracer_lut, w, h):
    for fmt in (0, 1, 2):
        g = synthetic_gbuffer(rt4, h, w, 100 + w)
        g["refl_prob"] = 0.0
        g["surface"] = np.maximum(g["surface"], 0) % 2  # mostly filterable, two surfaces
        frame = synthetic_frame(h, w, fmt, 200 + w)
        for levels in (1, 3, 6):
            p = rt4.denoise_params(levels=levels, cos_min=-2.0, depth_tol=1e9)  # only NaN / inf depths stop a tap
            want = denoise_ref.atrous(frame, g, **params_kw(p))
            # input, output and G-buffer rows padded, each by another amount; the output's padding keeps its bytes
            fin = synthetic_frame(h, w + 3, fmt, 1)
            fin[:, :w] = frame
            gin = synthetic_gbuffer(rt4, h, w + 2, 2)
            gin[:, :w] = g
            out = synthetic_frame(h, w + 5, fmt, 3)
            before = out.copy()
            tracer_lut.denoise_host(fin, gin, p, out=out, w=w)
            assert raw(out[:, :w]) == raw(want), (w, h, fmt, levels)
            assert raw(out[:, w:]) == raw(before[:, w:])


# ------------------------------------------------------------------------------------------ 7. synthetic G-buffer
@pytest.mark.parametrize("fmt", [0, 1, 2], ids=["f32", "f16", "rgba8"])
def test_synthetic_gbuffer(rt4, tracer_lut, fmt):
    g = synthetic_gbuffer(rt4, 17, 33, 7)
    frame = synthetic_frame(17, 33, fmt, 8)
    filt = denoise_ref.filterable(g, 0.5)
    hitp = g["surface"] >= 0
    assert (np.isnan(g["depth"]) & filt).any() and (np.isposinf(g["depth"]) & filt).any()
    assert ((g["normal"] == 0).all(axis=2) & filt).any() and (hitp & ~filt).any() and (~hitp).any()
    for levels in (1, 2, 3, 4):
        got = check(tracer_lut, frame, g, rt4.denoise_params(levels=levels), (fmt, levels))
    assert raw(got[..., 3]) == raw(frame[..., 3])  # alpha as stored
    assert raw(got[~filt]) == raw(frame[~filt])


# ------------------------------------------------------------------------------------------ 8. parameter edges
def test_parameter_edges(rt4, tracer_lut, rendered):
    frame, g = rendered["all_primitives", 0]
    got = check(tracer_lut, frame, g, rt4.denoise_params(max_refl_prob=-1.0), "max_refl_prob -1")
    assert raw(got) == raw(frame)  # nothing is filterable: the stored bits
    check(tracer_lut, frame, g, rt4.denoise_params(cos_min=1.0), "cos_min 1")
    check(tracer_lut, frame, g, rt4.denoise_params(depth_tol=0.0), "depth_tol 0")
    gs, fs = synthetic_gbuffer(rt4, 17, 33, 9), synthetic_frame(17, 33, 1, 10)
    check(tracer_lut, fs, gs, rt4.denoise_params(max_refl_prob=-1.0), "synthetic max_refl_prob -1")
    check(tracer_lut, fs, gs, rt4.denoise_params(cos_min=1.0, levels=2), "synthetic cos_min 1")
    check(tracer_lut, fs, gs, rt4.denoise_params(depth_tol=0.0, levels=2), "synthetic depth_tol 0")


# ------------------------------------------------------------------------------------------ 9. errors
def test_argument_errors_write_nothing(rt4, tracer_lut):
    import torch

    w, h = 16, 8
    buf = torch.full((2 * h, w, 4), 0.25, dtype=torch.float32, device="cuda")  # input rows 0..7, output rows 8..15
    gbuf = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    d_in, d_out = buf.data_ptr(), buf.data_ptr() + h * w * 16

    def status(*args, **kw):
        try:
            tracer_lut.denoise_device(*args, **kw)
        except rt4.RT4Error as e:
            return e.status
        return 0

    ok = rt4.denoise_params()
    assert status(d_in, w, d_in, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG  # the same buffer
    assert status(d_in, w, d_in + (h - 1) * w * 16, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG  # one row shared
    assert status(d_in, w, d_out - 16, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG  # one pixel shared
    for levels in (0, 7):
        assert status(d_in, w, d_out, w, 0, w, h, gbuf.data_ptr(), w, rt4.denoise_params(levels=levels), stream) == ERR_ARG
    assert status(d_in, w, d_out, w, 0, w, h, 0, w, ok, stream) == ERR_ARG  # null G-buffer
    assert status(0, w, d_out, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG
    assert status(d_in, w, 0, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG
    assert status(d_in, w, d_out, w, 9, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG  # unknown format
    assert status(d_in, w - 1, d_out, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == ERR_ARG  # stride below the width
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)
    # adjacent, not overlapping: accepted, and the input half keeps its bytes (the zeroed G-buffer is surface 0
    # everywhere: filterable)
    assert status(d_in, w, d_out, w, 0, w, h, gbuf.data_ptr(), w, ok, stream) == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:h]) == raw(before[:h])


# ------------------------------------------------------------------------------------------ 10. rt4_render --denoise
def test_cpp_host_denoise(rt4, tracer_lut, tmp_path):
    """lib/rt4_render -n 2 --denoise 3 on the sphere scene at 64 x 40: the _dn PPM equals the same loop driven from
    Python (two progressive frames, the G-buffer of the pose, the filter, write_ppm) byte for byte, and the plain PPM
    equals the one of a run without --denoise."""
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    exe = os.path.join(lib_dir, "rt4_render")
    props_path = os.path.join(lib_dir, "..", "..", "properties.txt")
    w, h, seed = 64, 40, 12345
    files = {}
    for tag, extra in (("dn", ["--denoise", "3"]), ("plain", [])):
        pre = str(tmp_path / tag)
        r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-n", "2", "-W", str(w), "-H", str(h), "--seed", str(seed),
                            "-o", pre] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        files[tag] = open(pre + "_yxz.ppm", "rb").read()
    assert files["dn"] == files["plain"]
    assert not os.path.exists(str(tmp_path / "plain") + "_yxz_dn.ppm")
    # the same loop from Python
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, w, h)
    cam = rt4.Camera(props)
    us = [cam.frame_uniforms(base, rt4.SECTION_YXZ, seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)) for n in (1, 2)]
    scene = rt4.Scene.builtin("sphere")
    tracer_lut.set_scene(scene)
    reg = rt4.region(w, h)
    frame = np.zeros((h, w, 4), np.float32)
    for u in us:
        tracer_lut.render_host(u, reg, frame)
    g = tracer_lut.render_gbuffer_host(us[-1], reg)
    dn = tracer_lut.denoise_host(frame, g, rt4.denoise_params(levels=3))
    rt4.write_ppm(str(tmp_path / "py_dn.ppm"), dn)
    rt4.write_ppm(str(tmp_path / "py.ppm"), frame)
    assert open(str(tmp_path / "py.ppm"), "rb").read() == files["plain"]
    assert open(str(tmp_path / "py_dn.ppm"), "rb").read() == open(str(tmp_path / "dn") + "_yxz_dn.ppm", "rb").read()
    assert raw(dn) == raw(denoise_ref.atrous(frame, g, levels=3))
    # refused together with --gpus
    r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8", "--gpus", "2", "--denoise"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--denoise" in r.stderr


def test_cpp_host_denoise_three_sections(rt4, tracer_lut, tmp_path):
    """rt4_render -3 --denoise 2: every section's image gets its own G-buffer and its own filtered image, each equal
    to the same steps from Python (properties.txt sizes: 121 x 75 and twice 60 x 37)."""
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    exe = os.path.join(lib_dir, "rt4_render")
    props_path = os.path.join(lib_dir, "..", "..", "properties.txt")
    pre, seed = str(tmp_path / "s"), 99
    r = subprocess.run([exe, "-p", props_path, "-s", "tiger", "-n", "1", "-3", "--seed", str(seed), "--denoise", "2", "-o", pre],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    tracer_lut.set_scene(rt4.Scene.builtin("tiger"))
    sections = [(rt4.SECTION_YXZ, "yxz", "main"), (rt4.SECTION_YWZ, "ywz", "additional"), (rt4.SECTION_YXW, "yxw", "additional")]
    for sec, tag, window in sections:
        w, h = rt4.window_cells(props, window)
        u = rt4.Camera(props).frame_uniforms(rt4.uniforms_from_properties(props, w, h, sec), sec, seed ^ 0x9E3779B9)
        frame = np.zeros((h, w, 4), np.float32)
        tracer_lut.render_host(u, rt4.region(w, h), frame)
        g = tracer_lut.render_gbuffer_host(u, rt4.region(w, h))
        dn = tracer_lut.denoise_host(frame, g, rt4.denoise_params(levels=2))
        for arr, suffix in ((frame, ""), (dn, "_dn")):
            path = str(tmp_path / f"py_{tag}{suffix}.ppm")
            rt4.write_ppm(path, arr)
            assert open(path, "rb").read() == open(f"{pre}_{tag}{suffix}.ppm", "rb").read(), (tag, suffix)
