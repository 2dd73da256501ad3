"""The contract every _host variant shares (rt4.h): a host image with padded rows goes to the device and back whole,
so the padding of every output keeps its bytes, no input changes, and the image itself is, bit for bit, what the same
call computes on unpadded contiguous arrays. Every entry point at 9 x 5 (a partial 8x8 tile in both directions), every
array with a row stride of w + 3 (the window arrays of the upscale 2 w + 3) and 0xA5 in the padding; fp32 frames, and
RGBA8 where the pixel size then differs from the G-buffer's. The tile image and the statistics of light_noise_host
have no stride to pad."""
import numpy as np
import pytest

from test_gpu_light_denoise import random_acc, random_gbuffer

pytestmark = pytest.mark.gpu

W, H, PAD = 9, 5, 3
FILL = 0xA5


def wide(a, w=None, stride=None):
    """a (h, w, ...) in rows of `stride` elements (default w + PAD); every byte of the padding is FILL."""
    w = a.shape[1] if w is None else w
    stride = w + PAD if stride is None else stride
    shape = (a.shape[0], stride) + a.shape[2:]
    out = np.full(int(np.prod(shape)) * a.dtype.itemsize, FILL, np.uint8).view(a.dtype).reshape(shape)
    out[:, :w] = a
    return out


def blank(h, w, tail, dtype, stride=None):
    """An output of FILL bytes throughout: the call has to write all of the image."""
    stride = w + PAD if stride is None else stride
    shape = (h, stride) + tail
    return np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, FILL, np.uint8).view(dtype).reshape(shape)


def row_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).reshape(a.shape[0], -1)


def image_bytes(a, w):
    return row_bytes(a[:, :w]).tobytes()


def padding_kept(a, w):
    return (row_bytes(a[:, w:]) == FILL).all()


class Inputs:
    """The padded inputs of one call and their bytes before it."""

    def __init__(self, **arrays):
        self.arrays = arrays
        self.before = {k: v.tobytes() for k, v in arrays.items()}
        self.__dict__.update(arrays)

    def unchanged(self):
        return all(v.tobytes() == self.before[k] for k, v in self.arrays.items())


def check_outputs(padded, plain, w=W):
    """padded / plain: the outputs of the padded call and of the contiguous one, in the same order."""
    for k, (got, want) in enumerate(zip(padded, plain)):
        assert padding_kept(got, w), k
        assert image_bytes(got, w) == image_bytes(want, w), k


@pytest.fixture(scope="module")
def sphere(rt4, tracer_lut):
    """(uniforms, region, G-buffer, window uniforms, window G-buffer) of the builtin sphere at 9 x 5 and at scale 2;
    read-only."""
    tracer_lut.set_scene(rt4.Scene.builtin("sphere"))
    u = rt4.make_uniforms(W, H, samples=1, reflections=1, seed=1)
    uw = rt4.upscale_uniforms(u, 2)
    g = tracer_lut.render_gbuffer_host(u, rt4.region(W, H))
    gw = tracer_lut.render_gbuffer_host(uw, rt4.region(2 * W, 2 * H))
    for a in (g, gw):
        a.setflags(write=False)
    assert (g["surface"] >= 0).any() and (g["surface"] < 0).any()
    return u, rt4.region(W, H), g, uw, gw


def random_frame(fmt_dtype, h, w, seed):
    rng = np.random.default_rng(seed)
    if np.dtype(fmt_dtype) == np.uint8:
        return rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    return rng.random((h, w, 4)).astype(fmt_dtype)


def test_render_gbuffer_host(rt4, tracer_lut, sphere):
    u, reg, g, _, _ = sphere
    out = blank(H, W, (), rt4.GBUFFER_DTYPE)
    tracer_lut.render_gbuffer_host(u, reg, out)
    check_outputs([out], [g])


@pytest.mark.parametrize("fmt", [0, 2], ids=["f32", "rgba8"])
def test_render_host_ex(rt4, tracer_lut, sphere, fmt):
    """The render blends into the frame it is given: the caller's image goes up first, padded rows and all."""
    u, reg, _, _, _ = sphere
    start = random_frame(rt4.FRAME_NUMPY[fmt], H, W, 11)
    plain = start.copy()
    n_plain = tracer_lut.render_host_ex(u, reg, plain, fmt)
    assert image_bytes(plain, W) != image_bytes(start, W)
    frame = wide(start)
    n = tracer_lut.render_host_ex(u, reg, frame, fmt)
    assert n == n_plain and n > 0
    check_outputs([frame], [plain])


@pytest.mark.parametrize("fmt", [0, 2], ids=["f32", "rgba8"])
def test_denoise_host(rt4, tracer_lut, fmt):
    dt = rt4.FRAME_NUMPY[fmt]
    frame, g = random_frame(dt, H, W, 1), random_gbuffer(rt4, H, W, 2)
    plain = tracer_lut.denoise_host(frame, g, fmt=fmt)
    ins = Inputs(frame=wide(frame), g=wide(g))
    out = blank(H, W, (4,), dt)
    tracer_lut.denoise_host(ins.frame, ins.g, out=out, fmt=fmt, w=W)
    assert ins.unchanged()
    check_outputs([out], [plain])
    assert image_bytes(plain, W) != image_bytes(frame, W)  # the filter did something


def test_reproject_host(rt4, tracer_lut, sphere):
    u, _, g, _, _ = sphere
    rng = np.random.default_rng(3)
    acc, hist = random_frame(np.float32, H, W, 4), rng.integers(0, 6, (H, W)).astype(np.int32)
    p = rt4.reproject_params(max_refl_prob=1.0)  # every hit is eligible: the same pose keeps what has a history
    plain = tracer_lut.reproject_host(u, g, u, g, acc, hist, p)
    assert (plain[1] > 0).any() and (plain[1] == 0).any()  # kept and restarted pixels
    ins = Inputs(gcur=wide(g), gprev=wide(g), acc=wide(acc), hist=wide(hist))
    acc_out, hist_out = blank(H, W, (4,), np.float32), blank(H, W, (), np.int32)
    tracer_lut.reproject_host(u, ins.gcur, u, ins.gprev, ins.acc, ins.hist, p, acc_out=acc_out, hist_out=hist_out, w=W)
    assert ins.unchanged()
    check_outputs([acc_out, hist_out], plain)


def test_upscale_host_guided(rt4, tracer_lut, sphere):
    u, _, g, _, gw = sphere
    cells = random_frame(np.float32, H, W, 5)
    plain = tracer_lut.upscale_host(u, 2, cells, g, gw)
    ins = Inputs(cells=wide(cells), g=wide(g), gw=wide(gw, stride=2 * W + PAD))
    out = blank(2 * H, 2 * W, (4,), np.float32, stride=2 * W + PAD)
    tracer_lut.upscale_host(u, 2, ins.cells, ins.g, ins.gw, out=out, cells_w=W)
    assert ins.unchanged()
    check_outputs([out], [plain], w=2 * W)


@pytest.mark.parametrize("listed", [False, True], ids=["whole", "tile0"])
def test_render_light_host(rt4, tracer_lut, sphere, listed):
    """1 sample, 1 reflection, 2 frames onto a synthetic accumulator; with the tile list [0] the second tile column
    (x >= 8) keeps its state."""
    u, reg, _, _, _ = sphere
    us = [u, rt4.make_uniforms(W, H, samples=1, reflections=1, seed=2)]
    start = random_acc(rt4, H, W, 6)

    def render(light):
        if listed:
            return tracer_lut.render_light_tiles_host(us, reg, [0], light)
        return tracer_lut.render_light_host(us, reg, light)

    plain, n_plain = render(start.copy())
    assert image_bytes(plain, W) != image_bytes(start, W)
    if listed:
        assert image_bytes(plain[:, 8:], 1) == image_bytes(start[:, 8:], 1)
    light = wide(start)
    _, n = render(light)
    assert n == n_plain and n > 0
    check_outputs([light], [plain])


@pytest.mark.parametrize("fmt", [0, 2], ids=["f32", "rgba8"])
def test_light_resolve_host(rt4, tracer_lut, fmt):
    acc = random_acc(rt4, H, W, 7)
    plain = tracer_lut.light_resolve_host(acc, 1.0, fmt)
    ins = Inputs(acc=wide(acc))
    out = blank(H, W, (4,), rt4.FRAME_NUMPY[fmt])
    tracer_lut.light_resolve_host(ins.acc, 1.0, fmt, out=out, w=W)
    assert ins.unchanged()
    check_outputs([out], [plain])


def test_light_noise_host(rt4, tracer_lut):
    acc = random_acc(rt4, H, W, 8)
    se0, q0, tiles0, stats0 = tracer_lut.light_noise_host(acc, 1.0, 0.01)
    ins = Inputs(acc=wide(acc))
    se, q = blank(H, W, (), np.float32), blank(H, W, (), np.float32)
    _, _, tiles, stats = tracer_lut.light_noise_host(ins.acc, 1.0, 0.01, w=W, se=se, q=q)
    assert ins.unchanged()
    check_outputs([se, q], [se0, q0])
    assert tiles.tobytes() == tiles0.tobytes() and stats == stats0 and stats["measured"] > 0


def test_light_denoise_host(rt4, tracer_lut):
    acc, g = random_acc(rt4, H, W, 9), random_gbuffer(rt4, H, W, 10)
    plain = tracer_lut.light_denoise_host(acc, g, 1.0, filtered=True)
    ins = Inputs(acc=wide(acc), g=wide(g))
    out, fl = blank(H, W, (4,), np.float32), blank(H, W, (4,), np.float32)
    tracer_lut.light_denoise_host(ins.acc, ins.g, 1.0, out=out, filtered=fl, w=W)
    assert ins.unchanged()
    check_outputs([out, fl], plain)
