"""What the upscale definition of rt4.h does, on the CPU: the numpy restatement (upscale_ref.upscale) on G-buffers made
from numpy rays through the oracle's find_intersection and on cell images the oracle rendered (24 x 16 cells, 4 spp,
4 bounces, 48 progressive frames, seed 4242), against a window-resolution image of 48 frames (seed 777). No GPU: the
HIP kernel is held to this definition bit for bit in test_gpu_upscale.py.

The bounds are conditions on the definition, set with margin over a float64 prototype, not
measurements of this restatement: guided MSE <= 0.6 x the MSE of the reference's block stretch and below plain bilinear
interpolation, at most 2 % of the pixels without a counted tap, and on edge pixels (window pixels whose surface is not
their own cell's) guided <= 0.5 x nearest."""
import numpy as np
import pytest

import denoise_ref
import upscale_ref

CW, CH = 24, 16
FRAMES = 48
BOUNDED = ["sphere", "tiger", "cylinder4d", "hypercube"]
PRINTED = ["room", "all_primitives"]
SCALES = [4, 7]


def progressive(rt4, oracle, desc, w, h, seed):
    base = rt4.make_uniforms(w, h, samples=4, reflections=4, seed=seed)
    frame = np.zeros((h, w, 4), np.float32)
    for n in range(1, FRAMES + 1):
        oracle.render_fmt(desc, rt4.progressive_uniforms(base, n), rt4.region(w, h), rt4.FRAME_RGBA32F, frame=frame)
    frame.setflags(write=False)
    return frame


class SceneData:
    """Everything the tests need of one scene, made on first use and kept: G-buffers by scale (1 = the cells), the cell
    image and the window-resolution images by scale."""

    def __init__(self, rt4, oracle, name):
        self.rt4, self.oracle, self.name = rt4, oracle, name
        self.scene = rt4.Scene.named(name)
        self.marked = rt4.SceneDesc.from_buffer_copy(self.scene.to_bytes())
        self.table = denoise_ref.unique_colors(rt4, self.marked)
        self.u = rt4.make_uniforms(CW, CH, samples=4, reflections=4)
        self._g, self._truth, self._cells = {}, {}, None

    def gbuffer(self, s):
        if s not in self._g:
            rt4 = self.rt4
            u = rt4.upscale_uniforms(self.u, s)
            g, hit, col = denoise_ref.gbuffer_reference(rt4, self.oracle, self.marked, u, rt4.region(CW * s, CH * s))
            g["surface"] = denoise_ref.surfaces_from_colors(self.table, hit, col)
            g.setflags(write=False)
            self._g[s] = g
        return self._g[s]

    def cells(self):
        if self._cells is None:
            self._cells = progressive(self.rt4, self.oracle, self.scene.desc, CW, CH, 4242)
        return self._cells

    def truth(self, s):
        if s not in self._truth:
            self._truth[s] = progressive(self.rt4, self.oracle, self.scene.desc, CW * s, CH * s, 777)
        return self._truth[s]


@pytest.fixture(scope="module")
def data(rt4, oracle):
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = SceneData(rt4, oracle, name)
        return cache[name]

    return get


@pytest.fixture(scope="module")
def measured(data):
    """{(scene, scale): dict(nearest, guided, bilinear: MSE over all pixels; edge_nearest, edge_guided, edges;
    no_tap: the share of pixels with no counted tap)}."""
    cache = {}

    def get(name, s):
        if (name, s) not in cache:
            d = data(name)
            cells, truth = d.cells(), d.truth(s)[..., :3].astype(np.float64)
            guided, det = upscale_ref.upscale(d.u, s, cells, d.gbuffer(1), d.gbuffer(s), details=True)
            near = upscale_ref.nearest(cells, s)
            bil = upscale_ref.bilinear(d.u, s, cells)
            err = {k: ((v[..., :3].astype(np.float64) - truth) ** 2).mean(axis=2) for k, v in
                   (("nearest", near), ("guided", guided), ("bilinear", bil))}
            edge = d.gbuffer(s)["surface"] != upscale_ref.nearest(d.gbuffer(1)["surface"], s)
            m = {k: v.mean() for k, v in err.items()}
            m.update(edges=int(edge.sum()), no_tap=float((~det["kept"]).mean()),
                     edge_nearest=err["nearest"][edge].mean() if edge.any() else np.nan,
                     edge_guided=err["guided"][edge].mean() if edge.any() else np.nan)
            print(f"{name} scale {s}: guided/nearest {m['guided'] / m['nearest']:.3f}, bilinear/nearest "
                  f"{m['bilinear'] / m['nearest']:.3f}, no counted tap {m['no_tap']:.4f}, edge pixels {m['edges']}, "
                  f"guided/nearest there {m['edge_guided'] / m['edge_nearest']:.3f}")
            cache[(name, s)] = m
        return cache[(name, s)]

    return get


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", BOUNDED)
def test_guided_beats_the_stretch_and_bilinear(measured, name, s):
    m = measured(name, s)
    assert m["guided"] <= 0.6 * m["nearest"]
    assert m["guided"] < m["bilinear"]
    assert m["no_tap"] <= 0.02


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ["sphere", "hypercube"])
def test_edge_pixels(measured, name, s):
    m = measured(name, s)
    assert m["edges"] > 0
    assert m["edge_guided"] <= 0.5 * m["edge_nearest"]


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", PRINTED)
def test_scenes_reported_without_a_bound(measured, name, s):
    m = measured(name, s)  # printed above
    assert np.isfinite(m["guided"]) and np.isfinite(m["nearest"]) and 0.0 <= m["no_tap"] <= 1.0


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8], ids=["f32", "f16", "rgba8"])
def test_nearest_is_repeat(rt4, dtype):
    rng = np.random.default_rng(3)
    cells = rng.integers(0, 256, (5, 7, 4)).astype(np.uint8) if dtype == np.uint8 else (rng.random((5, 7, 4)) * 1.5).astype(dtype)
    u = rt4.make_uniforms(7, 5, samples=1, reflections=1)
    for s in (1, 3, 10):
        out = upscale_ref.upscale(u, s, cells, mode=upscale_ref.NEAREST)
        assert out.dtype == cells.dtype and out.shape == (5 * s, 7 * s, 4)
        assert out.tobytes() == np.repeat(np.repeat(cells, s, axis=0), s, axis=1).tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float16, np.uint8], ids=["f32", "f16", "rgba8"])
def test_scale_1_returns_the_colour(data, dtype):
    """At scale 1 with G_win == G_cells every pixel's own tap has k = 1 (ax = ay = 0): the colour comes back through
    the store rule, with alpha 1; only a hit with a non-finite depth has no tap and keeps its stored bits."""
    d = data("sphere")
    g = d.gbuffer(1)
    rng = np.random.default_rng(4)
    cells = rng.integers(0, 256, (CH, CW, 4)).astype(np.uint8) if dtype == np.uint8 else (rng.random((CH, CW, 4)) * 1.5).astype(dtype)
    out, det = upscale_ref.upscale(d.u, 1, cells, g, g, details=True)
    assert (det["counted"] == 1).all() and (det["candidates"] == 1).all() and det["kept"].all()
    want = cells.copy()
    want[..., :3] = denoise_ref.encode(denoise_ref.decode(cells)[..., :3], dtype)
    want[..., 3] = 255 if dtype == np.uint8 else 1
    assert out.tobytes() == want.tobytes()


@pytest.mark.parametrize("s", [3, 7])
@pytest.mark.parametrize("name", ["sphere", "tiger", "all_primitives", "hypercube"])
def test_window_gbuffer_at_cell_centres_names_the_cell(data, name, s):
    """For odd scales the centre pixel of a cell looks along the cell's own primary ray: the two G-buffers describe the
    same camera."""
    d = data(name)
    gc, gw = d.gbuffer(1), d.gbuffer(s)[s // 2::s, s // 2::s]
    assert gw.shape == gc.shape
    share = (gw["surface"] == gc["surface"]).mean()
    hits = (gc["surface"] >= 0) & (gw["surface"] == gc["surface"])
    with np.errstate(invalid="ignore"):
        rel = np.abs(gw["depth"][hits].astype(np.float64) / gc["depth"][hits] - 1).max()
    print(f"{name} scale {s}: cell centres with the cell's surface {share:.4f}, largest relative depth difference {rel:.2e}")
    assert share >= 0.99


def test_weights_against_float64():
    """For every scale and every x % s (three cells, so the first column's x0 = -1 and interior columns both occur):
    x0 and ax are floor and frac of the float64 (x + 0.5)/s - 0.5, ax as the float32 nearest to that frac."""
    for s in range(1, 65):
        x0, ax = upscale_ref.tap_positions(3, s)
        f = (np.arange(3 * s) + 0.5) / s - 0.5
        assert np.array_equal(x0, np.floor(f).astype(np.int64)), s
        assert np.array_equal(ax, (f - np.floor(f)).astype(np.float32)), s
        assert ((ax >= 0) & (ax < 1)).all()


def test_upscale_uniforms_changes_the_resolution_only(rt4):
    u = rt4.make_uniforms(121, 75, samples=3, reflections=5, seed=99, fi=10.0, te=5.0, part=0.25)
    for s in (1, 7, 64):
        w = rt4.upscale_uniforms(u, s)
        assert list(w.resolution) == [121.0 * s, 75.0 * s]
        wb, ub = bytearray(bytes(w)), bytearray(bytes(u))
        off = rt4.Uniforms.resolution.offset
        size = rt4.Uniforms.resolution.size
        wb[off:off + size] = ub[off:off + size]
        assert wb == ub
        ref = upscale_ref.window_uniforms(u, s)
        assert [float(v) for v in ref.resolution] == list(w.resolution)
    for bad in (0, -1, 65):
        with pytest.raises(rt4.RT4Error):
            rt4.upscale_uniforms(u, bad)
    with pytest.raises(rt4.RT4Error):
        rt4.upscale_uniforms(rt4.make_uniforms(1024, 16, 1, 1), 64)  # 65536 wide
    with pytest.raises(rt4.RT4Error):
        rt4.upscale_uniforms(rt4.make_uniforms(16, 256, 1, 1), 64)  # 16384 tall
    assert list(rt4.upscale_uniforms(rt4.make_uniforms(1023, 255, 1, 1), 64).resolution) == [65472.0, 16320.0]
