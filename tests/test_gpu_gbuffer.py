"""The primary-hit G-buffer (rt4.h rt4_render_gbuffer_device) on the MI355X against the numpy primary rays of
denoise_ref plus the oracle's find_intersection: every pixel, bit for bit, on the specialised kernels and on the generic
one; regions, picking, and that a G-buffer launch leaves the renders around it alone."""
import numpy as np
import pytest

import denoise_ref
import scene_builder

pytestmark = pytest.mark.gpu

W, H = 61, 37  # ragged 8x8 tiles in both directions
SCENES = ["sphere", "room", "tiger", "cylinder4d", "hypercube", "all_primitives", "tiger_two_mirrors", "composed"]
COMPOSED = "kind_twice"  # scene_builder: spheres, spaces, spheres again: no specialised kernel takes that group list
CAMERAS = ["default", "rotated", "ywz"]
MISS = (0.0, 0.0, 0.0, 0.0, np.inf, -1, 0.0, 0.0)


def uniforms(rt4, camera, w=W, h=H, name=None):
    kw = dict(samples=4, reflections=4, seed=12345)
    if name == "composed":
        kw["focus"] = scene_builder.case_focus(COMPOSED)
    if camera == "rotated":
        kw.update(fi=20.0, te=-10.0, psi=15.0)  # degrees (properties.txt units), all three non-zero
    if camera == "ywz":
        kw.update(section=rt4.SECTION_YWZ)
    return rt4.make_uniforms(w, h, **kw)


_marked = {}


def marked_scene(rt4, name):
    """(Scene whose every surface has a colour of its own, {colour: surface}); the kernel shape is the original's."""
    if name not in _marked:
        if name == "composed":
            d = scene_builder.build_case(rt4, COMPOSED)
        else:
            d = rt4.SceneDesc.from_buffer_copy(rt4.Scene.named(name).to_bytes())
        table = denoise_ref.unique_colors(rt4, d)
        _marked[name] = (rt4.Scene(d), table)
    return _marked[name]


_reference = {}


def reference(rt4, oracle, name, camera):
    """The expected G-buffer of (scene, camera), computed once and shared; never modified."""
    key = (name, camera)
    if key not in _reference:
        scene, table = marked_scene(rt4, name)
        g, hit, col = denoise_ref.gbuffer_reference(rt4, oracle, scene.desc, uniforms(rt4, camera, name=name), rt4.region(W, H))
        g["surface"] = denoise_ref.surfaces_from_colors(table, hit, col)
        g.setflags(write=False)
        _reference[key] = (g, hit, col)
    return _reference[key]


@pytest.fixture(scope="module")
def tracer_generic(rt4):
    t = rt4.Tracer(device=0, flags=rt4.FLAG_GENERIC_KERNEL)
    yield t
    t.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_floats(a, b):
    """The same bit patterns (the +inf distances of all_primitives' hits included; no view here has a NaN one)."""
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("generic", [False, True], ids=["specialised", "generic"])
@pytest.mark.parametrize("camera", CAMERAS)
@pytest.mark.parametrize("name", SCENES)
def test_gbuffer_parity(rt4, oracle, tracer, tracer_generic, name, camera, generic):
    scene, table = marked_scene(rt4, name)
    want, hit, col = reference(rt4, oracle, name, camera)
    t = tracer_generic if generic else tracer
    t.set_scene(scene)
    if generic or name == "composed":
        assert t.kernel_shape == 0xFFFFFFFF
    else:
        assert t.kernel_shape != 0xFFFFFFFF  # the marking did not change the kernel
    got = t.render_gbuffer_host(uniforms(rt4, camera, name=name), rt4.region(W, H))
    assert got.shape == (H, W)
    assert np.array_equal(got["surface"] >= 0, hit)
    assert 0 < hit.sum()  # the camera sees the scene
    assert same_floats(got["depth"], want["depth"])
    assert same_floats(got["normal"], want["normal"])
    assert np.array_equal(bits(got["glow"]), bits(want["glow"]))
    assert np.array_equal(bits(got["refl_prob"]), bits(want["refl_prob"]))
    assert np.array_equal(got["surface"], want["surface"])
    # the surface names the object the oracle hit: its colour through the public surface query
    n = scene.surface_count()
    assert got["surface"].max() < n
    colors = np.array([scene.surface(s)["color"] for s in range(n)], np.float32)
    assert np.array_equal(bits(colors[got["surface"][hit]]), bits(col[hit]))
    miss = got[~hit]
    for field, v in zip(("depth", "surface", "refl_prob", "glow"), MISS[4:]):
        assert np.array_equal(miss[field], np.full(miss.shape, v, miss[field].dtype)), field
    assert np.array_equal(bits(miss["normal"]), np.zeros((miss.size, 4), np.uint32))  # +0.0 four times


def test_cameras_see_misses_and_several_surfaces(rt4, oracle):
    """The parity cases are not trivial: sky pixels, at least two surfaces in every scene's default view, and hits
    whose distance is not finite (all_primitives: the cylinders' exact test can report them)."""
    for name in SCENES:
        g, hit, _ = reference(rt4, oracle, name, "default")
        assert len(np.unique(g["surface"][hit])) >= 2, name
    for name in ("sphere", "tiger", "cylinder4d", "hypercube", "tiger_two_mirrors", "composed"):
        assert (~reference(rt4, oracle, name, "default")[1]).any(), name
    g, hit, _ = reference(rt4, oracle, "all_primitives", "default")
    assert (~np.isfinite(g["depth"][hit])).any()


@pytest.mark.parametrize("name, generic", [("all_primitives", False), ("all_primitives", True), ("sphere", False)])
def test_gbuffer_regions(rt4, oracle, tracer, tracer_generic, name, generic):
    """A sub-rectangle, a banded region and a padded row stride give the full G-buffer's pixels; padding is untouched."""
    scene, _ = marked_scene(rt4, name)
    t = tracer_generic if generic else tracer
    t.set_scene(scene)
    u = uniforms(rt4, "rotated", name=name)
    full = t.render_gbuffer_host(u, rt4.region(W, H))
    want, _, _ = reference(rt4, oracle, name, "rotated")
    assert np.array_equal(full["surface"], want["surface"]) and same_floats(full["depth"], want["depth"])

    def padded(rows, cols):  # every byte 0xAB
        return np.frombuffer(bytes([0xAB]) * (32 * rows * cols), rt4.GBUFFER_DTYPE).reshape(rows, cols).copy()

    # sub-rectangle, x0 and y0 non-zero, ragged against the 8x8 tiles, row stride larger than w
    reg = rt4.region(29, 19, x0=13, y0=5)
    buf = padded(19, 40)
    t.render_gbuffer_host(u, reg, buf)
    assert buf[:, :29].tobytes() == full[5:24, 13:42].tobytes()
    assert buf[:, 29:].tobytes() == padded(19, 11).tobytes()
    # banded region: local rows 0..7 are image rows 2..9, rows 8..15 are 26..33, 16..18 are 50.. (outside: h = 16)
    reg = rt4.region(W, 16, x0=0, y0=2, band_rows=8, band_step=24)
    buf = padded(16, W + 3)
    t.render_gbuffer_host(u, reg, buf)
    rows = denoise_ref.region_rows(reg)
    assert list(rows[[0, 7, 8, 15]]) == [2, 9, 26, 33]
    assert buf[:, :W].tobytes() == full[rows].tobytes()
    assert buf[:, W:].tobytes() == padded(16, 3).tobytes()


def test_pick(rt4, oracle, tracer):
    scene, _ = marked_scene(rt4, "sphere")
    tracer.set_scene(scene)
    u = uniforms(rt4, "default", name="sphere")
    full = tracer.render_gbuffer_host(u, rt4.region(W, H))
    sky = tuple(int(v) for v in np.argwhere(full["surface"] < 0)[0])  # (y, x) of a sky pixel
    ball = tuple(int(v) for v in np.argwhere(full["surface"] == full["surface"].max())[0])
    cursors = [(0, 0), (W - 1, H - 1), (sky[1], sky[0]), (ball[1], ball[0])]  # two corners, the sky, a sphere
    for x, y in cursors:
        p = tracer.pick(u, x, y)
        assert p["px"].tobytes() == full[y, x].tobytes(), (x, y)
        assert p["hit"] == bool(full["surface"][y, x] >= 0)
        if p["hit"]:
            assert p["object"] == scene.surface(int(full["surface"][y, x]))
        else:
            assert p["object"] is None and np.isposinf(p["px"]["depth"])
    assert not tracer.pick(u, sky[1], sky[0])["hit"]
    assert tracer.pick(u, ball[1], ball[0])["object"]["kind"] == rt4.GROUP_SPHERES


def test_gbuffer_leaves_renders_alone(rt4, tracer_lut):
    """A G-buffer launch between two renders changes neither the frame nor the counter, and the render after it
    equals the one of a run without it. The G-buffer does not depend on seed, samples, part or bounces."""
    import torch

    scene = rt4.Scene.builtin("sphere")
    tracer_lut.set_scene(scene)
    reg = rt4.region(W, H)
    base = rt4.make_uniforms(W, H, samples=4, reflections=4, seed=4242)
    u1, u2 = rt4.progressive_uniforms(base, 1), rt4.progressive_uniforms(base, 2)
    stream = torch.cuda.current_stream().cuda_stream

    def run(with_gbuffer):
        frame = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
        gbuf = torch.zeros((H, W, 8), dtype=torch.float32, device="cuda")
        tracer_lut.render_device_ex(u1, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, cnt.data_ptr(), stream)
        torch.cuda.synchronize()
        mid = (frame.cpu().numpy().copy(), int(cnt.item()))
        if with_gbuffer:
            tracer_lut.render_gbuffer_device(u2, reg, gbuf.data_ptr(), W, stream)
            torch.cuda.synchronize()
            assert np.array_equal(bits(frame.cpu().numpy()), bits(mid[0])) and int(cnt.item()) == mid[1]
        tracer_lut.render_device_ex(u2, reg, frame.data_ptr(), rt4.FRAME_RGBA32F, W, cnt.data_ptr(), stream)
        torch.cuda.synchronize()
        return frame.cpu().numpy(), int(cnt.item()), gbuf.cpu().numpy()

    f0, c0, _ = run(False)
    f1, c1, g1 = run(True)
    assert c0 == c1 > 0 and np.array_equal(bits(f0), bits(f1))
    other = rt4.make_uniforms(W, H, samples=1, reflections=0, seed=1, part=0.25)
    host = tracer_lut.render_gbuffer_host(other, reg)
    assert host.tobytes() == g1.tobytes()
