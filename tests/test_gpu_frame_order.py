"""The queue order of a pipelined launch (rt4_render_frames_device): tile-major with the frames inside in the open
kernels without a tiger (sphere, hypercube), frame-major in the others (room, all_primitives). Nothing in the result
may depend on that order, so every case compares the pipelined call bit for bit, image and count, with the same
frames through rt4_render_device_ex (one launch per frame), and one case per scene with the CPU oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DT = {0: np.float32, 1: np.float16, 2: np.uint8}
SPP, BOUNCES = 2, 3


def same_bits(a, b):
    v = {np.dtype(np.float32): np.uint32, np.dtype(np.float16): np.uint16, np.dtype(np.uint8): np.uint8}[a.dtype]
    return np.array_equal(a.view(v), b.view(v))


def gpu_frames(rt4, tracer, us, reg, fmt, pipelined, snapshots=()):
    """The frames `us` into one zeroed frame on `tracer`, in one pipelined call or launch by launch. Returns
    {n: (frame, count)} after n frames for every n of `snapshots` (launch by launch only) and for len(us)."""
    import torch

    tdt = {0: torch.float32, 1: torch.float16, 2: torch.uint8}[fmt]
    fr = torch.zeros((reg.h, reg.w, 4), dtype=tdt, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    out = {}
    if pipelined:
        tracer.render_frames_device(us, reg, fr.data_ptr(), fmt, reg.w, cnt.data_ptr(), s)
    else:
        for n, u in enumerate(us, 1):
            tracer.render_device_ex(u, reg, fr.data_ptr(), fmt, reg.w, cnt.data_ptr(), s)
            if n in snapshots:
                torch.cuda.synchronize()
                out[n] = (fr.cpu().numpy(), int(cnt.item()))
    torch.cuda.synchronize()
    out[len(us)] = (fr.cpu().numpy(), int(cnt.item()))
    return out


def fresh(rt4, scene, us, reg, fmt, pipelined, snapshots=(), reserve=False):
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=scene)
    try:
        if reserve:
            t.reserve_frames(reg.w, reg.h)
        return gpu_frames(rt4, t, us, reg, fmt, pipelined, snapshots)
    finally:
        t.close()


def oracle_frames(oracle, scene, us, reg, fmt):
    c = np.zeros((reg.h, reg.w, 4), DT[fmt])
    n = 0
    for u in us:
        _, k = oracle.render_fmt(scene.desc, u, reg, fmt, frame=c)
        n += k
    return c, n


def classes(oracle, scene, u, reg):
    """(sky pixels, hit pixels) of the region from the oracle's per-pixel find counts: a pixel whose primary ray
    misses makes exactly one find call per sample."""
    _, _, _, counts = oracle.render(scene.desc, u, reg, pixel_counts=True)
    return int((counts == u.samples).sum()), int((counts > u.samples).sum())


FRAME_COUNTS = (2, 3, 7, 64, 65)  # 65: a launch of RT4_MAX_FRAMES (64) and a single frame
SIZES = ((72, 40), (70, 37))
_sequential = {}


def sphere_case(rt4, w, h):
    base = rt4.make_uniforms(w, h, samples=SPP, reflections=BOUNCES, seed=2024)
    return rt4.Scene.named("sphere"), base, rt4.region(w, h)


def sequential_sphere(rt4, w, h):
    """The launch-by-launch frames of the sphere cases, once per size: progressive frame n does not depend on how
    many follow it, so one run of 65 frames gives the reference of every frame count."""
    if (w, h) not in _sequential:
        scene, base, reg = sphere_case(rt4, w, h)
        us = [rt4.progressive_uniforms(base, n) for n in range(1, max(FRAME_COUNTS) + 1)]
        _sequential[(w, h)] = fresh(rt4, scene, us, reg, 0, False, snapshots=FRAME_COUNTS)
    return _sequential[(w, h)]


@pytest.mark.parametrize("n", FRAME_COUNTS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_frame_counts_and_ragged_sizes(rt4, oracle, size, n):
    """Sky above the horizon (the upper half, less the sphere in front of it) and ground below: the launch crosses
    from 16-iteration sky pixels to ground pixels. A queue item's frame is item % n, its tile item / n."""
    scene, base, reg = sphere_case(rt4, *size)
    sky, hit = classes(oracle, scene, base, reg)
    assert sky > 0 and hit > 0
    us = [rt4.progressive_uniforms(base, k) for k in range(1, n + 1)]
    p, np_ = fresh(rt4, scene, us, reg, 0, True, reserve=n % 2 == 1)[n]
    q, nq = sequential_sphere(rt4, *size)[n]
    assert np_ == nq
    assert same_bits(p, q)
    if n == 3:
        c, nc = oracle_frames(oracle, scene, us, reg, 0)
        assert np_ == nc
        assert same_bits(p, c)


@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
def test_progressive_formats(rt4, oracle, fmt):
    """A seed and a part per frame (progressive_uniforms), in fp32 and fp16, against the oracle and launch by launch."""
    scene, base, reg = sphere_case(rt4, 70, 37)
    us = [rt4.progressive_uniforms(base, k) for k in range(1, 6)]
    p, np_ = fresh(rt4, scene, us, reg, fmt, True)[5]
    q, nq = fresh(rt4, scene, us, reg, fmt, False)[5]
    c, nc = oracle_frames(oracle, scene, us, reg, fmt)
    assert np_ == nq == nc
    assert same_bits(p, q)
    assert same_bits(p, c)


@pytest.mark.parametrize("name", ["hypercube", "all_primitives"])
def test_several_tiles_per_claim(rt4, oracle, name):
    """The kernels that claim four queue items per atomic: a claim spans two tiles (4 items, 3 frames), and the
    last frame_tiles items are claimed one by one. The hypercube stands under a sky; all_primitives is closed and
    its tiger kernel keeps the frame-major queue."""
    scene = rt4.Scene.named(name)
    base = rt4.make_uniforms(70, 37, samples=SPP, reflections=BOUNCES, seed=515)
    reg = rt4.region(70, 37)
    sky, hit = classes(oracle, scene, base, reg)
    assert hit > 0 and (sky > 0) == (name == "hypercube")
    for n in (3, 7):
        us = [rt4.progressive_uniforms(base, k) for k in range(1, n + 1)]
        p, np_ = fresh(rt4, scene, us, reg, 0, True)[n]
        q, nq = fresh(rt4, scene, us, reg, 0, False)[n]
        assert np_ == nq
        assert same_bits(p, q)
        if n == 3:
            c, nc = oracle_frames(oracle, scene, us, reg, 0)
            assert np_ == nc
            assert same_bits(p, c)


def test_all_hit_scene_keeps_frame_major(rt4, oracle):
    """The room has no sky pixel; its lockstep kernel keeps the frame-major queue."""
    scene = rt4.Scene.named("room")
    base = rt4.make_uniforms(70, 37, samples=SPP, reflections=BOUNCES, seed=88)
    reg = rt4.region(70, 37)
    assert classes(oracle, scene, base, reg)[0] == 0
    us = [rt4.progressive_uniforms(base, k) for k in range(1, 6)]
    p, np_ = fresh(rt4, scene, us, reg, 0, True)[5]
    q, nq = fresh(rt4, scene, us, reg, 0, False)[5]
    c, nc = oracle_frames(oracle, scene, us, reg, 0)
    assert np_ == nq == nc
    assert same_bits(p, q)
    assert same_bits(p, c)


def test_all_sky_region(rt4, oracle):
    """A region of sky pixels only: every pixel ends after one find call per sample."""
    scene = rt4.Scene.named("sphere")
    base = rt4.make_uniforms(70, 80, samples=SPP, reflections=BOUNCES, seed=31)
    reg = rt4.region(70, 15)  # rows above the sphere
    assert classes(oracle, scene, base, reg) == (70 * 15, 0)
    us = [rt4.progressive_uniforms(base, k) for k in range(1, 4)]
    p, np_ = fresh(rt4, scene, us, reg, 0, True)[3]
    q, nq = fresh(rt4, scene, us, reg, 0, False)[3]
    assert np_ == nq == 3 * SPP * 70 * 15
    assert same_bits(p, q)


def test_banded_region(rt4, oracle):
    """A shard's band layout (8 rows of every 16) over sky and ground, ragged in both directions."""
    scene = rt4.Scene.named("sphere")
    base = rt4.make_uniforms(70, 80, samples=SPP, reflections=BOUNCES, seed=9)
    reg = rt4.region(70, 37, y0=3, band_rows=8, band_step=16)
    sky, hit = classes(oracle, scene, base, reg)
    assert sky > 0 and hit > 0
    us = [rt4.progressive_uniforms(base, k) for k in range(1, 5)]
    p, np_ = fresh(rt4, scene, us, reg, 0, True)[4]
    q, nq = fresh(rt4, scene, us, reg, 0, False)[4]
    c, nc = oracle_frames(oracle, scene, us, reg, 0)
    assert np_ == nq == nc
    assert same_bits(p, q)
    assert same_bits(p, c)


def test_order_cache_follows_the_camera(rt4, oracle):
    """One context, camera A twice, camera B, camera A again: nothing a context keeps from one call (the tile
    order of its serial launches is cached per camera) reaches the next; each image equals a fresh context's and
    the launch-by-launch frames."""
    scene = rt4.Scene.named("sphere")
    reg = rt4.region(72, 40)
    cam_a = rt4.make_uniforms(72, 40, samples=SPP, reflections=BOUNCES, seed=61)
    cam_b = rt4.make_uniforms(72, 40, samples=SPP, reflections=BOUNCES, seed=61, focus=(0.0, -2.0, -0.8, 0.0))
    # the sky at the tiles' centre pixels, which decide the classes: another partition of the tiles
    sky_a = (oracle.render(scene.desc, cam_a, reg, pixel_counts=True)[3] == SPP)[4::8, 4::8]
    sky_b = (oracle.render(scene.desc, cam_b, reg, pixel_counts=True)[3] == SPP)[4::8, 4::8]
    assert sky_a.any() and sky_b.any() and not np.array_equal(sky_a, sky_b)
    frames = {k: [rt4.progressive_uniforms(u, n) for n in range(1, 5)] for k, u in (("a", cam_a), ("b", cam_b))}
    want = {k: (fresh(rt4, scene, us, reg, 0, True)[4], fresh(rt4, scene, us, reg, 0, False)[4]) for k, us in frames.items()}
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=scene)
    try:
        for k in ("a", "a", "b", "a"):
            p, np_ = gpu_frames(rt4, t, frames[k], reg, 0, True)[4]
            for q, nq in want[k]:
                assert np_ == nq, k
                assert same_bits(p, q), k
    finally:
        t.close()
