"""Deferred hit shading in the deferred-sphere kernels (rt4_trace.hip RT4_DEFER_SHADE): a wave
parks its hit lanes until enough of them can be shaded in one trip. A parked lane draws no random number and counts
nothing, and its next find returns the same candidate, so every image and every intersection count must equal the
CPU oracle's bit for bit, whatever the threshold and the wait.

Every case runs on the product library and on the stress build lib_alt/shade/librt4.so (csrc/Makefile: a threshold
of 64 lanes and a wait of 7 iterations, pixel words outside the launch dropped), where nearly every hit parks for the
full wait, even on a one-wave image. The shapes are the smallest that reach each path of the rule:
  8x8, 4 spp, 8 bounces     one wave, sparse trips throughout: the wait expires (d), the last lanes fall under (c)
  24x16, 3 spp, 3 bounces   six tiles: the queue runs dry while lanes are parked
  16x8, 1 spp, 0 / 1 bounces every hit ends its path / the bounce limit and a parked hit coincide
  ground rows, sky rows     every primary ray hits / no lane ever hits
  70x37, 3 frames           pipelined progressive frames (partial tiles, every frame its own seed), f32 and f16
  40x24                     another scene on the same kernel, and the kernels the rule does not touch"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "4d_ray_tracing_amd")
STRESS = os.path.join(PKG, "lib_alt", "shade", "librt4.so")
BUILDS = ["product", "stress"]
SPHERE_SHAPE = 0x01030203  # kinds spaces | spheres, 1 space, 2 spheres, no cylinder: the deferred-sphere kernel
UNION_SHAPE = 0x01010209   # kinds spaces | cylinders union, 1 space: cylinder4d's kernel, no sphere
_libs = {}
_oracle = {}


def library(rt4, build):
    """None for the product (the package's own library), the loaded stress build otherwise."""
    if build == "product":
        return None
    if build not in _libs:
        if not os.path.exists(STRESS):
            pytest.fail(f"{STRESS} not built (make -C 4d_ray_tracing_amd/csrc all)")
        _libs[build] = rt4.load_variant(STRESS)
    return _libs[build]


def bits(a):
    return a.view(np.uint16 if a.dtype == np.float16 else np.uint32)


def oracle_frame(oracle, key, desc, u, reg, counts=False):
    """(frame, count, per-pixel counts) of one frame over zeros, computed once per case and shared by the builds."""
    if key not in _oracle:
        f, n, _, c = oracle.render(desc, u, reg, threads=4, pixel_counts=counts)
        _oracle[key] = (f, n, c)
    return _oracle[key]


def gpu_frame(rt4, build, scene, u, reg, flags=None, shape=None):
    t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT if flags is None else flags, scene=scene,
                   library=library(rt4, build))
    try:
        if shape is not None:
            assert t.kernel_shape == shape, f"kernel_shape {t.kernel_shape:#x}, expected {shape:#x}"
        frame = np.zeros((reg.h, reg.w, 4), np.float32)
        n = t.render_host(u, reg, frame)
    finally:
        t.close()
    return frame, n


def check_frame(rt4, oracle, build, name, scene, u, reg, flags=None, shape=None):
    want, n_want, _ = oracle_frame(oracle, name, scene.desc, u, reg)
    got, n_got = gpu_frame(rt4, build, scene, u, reg, flags, shape)
    assert n_got == n_want, f"{name} {build}: {n_got} intersections, the oracle counts {n_want}"
    assert np.array_equal(bits(got), bits(want)), f"{name} {build}: {int(np.any(got != want, axis=2).sum())} pixels differ"


@pytest.mark.parametrize("build", BUILDS)
def test_one_wave(rt4, oracle, build):
    """8x8, 4 spp, 8 bounces: one tile on one wave. After the primary hits the bounce rays mostly escape, so the
    wave's hit lanes are few in most iterations: they wait out RT4_DEFER_SHADE_WAIT (rule d), and the last active
    lanes of the launch are shaded under rule (c)."""
    u = rt4.make_uniforms(8, 8, samples=4, reflections=8, seed=901)
    check_frame(rt4, oracle, build, "one_wave", rt4.Scene.named("sphere"), u, rt4.region(8, 8), shape=SPHERE_SHAPE)


@pytest.mark.parametrize("build", BUILDS)
def test_queue_runs_dry_while_parked(rt4, oracle, build):
    """24x16, 3 spp, 3 bounces: six tiles. A 256-thread block holds four waves, so the tiles outnumber the waves
    that take them first and the queue empties while lanes of the last tiles are still parked."""
    u = rt4.make_uniforms(24, 16, samples=3, reflections=3, seed=902)
    check_frame(rt4, oracle, build, "queue_dry", rt4.Scene.named("sphere"), u, rt4.region(24, 16))


@pytest.mark.parametrize("bounces", [0, 1])
@pytest.mark.parametrize("build", BUILDS)
def test_bounce_limit(rt4, oracle, build, bounces):
    """16x8, 1 spp. Bounces 0: every hit ends its path in the trip that shades it. Bounces 1: a lane's second hit
    is at the bounce limit, so a parked hit and the end of its pixel coincide."""
    u = rt4.make_uniforms(16, 8, samples=1, reflections=bounces, seed=903 + bounces)
    check_frame(rt4, oracle, build, f"bounces_{bounces}", rt4.Scene.named("sphere"), u, rt4.region(16, 8))


GROUND = dict(w=64, h=16, x0=0, y0=24)  # rows 24..39 of a 64x40 image: the ground below the spheres
SKY = dict(w=64, h=8, x0=0, y0=0)       # rows 0..7: above the horizon and the spheres


@pytest.mark.parametrize("build", BUILDS)
def test_ground_only(rt4, oracle, build):
    """Rows 24..39 of the 64x40 sphere image, 4 spp, 8 bounces: every primary ray hits the ground. From the oracle's
    pixel_counts: a pixel whose primary ray misses counts exactly spp finds (all samples of a pixel share that ray),
    and here every pixel counts at least 2 x spp; the region's 1024 pixels run 4096 paths in 8865 finds, each path
    ends with at most one miss, so at least 4769 finds (53.8 %) are hits, against 38.8 % in the whole bench frame:
    every wave starts with a full hit trip and then thins out bounce by bounce."""
    spp = 4
    u = rt4.make_uniforms(64, 40, samples=spp, reflections=8, seed=31337)
    reg = rt4.region(**GROUND)
    scene = rt4.Scene.named("sphere")
    _, n_want, counts = oracle_frame(oracle, "ground", scene.desc, u, reg, counts=True)
    paths = spp * reg.w * reg.h
    assert int(counts.min()) >= 2 * spp  # every primary ray hits
    assert int(counts.sum()) == n_want == 8865
    assert n_want - paths == 4769  # finds that are hits, at the least: 53.8 %
    check_frame(rt4, oracle, build, "ground", scene, u, reg)


@pytest.mark.parametrize("build", BUILDS)
def test_sky_only(rt4, oracle, build):
    """Rows 0..7 of the same image: no ray ever hits, no lane ever parks, and the count is exactly spp x pixels."""
    spp = 4
    u = rt4.make_uniforms(64, 40, samples=spp, reflections=8, seed=31337)
    reg = rt4.region(**SKY)
    scene = rt4.Scene.named("sphere")
    _, n_want, counts = oracle_frame(oracle, "sky", scene.desc, u, reg, counts=True)
    assert n_want == spp * reg.w * reg.h and bool((counts == spp).all())
    check_frame(rt4, oracle, build, "sky", scene, u, reg)


@pytest.mark.parametrize("fmt", [0, 1], ids=["f32", "f16"])
@pytest.mark.parametrize("build", BUILDS)
def test_pipelined_progressive_frames(rt4, oracle, build, fmt):
    """Three progressive frames at 70x37 (partial tiles on both edges), pipelined in one call, against the same
    frames launch by launch and against the oracle's three frames."""
    import torch

    w, h = 70, 37
    scene = rt4.Scene.named("sphere")
    base = rt4.make_uniforms(w, h, samples=2, reflections=5, seed=906)
    us = [rt4.progressive_uniforms(base, n) for n in range(1, 4)]
    reg = rt4.region(w, h)
    key = ("frames", fmt)
    if key not in _oracle:
        want, n_want = np.zeros((h, w, 4), oracle.FRAME_DTYPES[fmt]), 0
        for u in us:
            _, k = oracle.render_fmt(scene.desc, u, reg, fmt, frame=want, threads=4)
            n_want += k
        _oracle[key] = (want, n_want)
    want, n_want = _oracle[key]
    tdt = torch.float32 if fmt == 0 else torch.float16
    for pipelined in (True, False):
        t = rt4.Tracer(device=0, flags=rt4.FLAG_SAMPLER_LUT, scene=scene, library=library(rt4, build))
        try:
            fr = torch.zeros((h, w, 4), dtype=tdt, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            s = torch.cuda.current_stream().cuda_stream
            if pipelined:
                t.render_frames_device(us, reg, fr.data_ptr(), fmt, w, cnt.data_ptr(), s)
            else:
                for u in us:
                    t.render_device_ex(u, reg, fr.data_ptr(), fmt, w, cnt.data_ptr(), s)
            torch.cuda.synchronize()
            got, n_got = fr.cpu().numpy(), int(cnt.item())
        finally:
            t.close()
        how = f"{build} {'pipelined' if pipelined else 'launch by launch'}"
        assert n_got == n_want, how
        assert np.array_equal(bits(got), bits(want)), how


def mirror_pair(rt4):
    """Another scene on the deferred-sphere kernel (one space, two spheres, the sphere scene's groups): two large
    mirror-like spheres close together over the ground, so paths bounce between them and a wave's hit lanes stay
    many for several bounces, the opposite of the sphere scene's quick escape to the sky."""
    d = rt4.SceneDesc.from_buffer_copy(rt4.Scene.builtin("sphere").to_bytes())
    for i, (x, r, refl, col) in enumerate([(-1.05, 1.0, 0.9, (0.9, 0.6, 0.3)), (0.8, 0.8, 0.6, (0.4, 0.5, 1.0))]):
        sp = d.spheres[i]
        sp.center[0], sp.center[1], sp.center[2], sp.center[3] = x, 1.0, 0.0, 0.0
        sp.r = r
        sp.material.glow = 0.0 if i == 0 else 1.5
        sp.material.refl_prob = refl
        sp.material.color[0], sp.material.color[1], sp.material.color[2] = col
    return rt4.Scene(d)


@pytest.mark.parametrize("build", BUILDS)
def test_other_scene_on_the_deferred_kernel(rt4, oracle, build):
    """40x24, 3 spp, 6 bounces on the mirror pair, which must select the deferred-sphere kernel. (The open
    reference scene cylinder4d has no sphere and runs the cylinders-union kernel: it is checked below with the
    kernels the rule does not touch.)"""
    u = rt4.make_uniforms(40, 24, samples=3, reflections=6, seed=907)
    check_frame(rt4, oracle, build, "mirror_pair", mirror_pair(rt4), u, rt4.region(40, 24), shape=SPHERE_SHAPE)


@pytest.mark.parametrize("kernel", ["generic", "reuse", "cylinder4d"])
@pytest.mark.parametrize("build", BUILDS)
def test_untouched_kernels_agree(rt4, oracle, build, kernel):
    """40x24: the sphere scene on the generic kernel and with primary reuse, and cylinder4d on its own kernel. None
    of them is a deferred-sphere kernel; they must agree with the oracle as before."""
    flags = rt4.FLAG_SAMPLER_LUT | {"generic": rt4.FLAG_GENERIC_KERNEL, "reuse": rt4.FLAG_PRIMARY_REUSE,
                                    "cylinder4d": 0}[kernel]
    name = "cylinder4d" if kernel == "cylinder4d" else "sphere"
    u = rt4.make_uniforms(40, 24, samples=3, reflections=4, seed=908)
    want, n_want, _ = oracle_frame(oracle, ("untouched", name), rt4.Scene.named(name).desc, u, rt4.region(40, 24))
    shape = {"generic": 0xFFFFFFFF, "reuse": SPHERE_SHAPE, "cylinder4d": UNION_SHAPE}[kernel]
    got, n_got = gpu_frame(rt4, build, rt4.Scene.named(name), u, rt4.region(40, 24), flags, shape)
    assert n_got == n_want, f"{kernel} {build}"
    assert np.array_equal(bits(got), bits(want)), f"{kernel} {build}"
