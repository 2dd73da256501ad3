"""The edges of the trace loop's refill (the inbox hand-out in at most two segments, the queue claim of one or
four tiles, the outbox ring) at the smallest shapes that reach them, through librt4.so against the CPU oracle:
images and intersection counts bit for bit, nothing tolerated.

Regions: 1x1 (one pixel), 8x8 (one tile), 13x11 (partial tiles on both edges: inbox entries with the "none"
pixel word), 67x9 (18 tiles, no multiple of the four-tile claim, so a claim straddles the frame boundary of a
pipelined launch and its spare tiles pick up the next frame's seed), 64x40 (40 tiles: with four tiles per claim a
wave owns 256 pixels, so its outbox ring overflows and is written out mid-launch).
Launches: one frame (overlapped and RT4_FLAG_SERIAL_FRAMES) and 2 and 5 progressive frames pipelined in one
rt4_render_frames_device call; every frame has its own seed and part, so a wrong frame or seed shows in the image.
spp 0 is the `active = NS > 0` path (a pixel goes from the inbox straight to the ring); its light sum over zero
samples is 0 / 0, and as everywhere in this suite (test_gpu_parity.bits_equal) a NaN equals a NaN:
the sign of the default NaN is the divider's (x86 and gfx950 differ), not the contract's. The caller's counter
starts nonzero: a launch adds to it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REGIONS = [(1, 1), (8, 8), (13, 11), (67, 9), (64, 40)]
SPP = (0, 1, 3)
BOUNCES = (0, 2)
COUNT0 = 1000003  # the counter's starting value

_tracers = {}
_oracle_frames = {}


@pytest.fixture(scope="module")
def tracer_of(rt4):
    """One context per flag word for the whole module (the scene is set per case)."""
    def get(flags, scene):
        t = _tracers.get(flags)
        if t is None:
            t = _tracers[flags] = rt4.Tracer(device=0, flags=flags)
        t.set_scene(scene)
        return t

    yield get
    for t in _tracers.values():
        t.close()
    _tracers.clear()


def same_bits(a, b):
    """Bit patterns equal, or both NaN (the suite's bar: test_gpu_parity.bits_equal)."""
    return bool(((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))).all())


def uniforms_of(rt4, reg, res, spp, bounces, n_frames):
    base = rt4.make_uniforms(res[0], res[1], samples=spp, reflections=bounces, seed=20241 + 7 * reg.w + reg.h)
    return [rt4.progressive_uniforms(base, n) for n in range(1, n_frames + 1)]


def oracle_frames(rt4, oracle, name, scene, reg, res, spp, bounces, n_frames):
    """(frame after n_frames progressive frames, their intersection count), computed once per case and shared:
    the frames of a shorter run are the first frames of a longer one."""
    key = (name, reg.w, reg.h, reg.y0, reg.band_step, res, spp, bounces)
    have = _oracle_frames.setdefault(key, [])
    us = uniforms_of(rt4, reg, res, spp, bounces, n_frames)
    while len(have) < n_frames:
        frame = have[-1][0].copy() if have else np.zeros((reg.h, reg.w, 4), np.float32)
        total = have[-1][1] if have else 0
        _, k = oracle.render_fmt(scene.desc, us[len(have)], reg, rt4.FRAME_RGBA32F, frame=frame, threads=4)
        have.append((frame, total + k))
    return have[n_frames - 1]


def gpu_frames(rt4, t, us, reg):
    """The frames of `us` into one zeroed device frame: a single frame through rt4_render_device_ex, several
    through one rt4_render_frames_device call. Returns (frame, counter - COUNT0)."""
    import torch

    fr = torch.zeros((reg.h, reg.w, 4), dtype=torch.float32, device="cuda")
    cnt = torch.full((1,), COUNT0, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    if len(us) == 1:
        t.render_device_ex(us[0], reg, fr.data_ptr(), rt4.FRAME_RGBA32F, reg.w, cnt.data_ptr(), s)
    else:
        t.render_frames_device(us, reg, fr.data_ptr(), rt4.FRAME_RGBA32F, reg.w, cnt.data_ptr(), s)
    torch.cuda.synchronize()
    return fr.cpu().numpy(), int(cnt.item()) - COUNT0


def check(rt4, oracle, tracer_of, name, flags, reg, res, spps=SPP, bounces=BOUNCES, serial=True):
    scene = rt4.Scene.named(name)
    for spp in spps:
        for nb in bounces:
            for n_frames, extra in ((1, 0), (1, rt4.FLAG_SERIAL_FRAMES), (2, 0), (5, 0)):
                if extra and not serial:
                    continue
                want, n_want = oracle_frames(rt4, oracle, name, scene, reg, res, spp, nb, n_frames)
                us = uniforms_of(rt4, reg, res, spp, nb, n_frames)
                got, n_got = gpu_frames(rt4, tracer_of(flags | extra, scene), us, reg)
                what = f"{name} {reg.w}x{reg.h} spp {spp} bounces {nb} frames {n_frames} flags {flags | extra:#x}"
                assert n_got == n_want, what
                assert same_bits(got, want), what


@pytest.mark.parametrize("wh", REGIONS, ids=lambda wh: f"{wh[0]}x{wh[1]}")
@pytest.mark.parametrize("sampler", ["lut", "inline"])
@pytest.mark.parametrize("name", ["sphere", "hypercube"])
def test_refill_edges_sphere_and_hypercube(rt4, oracle, tracer_of, name, sampler, wh):
    """The kernels of BASELINE configs 2 and 3 (deferred exact sphere tests; the hypercube), sampler table and
    inline sampler, over every region, sample count, bounce count and launch kind."""
    flags = rt4.FLAG_SAMPLER_LUT if sampler == "lut" else 0
    check(rt4, oracle, tracer_of, name, flags, rt4.region(*wh), wh)


@pytest.mark.parametrize("wh", [(13, 11), (67, 9)], ids=lambda wh: f"{wh[0]}x{wh[1]}")
@pytest.mark.parametrize("name", ["all_primitives", "tiger_two_mirrors"])
def test_refill_edges_tiger_kernels(rt4, oracle, tracer_of, name, wh):
    """The deferred-tiger (all_primitives) and lockstep (the mirror room) instantiations of the same loop."""
    check(rt4, oracle, tracer_of, name, rt4.FLAG_SAMPLER_LUT, rt4.region(*wh), wh)


@pytest.mark.parametrize("kernel", ["generic", "reuse"])
@pytest.mark.parametrize("name", ["sphere", "hypercube"])
def test_refill_edges_generic_and_primary_reuse(rt4, oracle, tracer_of, name, kernel):
    """The generic kernel and RT4_FLAG_PRIMARY_REUSE on the region with partial tiles."""
    flags = rt4.FLAG_SAMPLER_LUT | (rt4.FLAG_GENERIC_KERNEL if kernel == "generic" else rt4.FLAG_PRIMARY_REUSE)
    check(rt4, oracle, tracer_of, name, flags, rt4.region(13, 11), (13, 11))


@pytest.mark.parametrize("name", ["sphere", "hypercube"])
def test_refill_edges_band_region(rt4, oracle, tracer_of, name):
    """A band layout (every third row of a 67x27 image, one row per band): 67x9 pixels, 18 tiles."""
    reg = rt4.region(67, 9, y0=1, band_rows=1, band_step=3)
    check(rt4, oracle, tracer_of, name, rt4.FLAG_SAMPLER_LUT, reg, (67, 27))
