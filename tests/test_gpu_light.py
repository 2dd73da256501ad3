"""The HIP light accumulator (rt4.h rt4_render_light_device, rt4_light_resolve_device, rt4_light_noise_device) on the
GPU: one frame against the CPU oracle in every kernel variant, the fold, the resolve and the noise maps against their
definition restated in numpy (light_ref) bit for bit, the argument errors, and the colour accumulators after light
launches on the same context (they share the frame scratch)."""
import ctypes

import numpy as np
import pytest

import light_ref
from denoise_ref import region_rows

pytestmark = pytest.mark.gpu

ERR_ARG = -1
DT = {0: np.float32, 1: np.float16, 2: np.uint8}
FMT_IDS = ["f32", "f16", "rgba8"]
SCENES = ["sphere", "all_primitives", "tiger"]
FLAGS = {"default": 0, "generic": 0x2, "lut": 0x1, "reuse": 0x4, "serial": 0x8}
STATS_DTYPE = np.dtype([("pixels", "<u8"), ("measured", "<u8"), ("above", "<u8"), ("max_q", "<f4"), ("max_se", "<f4")])


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def copy_uniforms(rt4, u, **fields):
    c = rt4.Uniforms.from_buffer_copy(bytes(u))
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def as_ref(acc):
    """An rt4.LIGHT_DTYPE array as light_ref's (the same layout)."""
    return np.ascontiguousarray(acc).view(light_ref.LIGHT_DTYPE)


@pytest.fixture(scope="module")
def tracers(rt4):
    made = {}

    def get(flag_name):
        if flag_name not in made:
            made[flag_name] = rt4.Tracer(device=0, flags=FLAGS[flag_name])
        return made[flag_name]

    yield get
    for t in made.values():
        t.close()


# ------------------------------------------------------------------------------------------ 1. against the oracle
OW, OH, OSPP, OBOUNCES = 33, 17, 2, 3


@pytest.fixture(scope="module")
def oracle_frames(rt4, oracle):
    """{scene: (uniforms, the oracle's part = 1 frame (read-only), its intersection count)} at 33 x 17."""
    out = {}
    for name in SCENES:
        u = rt4.make_uniforms(OW, OH, samples=OSPP, reflections=OBOUNCES, seed=2024, part=1.0)
        frame, n, _, _ = oracle.render(rt4.Scene.named(name).desc, u, rt4.region(OW, OH))
        frame.setflags(write=False)
        out[name] = (u, frame, n)
    return out


@pytest.mark.parametrize("flag_name", list(FLAGS))
@pytest.mark.parametrize("name", SCENES)
def test_one_frame_against_the_oracle(rt4, tracers, oracle_frames, name, flag_name):
    """One frame into an empty accumulator: the resolved RGBA32F image is the oracle's part = 1 frame bit for bit, the
    count is the oracle's, and mean is the light behind the oracle's colour.

    The bound on mean: the oracle's colour is c = 1 - 1/fma(k, x, 1) in fp32, three roundings (the fma u, the quotient
    r = 1/u <= 1, the difference c = 1 - r < 1), each within 2^-24 of its result: |dc| <= (r + r + c) 2^-24 =
    (1 + r) 2^-24 <= 2 * 2^-24. The inversion x = c / (k (1 - c)) has dx/dc = (k x + 1)^2 / k, so the float64
    inversion of the oracle's colour lies within 2 * 2^-24 * (k x + 1)^2 / k of x to first order; 4 * leaves a factor
    of two for the second-order term where c is close to 1."""
    u, want, n_want = oracle_frames[name]
    t = tracers(flag_name)
    t.set_scene(rt4.Scene.named(name))
    acc, n_got = t.render_light_host([copy_uniforms(rt4, u, part=0.25)], rt4.region(OW, OH))  # part is ignored
    k = u.light_to_color_conversion_coefficient
    assert n_got == n_want
    assert (acc["n"] == 1).all() and not acc["m2"].any() and not acc["reserved"].any()
    image = t.light_resolve_host(acc, k)
    assert raw(image) == raw(want), (name, flag_name)
    c = want[..., :3].astype(np.float64)
    assert (c < 1).all()
    x64 = c / (k * (1.0 - c))
    err = np.abs(acc["mean"].astype(np.float64) - x64)
    bound = 4 * 2.0 ** -24 * (k * x64 + 1) ** 2 / k
    print(f"{name} {flag_name}: largest error / bound {np.max(err / bound):.3f}")
    assert (err <= bound).all()
    assert raw(acc["mean_y"]) == raw(light_ref.luminance(acc["mean"]))


# ------------------------------------------------------------------------------------------ 2. the fold
SHAPES = [(1, 1), (5, 3), (8, 8), (64, 1), (33, 17)]
POISON = 0xAB


def frame_uniforms(rt4, w, h, n, spp=2):
    return [rt4.make_uniforms(w, h, samples=spp, reflections=3, seed=s) for s in range(1, n + 1)]


def frames_light(tracer, rt4, us, reg):
    """Every frame's light (h, w, 3): the mean of a one-frame accumulation."""
    return [tracer.render_light_host([u], reg)[0]["mean"].copy() for u in us]


def padded_empty(rt4, h, w, extra):
    """An empty accumulator in the left w columns of a wider array whose padding holds other bytes."""
    a = np.zeros((h, w + extra), rt4.LIGHT_DTYPE)
    a.view(np.uint8).reshape(h, w + extra, 32)[:, w:] = POISON
    return a


def padding_kept(a, w):
    return (a.view(np.uint8).reshape(a.shape[0], a.shape[1], 32)[:, w:] == POISON).all()


@pytest.fixture(scope="module")
def folds(rt4, tracers):
    """{(w, h): (uniforms of 5 frames, their light, the reference accumulator after 1..5 frames)} of sphere."""
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    out = {}
    for w, h in SHAPES:
        us = frame_uniforms(rt4, w, h, 5)
        xs = frames_light(t, rt4, us, rt4.region(w, h))
        refs, acc = [], np.zeros((h, w), light_ref.LIGHT_DTYPE)
        for x in xs:
            acc = light_ref.apply(acc, x)
            acc.setflags(write=False)
            refs.append(acc)
        out[(w, h)] = (us, xs, refs)
    return out


@pytest.mark.parametrize("w, h", SHAPES)
def test_fold_equals_reference(rt4, tracers, folds, w, h):
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    us, xs, refs = folds[(w, h)]
    reg = rt4.region(w, h)
    assert any(x.any() for x in xs)
    for n in (1, 2, 3, 5):
        acc = padded_empty(rt4, h, w, n)
        t.render_light_host(us[:n], reg, acc)
        assert light_ref.same_acc(as_ref(acc[:, :w]), refs[n - 1]), (w, h, n)
        assert not acc["reserved"][:, :w].any() and padding_kept(acc, w)
    # 3 frames, then 2 onto them: the 5-frame accumulator
    acc = padded_empty(rt4, h, w, 2)
    t.render_light_host(us[:3], reg, acc)
    t.render_light_host(us[3:], reg, acc)
    assert light_ref.same_acc(as_ref(acc[:, :w]), refs[4]) and padding_kept(acc, w)
    if (w, h) == (33, 17):
        assert (refs[4]["m2"] > 0).any() and len(np.unique(refs[4]["mean_y"])) > 50  # there is something to get wrong


def test_fold_across_a_launch_boundary(rt4, tracers):
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    w = h = 8
    n = rt4.MAX_FRAMES + 1
    assert t.frames_per_launch(w, h) == rt4.MAX_FRAMES
    us = frame_uniforms(rt4, w, h, n, spp=1)
    reg = rt4.region(w, h)
    singles = [t.render_light_host([u], reg) for u in us]
    want = light_ref.fold(np.zeros((h, w), light_ref.LIGHT_DTYPE), [a["mean"] for a, _ in singles])
    got, count = t.render_light_host(us, reg)
    assert light_ref.same_acc(as_ref(got), want) and (got["n"] == n).all()
    assert count == sum(c for _, c in singles)


def test_fold_regions(rt4, tracers, folds):
    """A region with an offset and a banded region accumulate the pixels the whole frame does, at region-local places."""
    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    us, _, refs = folds[(33, 17)]
    whole = refs[2]
    sub = rt4.region(20, 9, x0=7, y0=5)
    acc, _ = t.render_light_host(us[:3], sub)
    assert light_ref.same_acc(as_ref(acc), whole[5:14, 7:27])
    total = 0
    for rank in range(3):
        reg, _ = rt4.band_plan(33, 17, 3, rank, band=2)
        assert reg.band_rows == 2 and reg.h > 0
        acc = padded_empty(rt4, reg.h, 33, 1)
        t.render_light_host(us[:3], reg, acc)
        assert light_ref.same_acc(as_ref(acc[:, :33]), whole[region_rows(reg)]), rank
        assert padding_kept(acc, 33)
        total += reg.h
    assert total == 17


# ------------------------------------------------------------------------------------------ 3. resolve and noise
def synthetic_acc(seed=5, w=33, h=17):
    """An accumulator no renderer made: n of 0, 1, 2 and INT32_MAX, m2 of 0, huge and NaN, mean_y of 0, inf and NaN,
    negative means (k * mean = -1 and below included), other bytes in reserved."""
    rng = np.random.default_rng(seed)
    a = np.zeros((h, w), light_ref.LIGHT_DTYPE)
    a["n"] = rng.choice(np.array([0, 1, 2, 3, 100, light_ref.INT32_MAX], np.int64), (h, w)).astype(np.int32)
    mean = (rng.random((h, w, 3)) * rng.choice([0.01, 1.0, 30.0], (h, w, 1))).astype(np.float32)
    pick = rng.random((h, w, 3))
    mean[pick < 0.1] = np.float32(-0.5)
    mean[(pick >= 0.1) & (pick < 0.15)] = np.float32(-1.0)
    mean[(pick >= 0.15) & (pick < 0.2)] = np.float32(-2.0)
    mean[(pick >= 0.2) & (pick < 0.25)] = np.float32(3e38)
    a["mean"] = mean
    my = (rng.random((h, w)) * 2).astype(np.float32)
    pick = rng.random((h, w))
    my[pick < 0.1] = 0.0
    my[(pick >= 0.1) & (pick < 0.2)] = np.inf
    my[(pick >= 0.2) & (pick < 0.3)] = np.nan
    my[(pick >= 0.3) & (pick < 0.35)] = -0.25
    a["mean_y"] = my
    m2 = (rng.random((h, w)) * 10).astype(np.float32)
    pick = rng.random((h, w))
    m2[pick < 0.15] = 0.0
    m2[(pick >= 0.15) & (pick < 0.3)] = np.float32(1e30)
    m2[(pick >= 0.3) & (pick < 0.4)] = np.nan
    m2[(pick >= 0.4) & (pick < 0.45)] = np.inf
    a["m2"] = m2
    a["reserved"] = 7.0
    return a


def check_resolve(rt4, tracer, acc, k, what):
    for fmt in (0, 1, 2):
        got = tracer.light_resolve_host(np.ascontiguousarray(acc).view(rt4.LIGHT_DTYPE), k, fmt)
        want = light_ref.resolve(acc, k, DT[fmt])
        assert got.dtype == want.dtype and raw(got) == raw(want), (what, FMT_IDS[fmt])


def check_noise(rt4, tracer, acc, k, thr, what, **outputs):
    got = tracer.light_noise_host(np.ascontiguousarray(acc).view(rt4.LIGHT_DTYPE), k, thr, **outputs)
    want = light_ref.noise(acc, k, thr)
    for g, w_, name in zip(got[:2], want[:2], ("se", "q")):
        assert g is None or light_ref.same_floats(g[:, :w_.shape[1]], w_), (what, name)  # a padded map: its image
    assert got[2] is None or raw(got[2]) == raw(want[2]), (what, "tiles")
    gs, ws = got[3], want[3]
    assert {f: gs[f] for f in ("pixels", "measured", "above")} == {f: ws[f] for f in ("pixels", "measured", "above")}, what
    assert np.float32(gs["max_q"]).tobytes() == np.float32(ws["max_q"]).tobytes(), (what, gs, ws)
    assert np.float32(gs["max_se"]).tobytes() == np.float32(ws["max_se"]).tobytes(), (what, gs, ws)
    return want


def thresholds_of(acc, k):
    """0, and values that equal a measured pixel's q exactly: the median, the largest and the smallest positive one."""
    _, q, _, _ = light_ref.noise(acc, k, 0.0)
    with np.errstate(invalid="ignore"):
        qs = np.sort(q[(acc["n"] >= 2) & np.isfinite(q) & (q > 0)])
    return [0.0] + ([float(qs[len(qs) // 2]), float(qs[-1]), float(qs[0])] if len(qs) else [])


def test_resolve_and_noise_rendered(rt4, tracers, folds):
    t = tracers("default")
    for (w, h) in ((33, 17), (5, 3), (64, 1)):
        acc = folds[(w, h)][2][4]
        check_resolve(rt4, t, acc, 1.0, (w, h))
        ths = thresholds_of(acc, 1.0)
        for thr in ths:
            want = check_noise(rt4, t, acc, 1.0, thr, (w, h, thr))
            if thr > 0:  # a pixel whose q equals the threshold is not above it, and shows
                assert (want[1] == np.float32(thr)).any()
        if (w, h) == (33, 17):
            assert len(ths) == 4
            counts = [light_ref.noise(acc, 1.0, thr)[3]["above"] for thr in ths]
            assert counts[2] == 0 and counts[0] > counts[3] > counts[1] > 0


@pytest.mark.parametrize("k", [1.0, 0.7])
def test_resolve_and_noise_synthetic(rt4, tracers, k):
    t = tracers("default")
    acc = synthetic_acc()
    se, q, _, stats = light_ref.noise(acc, k, 0.0)
    assert np.isnan(q).any() and np.isposinf(q).any() and (q == 0).any() and 0 < stats["measured"] < stats["pixels"]
    assert set(np.unique(acc["n"])) >= {0, 1, 2, light_ref.INT32_MAX}
    check_resolve(rt4, t, acc, k, ("synthetic", k))
    for thr in thresholds_of(acc, k) + [-1.0, float("nan"), float("inf")]:
        check_noise(rt4, t, acc, k, thr, ("synthetic", k, thr))
    # every optional output left out in turn, and all of them
    thr = thresholds_of(acc, k)[1]
    for leave in ("se", "q", "tiles"):
        check_noise(rt4, t, acc, k, thr, ("without", leave), **{leave: False})
    check_noise(rt4, t, acc, k, thr, "stats only", se=False, q=False, tiles=False)
    # padded maps keep their padding
    sem, qm = np.full((17, 40), 5.0, np.float32), np.full((17, 40), 6.0, np.float32)
    check_noise(rt4, t, acc, k, thr, "padded maps", w=33, se=sem, q=qm)
    assert (sem[:, 33:] == 5.0).all() and (qm[:, 33:] == 6.0).all()
    # padded accumulator and frame
    wide = np.zeros((17, 36), light_ref.LIGHT_DTYPE)
    wide[:, :33] = acc
    wide[:, 33:] = synthetic_acc(6, 3, 17)
    out = np.full((17, 35, 4), 9, np.float16)
    t.light_resolve_host(wide.view(rt4.LIGHT_DTYPE), k, 1, out=out, w=33)
    assert raw(out[:, :33]) == raw(light_ref.resolve(acc, k, np.float16)) and (out[:, 33:] == 9).all()
    got = t.light_noise_host(wide.view(rt4.LIGHT_DTYPE), k, thr, w=33)
    assert light_ref.same_floats(got[1], light_ref.noise(acc, k, thr)[1])


def test_noise_stats_do_not_accumulate(rt4, tracers):
    """Two calls into the same, poisoned d_stats: the second one's figures, not the sum."""
    import torch

    t = tracers("default")
    acc = synthetic_acc()
    h, w = acc.shape
    d_acc = torch.from_numpy(acc.view(np.uint8).reshape(h, w * 32).copy()).cuda()
    d_stats = torch.full((4,), -1, dtype=torch.int64, device="cuda")
    d_tiles = torch.full((3, 5), -1, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    thr = thresholds_of(acc, 1.0)[1]
    for rep in range(2):
        t.light_noise_device(d_acc.data_ptr(), w, w, h, 1.0, thr, 0, 0, w, d_tiles.data_ptr(), d_stats.data_ptr(), stream)
        torch.cuda.synchronize()
        got = np.frombuffer(d_stats.cpu().numpy().tobytes(), STATS_DTYPE)[0]
        _, _, tiles, want = light_ref.noise(acc, 1.0, thr)
        assert (int(got["pixels"]), int(got["measured"]), int(got["above"])) == (want["pixels"], want["measured"], want["above"]), rep
        assert got["max_q"] == np.float32(want["max_q"]) and got["max_se"] == np.float32(want["max_se"])
        assert raw(d_tiles.cpu().numpy()) == raw(tiles)
    assert raw(d_acc.cpu().numpy()) == raw(acc)  # the accumulator is read only


# ------------------------------------------------------------------------------------------ 4. errors
def test_argument_errors_write_nothing(rt4, tracers):
    import torch

    t = tracers("default")
    t.set_scene(rt4.Scene.named("sphere"))
    w, h = 16, 8
    u = rt4.make_uniforms(w, h, samples=1, reflections=1)
    # one buffer of rows of w 32-B records: the accumulator rows 0..7, an fp32 frame rows 8..11, the se map row 12, the
    # q map row 13, the tile image and the statistics row 14
    buf = torch.full((15 * w, 8), 0.25, dtype=torch.float32, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    row = w * 32
    p0 = buf.data_ptr()
    light, frame, se, q, tiles, stats = p0, p0 + 8 * row, p0 + 12 * row, p0 + 13 * row, p0 + 14 * row, p0 + 14 * row + 64
    reg = rt4.region(w, h)

    def status(fn, *args):
        try:
            fn(*args)
        except rt4.RT4Error as e:
            return e.status
        return 0

    def render(us=(u,), reg=reg, light=light, stride=w):
        return status(t.render_light_device, list(us), reg, light, stride, 0, stream)

    def render_raw(us, n_frames):  # what the binding cannot say: no uniforms, no frames
        err = ctypes.create_string_buffer(256)
        return rt4.lib.rt4_render_light_device(t._h, us, n_frames, ctypes.byref(reg), light, w, None, stream, err, len(err))

    assert render(light=0) == ERR_ARG and render_raw(None, 1) == ERR_ARG  # null pointers
    assert render_raw((rt4.Uniforms * 1)(u), 0) == ERR_ARG  # no frames
    assert render(light=light + 8) == ERR_ARG  # alignment
    assert render(stride=w - 1) == ERR_ARG
    assert render(reg=rt4.region(8192, 1), stride=8192) == ERR_ARG and render(reg=rt4.region(1, 8192), stride=1) == ERR_ARG
    assert render(us=(u, copy_uniforms(rt4, u, samples=2))) == ERR_ARG  # more than seed and part differ
    assert render(reg=rt4.region(w, h, band_rows=2, band_step=1)) == ERR_ARG

    def resolve(light=light, ls=w, frame=frame, fmt=0, fs=w, ww=w, hh=h):
        return status(t.light_resolve_device, light, ls, 1.0, frame, fmt, fs, ww, hh, stream)

    assert resolve(light=0) == ERR_ARG and resolve(frame=0) == ERR_ARG
    assert resolve(fmt=9) == ERR_ARG
    assert resolve(ls=w - 1) == ERR_ARG and resolve(fs=w - 1) == ERR_ARG
    assert resolve(ww=0) == ERR_ARG and resolve(hh=0) == ERR_ARG and resolve(ww=65536, ls=65536, fs=65536) == ERR_ARG
    assert resolve(light=light + 8) == ERR_ARG and resolve(frame=frame + 8) == ERR_ARG and resolve(frame=frame + 2, fmt=2) == ERR_ARG
    assert resolve(frame=light + 8 * row - 16) == ERR_ARG  # the frame's first pixel is the accumulator's last half record

    def noise(light=light, ls=w, ww=w, hh=h, se=se, q=q, ms=w, tiles=tiles, stats=stats):
        return status(t.light_noise_device, light, ls, ww, hh, 1.0, 0.1, se, q, ms, tiles, stats, stream)

    assert noise(light=0) == ERR_ARG and noise(stats=0) == ERR_ARG
    assert noise(ls=w - 1) == ERR_ARG and noise(ms=w - 1) == ERR_ARG
    assert noise(ww=0) == ERR_ARG and noise(hh=65536) == ERR_ARG
    assert noise(light=light + 8) == ERR_ARG and noise(se=se + 2) == ERR_ARG and noise(q=q + 1) == ERR_ARG
    assert noise(tiles=tiles + 2) == ERR_ARG and noise(stats=stats + 4) == ERR_ARG
    assert noise(se=light + 8 * row - 4) == ERR_ARG and noise(stats=light) == ERR_ARG  # an output inside the accumulator
    assert noise(q=se) == ERR_ARG and noise(tiles=stats) == ERR_ARG and noise(stats=q + 4 * (h - 1) * w) == ERR_ARG  # two outputs
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)
    # adjacent, not overlapping: accepted; the accumulator is written by the render only
    buf[:8 * w] = 0
    assert render() == 0 and resolve() == 0 and noise() == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    acc = after[:8 * w].view(rt4.LIGHT_DTYPE).reshape(h, w)
    assert (acc["n"] == 1).all()
    assert raw(after[8 * w:12 * w]) == raw(light_ref.resolve(as_ref(acc), 1.0))
    maps = after[12 * w:14 * w].reshape(2, -1)[:, :w * h]  # the se map and the q map, 128 floats of their 128-float rows
    assert np.isposinf(maps).all()  # n = 1: unmeasured
    got = np.frombuffer(after[14 * w:].tobytes()[64:96], STATS_DTYPE)[0]
    assert (int(got["pixels"]), int(got["measured"]), int(got["above"])) == (w * h, 0, 0)


# ------------------------------------------------------------------------------------------ 5. the default path
@pytest.mark.parametrize("flag_name", ["default", "serial"])
def test_colour_accumulators_after_light_launches(rt4, tracers, oracle, flag_name):
    """rt4_render_frames_device and rt4_render_device_ex after light launches on the same context still match the
    oracle: they share the frame-colour scratch."""
    import torch

    t = tracers(flag_name)
    scene = rt4.Scene.named("sphere")
    t.set_scene(scene)
    w, h = 33, 17
    reg = rt4.region(w, h)
    base = rt4.make_uniforms(w, h, samples=2, reflections=3, seed=99)
    us = [rt4.progressive_uniforms(base, n) for n in range(1, 4)]
    stream = torch.cuda.current_stream().cuda_stream
    light = torch.zeros((h, w, 8), dtype=torch.float32, device="cuda")
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    single = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    cnt = torch.zeros(3, dtype=torch.int64, device="cuda")
    t.render_light_device(us, reg, light.data_ptr(), w, cnt[0:].data_ptr(), stream)
    t.render_frames_device(us, reg, frame.data_ptr(), 0, w, cnt[1:].data_ptr(), stream)
    t.render_light_device(us[:1], reg, light.data_ptr(), w, cnt[0:].data_ptr(), stream)
    t.render_device_ex(us[0], reg, single.data_ptr(), 0, w, cnt[2:].data_ptr(), stream)
    torch.cuda.synchronize()
    want, m = np.zeros((h, w, 4), np.float32), []
    for uf in us:
        m.append(oracle.render_fmt(scene.desc, uf, reg, 0, frame=want)[1])
    first, _ = oracle.render_fmt(scene.desc, us[0], reg, 0)
    assert raw(frame.cpu().numpy()) == raw(want) and raw(single.cpu().numpy()) == raw(first)
    assert cnt.cpu().tolist() == [sum(m) + m[0], sum(m), m[0]]
    acc = light.cpu().numpy().view(rt4.LIGHT_DTYPE).reshape(h, w)
    assert (acc["n"] == 4).all()
