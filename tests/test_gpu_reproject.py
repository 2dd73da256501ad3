"""The HIP temporal reprojection (rt4.h rt4_reproject_device, rt4_temporal_blend_device, rt4_temporal) against its
definition restated in numpy (reproject_ref), bit for bit: rendered G-buffers and frames at the shared camera moves in
every format, synthetic G-buffers with the awkward values, degenerate sizes with padded strides, the parameter edges,
the blend against the plain progressive image, the stateful helper against the stateless entry points, the
end-to-end gain after a camera move, the argument errors and the --reproject switch of the host program."""
import os
import subprocess

import numpy as np
import pytest

import reproject_ref

pytestmark = pytest.mark.gpu

W, H = 61, 37
DT = {0: np.float32, 1: np.float16, 2: np.uint8}
FMT_IDS = ["f32", "f16", "rgba8"]
ERR_ARG = -1
POSE_NAMES = [n for n, _, _ in reproject_ref.POSES]


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def params_kw(p):
    return dict(cos_min=p.cos_min, plane_tol=p.plane_tol, slice_tol=p.slice_tol, max_refl_prob=p.max_refl_prob,
                max_history=p.max_history)


def copy_uniforms(rt4, u, **fields):
    c = rt4.Uniforms.from_buffer_copy(bytes(u))
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def check(rt4, tracer, u_cur, g_cur, u_prev, g_prev, acc, hist, p=None, what=""):
    """One reprojection on the GPU against the reference; returns the reference's (acc, hist, details)."""
    p = p if p is not None else rt4.reproject_params()
    got_acc, got_hist = tracer.reproject_host(u_cur, g_cur, u_prev, g_prev, acc, hist, p)
    want_acc, want_hist, d = reproject_ref.reproject(u_cur, g_cur, u_prev, g_prev, acc, hist, details=True, **params_kw(p))
    assert got_acc.dtype == acc.dtype
    assert raw(got_hist) == raw(want_hist), what
    assert raw(got_acc) == raw(want_acc), what
    return want_acc, want_hist, d


def random_history(h, w, seed):
    """0..5, a quarter of them zeros."""
    rng = np.random.default_rng(seed)
    hist = rng.integers(1, 6, (h, w)).astype(np.int32)
    hist[rng.random((h, w)) < 0.25] = 0
    return hist


# ------------------------------------------------------------------------------------------ 1. rendered input
@pytest.fixture(scope="module")
def rendered(rt4, tracer_lut):
    """{scene: dict(u_prev, g_prev, frames {fmt: 4-spp frame of the old view}, views {pose: (u, g)})} at 61 x 37."""
    out = {}
    reg = rt4.region(W, H)
    u_prev = rt4.make_uniforms(W, H, samples=4, reflections=4, seed=12345)
    for name in ("sphere", "all_primitives"):
        tracer_lut.set_scene(rt4.Scene.named(name))
        entry = dict(u_prev=u_prev, g_prev=tracer_lut.render_gbuffer_host(u_prev, reg), frames={}, views={})
        for fmt in (0, 1, 2):
            frame = np.zeros((H, W, 4), DT[fmt])
            tracer_lut.render_host_ex(u_prev, reg, frame, fmt)
            frame.setflags(write=False)
            entry["frames"][fmt] = frame
        for pose, kind, amount in reproject_ref.POSES:
            u = reproject_ref.pose_uniforms(rt4, W, H, kind, amount)
            g = tracer_lut.render_gbuffer_host(u, reg)
            g.setflags(write=False)
            entry["views"][pose] = (u, g)
        entry["g_prev"].setflags(write=False)
        out[name] = entry
    return out


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
@pytest.mark.parametrize("name", ["sphere", "all_primitives"])
def test_rendered_input_every_pose(rt4, tracer_lut, rendered, name, fmt):
    r = rendered[name]
    hist = random_history(H, W, 21)
    for pose in POSE_NAMES:
        u, g = r["views"][pose]
        _, want_hist, d = check(rt4, tracer_lut, u, g, r["u_prev"], r["g_prev"], r["frames"][fmt], hist, what=(name, fmt, pose))
        # the reference keeps and drops pixels in every case but two: the identity pose drops only where the old
        # history is 0, and the 0.3 move along w leaves no point of all_primitives inside the old slice
        assert d["kept"].any() != ((name, pose) == ("all_primitives", "w+0.3")), (name, pose)
        if pose != "identity":
            assert (d["eligible"] & ~d["kept"]).any(), (name, pose)
        assert want_hist.max() <= 5 and (want_hist[~d["kept"]] == 0).all()


# ------------------------------------------------------------------------------------------ 2. synthetic G-buffers
PLANE_D = 3.0  # the synthetic surface: the plane at this distance in front of the default camera


def pixel_world_width(u, w):
    return PLANE_D / 1.5 * u.mtr_sizes[0] / w  # focus_to_matrix 1.5 (rt4.make_uniforms)


def synthetic_view(rt4, u, h, w, seed, awkward=True):
    """A G-buffer no renderer made, for the camera u: a plane facing the default camera, surfaces numbered by world x
    (cells one pixel wide on the right half: stripes of alternating surfaces), then the awkward values sprinkled in."""
    rng = np.random.default_rng(seed)
    d = reproject_ref._directions(u, w, h).astype(np.float64)
    base = rt4.make_uniforms(w, h, samples=1, reflections=1)
    f = np.array(list(base.vec_to_mtr), np.float64)
    f /= np.linalg.norm(f)
    p0 = np.array(list(base.focus), np.float64) + PLANE_D * f  # a point of the plane
    with np.errstate(all="ignore"):
        z = ((p0 - np.array(list(u.focus), np.float64)) @ f) / (d @ f)
    X = np.array(list(u.focus), np.float64) + d * z[..., None]
    cell = pixel_world_width(base, w)
    xc = X[..., 0] + 0.5 * cell  # cell borders between the default camera's pixel centres
    with np.errstate(all="ignore"):
        sid = np.where(X[..., 0] > 0, np.floor(xc / cell).astype(np.int64) % 2, 2 + np.floor(xc / (5 * cell)).astype(np.int64) % 3)
    g = np.zeros((h, w), rt4.GBUFFER_DTYPE)
    n = np.broadcast_to(-f, (h, w, 4)).copy()
    refl = np.zeros((h, w), np.float32)
    if awkward:
        n += rng.normal(0, 0.12, (h, w, 4)) * (rng.random((h, w, 1)) < 0.3)  # some pairs fall under cos_min = 0.9
        n /= np.linalg.norm(n, axis=2, keepdims=True)
        n[rng.random((h, w)) < 0.05] = 0.0  # zero normals: every dot is 0
        z = z * np.where(rng.random((h, w)) < 0.15, 1.0 + rng.normal(0, 0.05, (h, w)), 1.0)  # off the tangent plane
        z[rng.random((h, w)) < 0.04] = np.nan
        z[rng.random((h, w)) < 0.04] = np.inf
        sid[rng.random((h, w)) < 0.06] = -1
        refl = rng.choice(np.array([0.0, 0.3, 0.5, 0.50000006, 0.7], np.float32), (h, w))
    g["normal"] = n.astype(np.float32)
    g["depth"] = z.astype(np.float32)
    g["surface"] = sid
    g["refl_prob"] = refl
    return g


def synthetic_frame(h, w, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    return (rng.random((h, w, 4)) * 1.5).astype(DT[fmt])  # alpha is not 1: the output's must be


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_synthetic_gbuffers(rt4, tracer_lut, fmt):
    w, h = 33, 17
    u_cur = rt4.make_uniforms(w, h, samples=1, reflections=1)
    g_cur = synthetic_view(rt4, u_cur, h, w, 7)
    elig = (g_cur["surface"] >= 0) & (g_cur["refl_prob"] <= np.float32(0.5)) & (np.abs(g_cur["depth"]) < np.inf)
    assert np.isnan(g_cur["depth"]).any() and np.isposinf(g_cur["depth"]).any() and (g_cur["surface"] < 0).any()
    assert ((g_cur["normal"] == 0).all(axis=2) & elig).any()
    assert (g_cur["refl_prob"] == np.float32(0.5)).any() and (g_cur["refl_prob"] == np.float32(0.50000006)).any()
    assert (np.diff(g_cur["surface"][:, w // 2 + 2:], axis=1) != 0).mean() > 0.5  # stripes one pixel wide
    acc = synthetic_frame(h, w, fmt, 8)
    hist = random_history(h, w, 9)
    seen = set()
    for pixels in (0.0, 0.5, -0.5, 1.5, -1.5, 0.25):  # fx = x + pixels on the plane
        focus = list(u_cur.focus)
        focus[0] = float(np.float32(focus[0] - pixels * pixel_world_width(u_cur, w)))
        u_prev = rt4.make_uniforms(w, h, samples=1, reflections=1, focus=tuple(focus))
        g_prev = synthetic_view(rt4, u_prev, h, w, 10)
        want_acc, _, d = check(rt4, tracer_lut, u_cur, g_cur, u_prev, g_prev, acc, hist, what=(fmt, pixels))
        assert not (d["kept"] & ~elig).any()
        if pixels in (0.5, 0.25):
            assert d["kept"].any() and (elig & ~d["kept"]).any()
            assert (want_acc[..., 3] == (255 if fmt == 2 else 1)).all()
        with np.errstate(invalid="ignore"):
            fx = d["fx"][elig]
            seen |= {"(-1,0)"} if ((fx > -1) & (fx < 0)).any() else set()
            seen |= {"(w-1,w)"} if ((fx > w - 1) & (fx < w)).any() else set()
            seen |= {"<-1"} if (fx < -1).any() else set()
            seen |= {">w"} if (fx > w).any() else set()
    assert seen == {"(-1,0)", "(w-1,w)", "<-1", ">w"}, seen
    # previous history 0 everywhere: everything restarts
    _, want_hist, d = check(rt4, tracer_lut, u_cur, g_cur, u_prev, g_prev, acc, np.zeros((h, w), np.int32), what="history 0")
    assert not d["kept"].any() and not want_hist.any()
    # a degenerate previous camera (vec_to_mtr = 0: a is 0 / 0): everything restarts
    u_deg = copy_uniforms(rt4, u_prev)
    for k in range(4):
        u_deg.vec_to_mtr[k] = 0.0
    want_acc, want_hist, d = check(rt4, tracer_lut, u_cur, g_cur, u_deg, g_prev, acc, hist, what="degenerate camera")
    assert not d["kept"].any() and not want_acc[..., :3].any()


# ------------------------------------------------------------------------------------------ 3. degenerate sizes
@pytest.mark.parametrize("w, h", [(1, 1), (5, 3), (8, 8), (64, 1)])
def test_degenerate_sizes_and_strides(rt4, tracer_lut, w, h):
    u_cur = rt4.make_uniforms(w, h, samples=1, reflections=1)
    focus = list(u_cur.focus)
    focus[0] = float(np.float32(focus[0] - 0.3 * pixel_world_width(u_cur, w)))
    u_prev = rt4.make_uniforms(w, h, samples=1, reflections=1, focus=tuple(focus))
    g_cur = synthetic_view(rt4, u_cur, h, w, 30 + w, awkward=False)
    g_prev = synthetic_view(rt4, u_prev, h, w, 31 + w, awkward=False)
    hist = np.full((h, w), 3, np.int32)
    for fmt in (0, 1, 2):
        acc = synthetic_frame(h, w, fmt, 32 + w)
        want_acc, want_hist, d = reproject_ref.reproject(u_cur, g_cur, u_prev, g_prev, acc, hist, details=True)
        assert d["kept"].any()

        def padded(a, extra, filler):  # the image in the left columns of a wider array with other bytes in the padding
            out = filler[:, :w + extra].copy()
            out[:, :w] = a
            return np.ascontiguousarray(out)

        # every stride padded by another amount; the outputs' padding keeps its bytes
        gc = padded(g_cur, 1, synthetic_view(rt4, rt4.make_uniforms(w + 1, h, 1, 1), h, w + 1, 1))
        gp = padded(g_prev, 2, synthetic_view(rt4, rt4.make_uniforms(w + 2, h, 1, 1), h, w + 2, 2))
        ap = padded(acc, 3, synthetic_frame(h, w + 3, fmt, 3))
        hp = padded(hist, 4, random_history(h, w + 4, 4))
        ao = synthetic_frame(h, w + 5, fmt, 5)
        ho = random_history(h, w + 6, 6) + 7
        ao0, ho0 = ao.copy(), ho.copy()
        tracer_lut.reproject_host(u_cur, gc, u_prev, gp, ap, hp, acc_out=ao, hist_out=ho, w=w)
        assert raw(ao[:, :w]) == raw(want_acc) and raw(ho[:, :w]) == raw(want_hist), (w, h, fmt)
        assert raw(ao[:, w:]) == raw(ao0[:, w:]) and raw(ho[:, w:]) == raw(ho0[:, w:])


# ------------------------------------------------------------------------------------------ 4. parameter edges
def test_parameter_edges(rt4, tracer_lut, rendered):
    r = rendered["all_primitives"]
    u, g = r["views"]["x+0.05"]
    hist = random_history(H, W, 41)
    args = (rt4, tracer_lut, u, g, r["u_prev"], r["g_prev"], r["frames"][0], hist)
    _, want_hist, d = check(*args, p=rt4.reproject_params(max_refl_prob=-1.0), what="max_refl_prob -1")
    assert not d["kept"].any() and not want_hist.any()  # nothing is eligible
    check(*args, p=rt4.reproject_params(cos_min=1.0), what="cos_min 1")
    check(*args, p=rt4.reproject_params(plane_tol=0.0), what="plane_tol 0")
    check(*args, p=rt4.reproject_params(slice_tol=0.0), what="slice_tol 0")
    _, want_hist, d = check(*args, p=rt4.reproject_params(max_history=1), what="max_history 1")
    assert d["kept"].any() and set(np.unique(want_hist)) == {0, 1}
    # the synthetic buffers under the same edges
    w, h = 33, 17
    u_cur = rt4.make_uniforms(w, h, samples=1, reflections=1)
    focus = list(u_cur.focus)
    focus[0] = float(np.float32(focus[0] - 0.25 * pixel_world_width(u_cur, w)))
    u_prev = rt4.make_uniforms(w, h, samples=1, reflections=1, focus=tuple(focus))
    sargs = (rt4, tracer_lut, u_cur, synthetic_view(rt4, u_cur, h, w, 42), u_prev, synthetic_view(rt4, u_prev, h, w, 43),
             synthetic_frame(h, w, 1, 44), random_history(h, w, 45))
    for kw in (dict(max_refl_prob=-1.0), dict(cos_min=1.0), dict(plane_tol=0.0), dict(slice_tol=0.0), dict(max_history=1)):
        check(*sargs, p=rt4.reproject_params(**kw), what=("synthetic", kw))


# ------------------------------------------------------------------------------------------ 5. blend
def gpu_blend(tracer, sample, acc, hist):
    """rt4_temporal_blend_device on copies of host arrays; returns (acc, hist) on the host."""
    import torch

    s, a, hh = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (sample, acc, hist))
    h, w = hist.shape
    fmt = {np.dtype("float32"): 0, np.dtype("float16"): 1, np.dtype("uint8"): 2}[acc.dtype]
    tracer.temporal_blend_device(s.data_ptr(), w, a.data_ptr(), w, fmt, hh.data_ptr(), w, w, h,
                                 torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return a.cpu().numpy(), hh.cpu().numpy()


@pytest.fixture(scope="module")
def progressive(rt4, tracer_lut):
    """Four progressive frames of sphere at 61 x 37: the uniforms, every frame's sample (part = 1 into one fp32 buffer)
    and the plain progressive image after every frame in each format."""
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    reg = rt4.region(W, H)
    base = rt4.make_uniforms(W, H, samples=2, reflections=4, seed=4242)
    us = [rt4.progressive_uniforms(base, n) for n in range(1, 5)]
    samples, sample = [], np.zeros((H, W, 4), np.float32)
    for u in us:
        tracer_lut.render_host_ex(copy_uniforms(rt4, u, part=1.0), reg, sample, 0)
        samples.append(sample.copy())
    plain = {}
    for fmt in (0, 1, 2):
        frame, plain[fmt] = np.zeros((H, W, 4), DT[fmt]), []
        for u in us:
            tracer_lut.render_host_ex(u, reg, frame, fmt)
            plain[fmt].append(frame.copy())
    return dict(base=base, us=us, samples=samples, plain=plain)


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_blend_equals_progressive(rt4, tracer_lut, progressive, fmt):
    acc, hist = np.zeros((H, W, 4), DT[fmt]), np.zeros((H, W), np.int32)
    for n, sample in enumerate(progressive["samples"], 1):
        acc, hist = gpu_blend(tracer_lut, sample, acc, hist)
        assert raw(acc) == raw(progressive["plain"][fmt][n - 1]), (fmt, n)
    assert (hist == 4).all()
    # a history of the pixel's own against the numpy blend
    rng = np.random.default_rng(51)
    hist = rng.integers(0, 300, (H, W)).astype(np.int32)
    hist[0, :4] = [0, 2 ** 31 - 2, 2 ** 31 - 1, 1]
    old = progressive["plain"][fmt][1]
    got_acc, got_hist = gpu_blend(tracer_lut, progressive["samples"][3], old, hist)
    want_acc, want_hist = reproject_ref.blend(progressive["samples"][3], old, hist)
    assert raw(got_hist) == raw(want_hist) and raw(got_acc) == raw(want_acc)


# ------------------------------------------------------------------------------------------ 6. rt4_temporal
@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_temporal_resting_camera(rt4, tracer_lut, progressive, fmt):
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    t = rt4.Temporal(tracer_lut, W, H, fmt)
    try:
        assert t.bytes() == W * H * (2 * np.dtype(DT[fmt]).itemsize * 4 + 2 * 4 + 2 * 32 + 16)
        for n, u in enumerate(progressive["us"], 1):
            t.frame(copy_uniforms(rt4, u, part=0.123))  # part is ignored
            assert raw(t.image()) == raw(progressive["plain"][fmt][n - 1]), (fmt, n)
        assert (t.history() == 4).all()
        assert raw(t.gbuffer()) == raw(tracer_lut.render_gbuffer_host(progressive["us"][0], rt4.region(W, H)))
    finally:
        t.close()


def stateless_step(rt4, tracer, state, u, fmt, params=None):
    """One rt4_temporal_frame_device from Python with the stateless entry points; state: dict(acc, hist, g, u, sample)."""
    reg = rt4.region(W, H)
    if state.get("u") is None:
        state["g"] = tracer.render_gbuffer_host(u, reg)
        state["hist"] = np.zeros((H, W), np.int32)
    elif any(bytes(getattr(u, f)) != bytes(getattr(state["u"], f))
             for f in ("resolution", "mtr_sizes", "focus", "vec_to_mtr", "top_drct", "right_drct")):
        g = tracer.render_gbuffer_host(u, reg)
        state["acc"], state["hist"] = tracer.reproject_host(u, g, state["u"], state["g"], state["acc"], state["hist"], params)
        state["g"] = g
    state["u"] = u
    tracer.render_host_ex(copy_uniforms(rt4, u, part=1.0), reg, state["sample"], 0)
    state["acc"], state["hist"] = gpu_blend(tracer, state["sample"], state["acc"], state["hist"])


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_temporal_moving_camera(rt4, tracer_lut, fmt):
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    poses = [("x", 0.0), ("x", 0.0), ("x", 0.05), ("x", 0.05), ("te", 0.05), ("w", 0.05)]
    us = [reproject_ref.pose_uniforms(rt4, W, H, kind, amount, samples=1, seed=1000 + n) for n, (kind, amount) in enumerate(poses)]
    t = rt4.Temporal(tracer_lut, W, H, fmt)
    try:
        state = dict(acc=np.zeros((H, W, 4), DT[fmt]), sample=np.zeros((H, W, 4), np.float32))
        for n, u in enumerate(us):
            t.frame(u)
            stateless_step(rt4, tracer_lut, state, u, fmt)
            assert raw(t.history()) == raw(state["hist"]), (fmt, n)
            assert raw(t.image()) == raw(state["acc"]), (fmt, n)
            assert raw(t.gbuffer()) == raw(state["g"]), (fmt, n)
        hist = t.history()
        assert hist.max() >= 3 and (hist == 1).any()  # history survived the moves, and some pixels restarted
        # after reset the next frame is a first frame
        t.reset()
        t.frame(us[-1])
        first = np.zeros((H, W, 4), DT[fmt])
        tracer_lut.render_host_ex(copy_uniforms(rt4, us[-1], part=1.0), rt4.region(W, H), first, fmt)
        assert raw(t.image()) == raw(first) and (t.history() == 1).all()
    finally:
        t.close()


# ------------------------------------------------------------------------------------------ 7. it helps
def test_history_survives_a_move_and_helps(rt4, tracer_lut):
    """16 temporal frames at pose A, then one at B (A moved +0.05 along x), 1 spp, against a 256-frame plain
    progressive image at B: where the history survived (>= 2 after the move) the temporal image is closer to it than a
    plain first frame at B with the same seed; where it restarted (history 1) the two are byte-equal."""
    import torch

    w, h = 64, 40
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    reg = rt4.region(w, h)
    base_a = reproject_ref.pose_uniforms(rt4, w, h, "x", 0.0, samples=1, seed=31337)
    base_b = reproject_ref.pose_uniforms(rt4, w, h, "x", 0.05, samples=1, seed=31337)
    u_b = rt4.progressive_uniforms(base_b, 17)
    t = rt4.Temporal(tracer_lut, w, h, 0)
    try:
        for n in range(1, 17):
            t.frame(rt4.progressive_uniforms(base_a, n))
        t.frame(u_b)
        temporal, hist = t.image(), t.history()
    finally:
        t.close()
    first = np.zeros((h, w, 4), np.float32)
    tracer_lut.render_host_ex(copy_uniforms(rt4, u_b, part=1.0), reg, first, 0)
    yard = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    target_base = reproject_ref.pose_uniforms(rt4, w, h, "x", 0.05, samples=1, seed=777)
    for lo in range(1, 257, 64):
        tracer_lut.render_frames_device([rt4.progressive_uniforms(target_base, n) for n in range(lo, lo + 64)], reg,
                                        yard.data_ptr(), 0, w, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    yard = yard.cpu().numpy()[..., :3].astype(np.float64)
    kept, restarted = hist >= 2, hist == 1
    assert kept.sum() > w * h // 4 and restarted.any() and (kept | restarted).all()
    assert (hist[kept] == 17).all()
    mae_t = np.abs(temporal[..., :3] - yard)[kept].mean()
    mae_1 = np.abs(first[..., :3] - yard)[kept].mean()
    print(f"pixels with history: MAE temporal {mae_t:.4f}, plain first frame {mae_1:.4f}")
    assert mae_t < mae_1
    assert raw(temporal[restarted]) == raw(first[restarted])


# ------------------------------------------------------------------------------------------ 8. errors
def test_argument_errors_write_nothing(rt4, tracer_lut):
    import torch

    w, h = 16, 8
    u = rt4.make_uniforms(w, h, samples=1, reflections=1)
    # one buffer of 16-B units, rows of w units: G_cur rows 0..15, G_prev 16..31 (32 B per pixel), acc_prev 32..39,
    # acc_out 40..47 (fp32 frames), hist_prev 48..49, hist_out 50..51 (4 B per pixel)
    buf = torch.full((52 * w, 4), 0.25, dtype=torch.float32, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    row = w * 16
    p0 = buf.data_ptr()
    gc, gp, ap, ao, hp, ho = p0, p0 + 16 * row, p0 + 32 * row, p0 + 40 * row, p0 + 48 * row, p0 + 50 * row
    ok = rt4.reproject_params()

    def status(*args, **kw):
        try:
            tracer_lut.reproject_device(*args, **kw)
        except rt4.RT4Error as e:
            return e.status
        return 0

    def call(u_cur=u, gc=gc, u_prev=u, gp=gp, ap=ap, hp=hp, ao=ao, ho=ho, fmt=0, ww=w, hh=h, p=ok, strides=(w,) * 6):
        return status(u_cur, gc, strides[0], u_prev, gp, strides[1], ap, strides[2], hp, strides[3], ao, strides[4], ho,
                      strides[5], fmt, ww, hh, p, stream)

    for name in ("gc", "gp", "ap", "hp", "ao", "ho"):
        assert call(**{name: 0}) == ERR_ARG, name  # null pointers
    assert call(u_cur=None) == ERR_ARG and call(u_prev=None) == ERR_ARG
    assert call(fmt=9) == ERR_ARG  # unknown format
    for k in range(6):
        assert call(strides=tuple(w - 1 if q == k else w for q in range(6))) == ERR_ARG  # stride below the width
    assert call(u_cur=rt4.make_uniforms(w + 1, h, 1, 1)) == ERR_ARG  # resolution != (w, h)
    assert call(u_prev=rt4.make_uniforms(w, h + 1, 1, 1)) == ERR_ARG
    assert call(p=rt4.reproject_params(max_history=0)) == ERR_ARG
    assert call(gc=gc + 4) == ERR_ARG and call(ap=ap + 4) == ERR_ARG and call(ho=ho + 2) == ERR_ARG  # alignment
    # each output overlapping each input by one pixel
    assert call(ao=gc + 16 * row - 16) == ERR_ARG  # acc_out's first pixel is G_cur's last half record
    assert call(ao=gp + 16 * row - 16) == ERR_ARG
    assert call(ao=ap + 8 * row - 16) == ERR_ARG
    assert call(ao=hp + 2 * row - 16, fmt=2) == ERR_ARG  # 4-B pixels: the last history element
    assert call(ho=gc + 16 * row - 4) == ERR_ARG
    assert call(ho=gp + 16 * row - 4) == ERR_ARG
    assert call(ho=ap + 8 * row - 4) == ERR_ARG
    assert call(ho=hp + 2 * row - 4) == ERR_ARG
    assert call(ao=ap) == ERR_ARG and call(ho=hp) == ERR_ARG  # in place
    assert call(ho=ao + 8 * row - 4) == ERR_ARG  # the two outputs
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)
    # adjacent, not overlapping: accepted, and the inputs keep their bytes
    assert call() == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:40 * w]) == raw(before[:40 * w]) and raw(after[48 * w:50 * w]) == raw(before[48 * w:50 * w])
    assert raw(after[40 * w:48 * w]) != raw(before[40 * w:48 * w])  # and the outputs were written
    # the blend's own checks
    def bstatus(*args):
        try:
            tracer_lut.temporal_blend_device(*args, stream)
        except rt4.RT4Error as e:
            return e.status
        return 0

    before = after.copy()
    assert bstatus(0, w, ao, w, 0, ho, w, w, h) == ERR_ARG and bstatus(ap, w, 0, w, 0, ho, w, w, h) == ERR_ARG
    assert bstatus(ap, w, ao, w, 0, 0, w, w, h) == ERR_ARG and bstatus(ap, w, ao, w, 9, ho, w, w, h) == ERR_ARG
    assert bstatus(ap, w - 1, ao, w, 0, ho, w, w, h) == ERR_ARG and bstatus(ap, w, ap, w, 0, ho, w, w, h) == ERR_ARG
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)


# ------------------------------------------------------------------------------------------ 9. rt4_render --reproject
def render_paths(rt4):
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    return os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")


def test_cpp_host_reproject(rt4, tracer_lut, tmp_path):
    exe, props_path = render_paths(rt4)
    w, h, seed, frames = 64, 40, 12345, 4
    common = [exe, "-p", props_path, "-s", "sphere", "-n", str(frames), "-W", str(w), "-H", str(h), "--seed", str(seed)]

    def run(tag, extra):
        pre = str(tmp_path / tag)
        r = subprocess.run(common + ["-o", pre] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return open(pre + "_yxz.ppm", "rb").read()

    moving = run("mv", ["--keys", "D", "--move-seconds", "0.02", "--reproject"])
    # the same loop from Python
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, w, h)
    cam = rt4.Camera(props)
    tracer_lut.set_scene(rt4.Scene.builtin("sphere"))
    t = rt4.Temporal(tracer_lut, w, h, 0)
    try:
        for n in range(1, frames + 1):
            t.frame(cam.frame_uniforms(base, rt4.SECTION_YXZ, seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)))
            cam.move(rt4.KEY_RIGHT, 0.02)
        image, hist = t.image(), t.history()
    finally:
        t.close()
    assert hist.max() == frames and (hist < frames).any()  # the camera did move, and history survived it
    rt4.write_ppm(str(tmp_path / "py.ppm"), image)
    assert open(str(tmp_path / "py.ppm"), "rb").read() == moving
    assert moving != run("mv_plain", ["--keys", "D", "--move-seconds", "0.02"])
    # a resting camera: the image of the run without the flag
    assert run("rest", ["--reproject"]) == run("rest_plain", [])
    # refused combinations name the flag
    for extra in (["--gpus", "2"], ["--resume", str(tmp_path / "none.ckpt")], ["--checkpoint", str(tmp_path / "c.ckpt")],
                  ["--frame-by-frame"]):
        r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8", "--reproject"] + extra,
                           capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and "--reproject" in r.stderr, extra


def test_cpp_host_reproject_three_sections_denoised(rt4, tracer_lut, tmp_path):
    """rt4_render -3 --reproject --denoise 2 with a moving camera: every section's temporal image and its filtered
    image equal the same steps from Python (properties.txt sizes)."""
    exe, props_path = render_paths(rt4)
    pre, seed, frames = str(tmp_path / "s"), 99, 3
    r = subprocess.run([exe, "-p", props_path, "-s", "tiger", "-n", str(frames), "-3", "--seed", str(seed), "--keys", "W",
                        "--move-seconds", "0.02", "--reproject", "--denoise", "2", "-o", pre],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    tracer_lut.set_scene(rt4.Scene.builtin("tiger"))
    sections = [(rt4.SECTION_YXZ, "yxz", "main"), (rt4.SECTION_YWZ, "ywz", "additional"), (rt4.SECTION_YXW, "yxw", "additional")]
    for sec, tag, window in sections:
        w, h = rt4.window_cells(props, window)
        base = rt4.uniforms_from_properties(props, w, h, sec)
        cam = rt4.Camera(props)
        t = rt4.Temporal(tracer_lut, w, h, 0)
        try:
            for n in range(1, frames + 1):
                t.frame(cam.frame_uniforms(base, sec, seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)))
                cam.move(rt4.KEY_FORWARD, 0.02)
            image, g = t.image(), t.gbuffer()
        finally:
            t.close()
        dn = tracer_lut.denoise_host(image, g, rt4.denoise_params(levels=2))
        for arr, suffix in ((image, ""), (dn, "_dn")):
            path = str(tmp_path / f"py_{tag}{suffix}.ppm")
            rt4.write_ppm(path, arr)
            assert open(path, "rb").read() == open(f"{pre}_{tag}{suffix}.ppm", "rb").read(), (tag, suffix)
