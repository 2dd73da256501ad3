"""The HIP upscale (rt4.h rt4_upscale_device, rt4_upscale_host, rt4_window) against its definition restated in numpy
(upscale_ref), bit for bit: rendered G-buffers and cell frames at every scale, format and mode, synthetic G-buffers with
the awkward values, degenerate sizes with padded strides, the parameter edges, host against device, the argument
errors, the stateful helper against the stateless entry points, its composition with the temporal image and the
filter, the --window switch of the host program, and the end-to-end gain over the reference's block stretch.

That a resting camera's present renders no G-buffer is checked by withholding the scene: after rt4_context_set_scene
to another scene without rt4_window_reset, a present at the same pose leaves rt4_window_gbuffer byte-equal."""
import os
import subprocess

import numpy as np
import pytest

import upscale_ref

pytestmark = pytest.mark.gpu

CW, CH = 24, 16
DT = {0: np.float32, 1: np.float16, 2: np.uint8}
FMT_IDS = ["f32", "f16", "rgba8"]
ERR_ARG = -1
SCALES = [1, 2, 3, 4, 7, 10, 64]
NEAREST, GUIDED = 0, 1


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def window_gbuffer(rt4, tracer, u_cells, s):
    uw = rt4.upscale_uniforms(u_cells, s)
    return tracer.render_gbuffer_host(uw, rt4.region(int(uw.resolution[0]), int(uw.resolution[1])))


def check(rt4, tracer, u, s, cells, gc, gw, p=None, what="", plan=None):
    """One guided upscale on the GPU against the reference; returns the reference's tap plan."""
    p = p if p is not None else rt4.upscale_params()
    got = tracer.upscale_host(u, s, cells, gc, gw, p)
    if plan is None:
        plan = upscale_ref.tap_plan(u, s, gc, gw, cos_min=p.cos_min, plane_tol=p.plane_tol)
    want = upscale_ref.apply_plan(plan, s, cells)
    assert got.dtype == cells.dtype and got.shape == want.shape
    assert raw(got) == raw(want), what
    return plan


# ------------------------------------------------------------------------------------------ 1. rendered input
@pytest.fixture(scope="module")
def rendered(rt4, tracer_lut):
    """{scene: dict(u, g (the cells' G-buffer), frames {fmt: a 4-spp cell frame})} at 24 x 16 cells."""
    out = {}
    reg = rt4.region(CW, CH)
    u = rt4.make_uniforms(CW, CH, samples=4, reflections=4, seed=12345)
    for name in ("sphere", "all_primitives"):
        tracer_lut.set_scene(rt4.Scene.named(name))
        entry = dict(u=u, g=tracer_lut.render_gbuffer_host(u, reg), frames={})
        entry["g"].setflags(write=False)
        for fmt in (0, 1, 2):
            frame = np.zeros((CH, CW, 4), DT[fmt])
            tracer_lut.render_host_ex(u, reg, frame, fmt)
            frame.setflags(write=False)
            entry["frames"][fmt] = frame
        out[name] = entry
    return out


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("name", ["sphere", "all_primitives"])
def test_rendered_input(rt4, tracer_lut, rendered, name, s):
    r = rendered[name]
    tracer_lut.set_scene(rt4.Scene.named(name))
    gw = window_gbuffer(rt4, tracer_lut, r["u"], s)
    plan = None
    for fmt in (0, 1, 2):
        cells = r["frames"][fmt]
        plan = check(rt4, tracer_lut, r["u"], s, cells, r["g"], gw, what=(name, s, fmt), plan=plan)
        near = tracer_lut.upscale_host(r["u"], s, cells, params=rt4.upscale_params(mode=NEAREST))
        assert raw(near) == raw(upscale_ref.nearest(cells, s)), (name, s, fmt, "nearest")
        assert raw(near) == raw(tracer_lut.upscale_host(r["u"], s, cells, r["g"], gw, rt4.upscale_params(mode=NEAREST)))
    assert plan["counted"].any()
    if name == "sphere":
        assert plan["kept"][gw["surface"] < 0].any()  # the sky interpolates among sky cells
    if s >= 2:  # no case passes vacuously: taps counted, taps dropped, and pixels that fall back to their cell
        assert (plan["candidates"] > plan["counted"]).any(), (name, s)
        assert (~plan["kept"]).any(), (name, s)
        assert (plan["counted"] == 4).any(), (name, s)


# ------------------------------------------------------------------------------------------ 2. synthetic G-buffers
PLANE_D = 3.0  # the synthetic surface: the plane at this distance in front of the default camera


def plane_view(rt4, u, w, h):
    """Depth and normal of the plane for the w x h image of camera u (float64 depth, float32 normal)."""
    d = upscale_ref._directions(u, w, h).astype(np.float64)
    f = np.array(list(u.vec_to_mtr), np.float64)
    f /= np.linalg.norm(f)
    return PLANE_D / (d @ f), (-f).astype(np.float32)


def synthetic(rt4, u, cw, ch, s, seed, awkward=True):
    """(g_cells, g_win) no renderer made: the plane facing the camera; cells numbered in stripes one cell wide on the
    right half and one surface on the left; the window's surfaces are those of the cell one window pixel to the right
    (so edges fall inside cells), plus a patch of a surface that no cell has; then the awkward values sprinkled in."""
    rng = np.random.default_rng(seed)
    dt = rt4.GBUFFER_DTYPE
    out = []
    for (w, h, k) in ((cw, ch, 1), (cw * s, ch * s, s)):
        uk = upscale_ref.window_uniforms(u, k)
        z, n = plane_view(rt4, uk, w, h)
        g = np.zeros((h, w), dt)
        cx = np.minimum((np.arange(w) + (1 if k > 1 else 0)) // k, cw - 1)
        sid = np.where(cx >= cw // 2, cx % 2, 2)
        sid = np.broadcast_to(sid[None, :], (h, w)).copy()
        nn = np.broadcast_to(n, (h, w, 4)).astype(np.float64).copy()
        if k > 1 and h >= 3 and w >= 3:
            sid[h // 3:h // 3 + max(1, k // 2), w // 4:w // 4 + k + 1] = 9  # a window-only surface: the fallback
        if awkward:
            nn += rng.normal(0, 0.12, (h, w, 4)) * (rng.random((h, w, 1)) < 0.3)  # some pairs fall under cos_min = 0.9
            nn /= np.linalg.norm(nn, axis=2, keepdims=True)
            nn[rng.random((h, w)) < 0.05] = 0.0  # zero normals: every dot is 0
            z = z * np.where(rng.random((h, w)) < 0.2, 1.0 + rng.normal(0, 0.05, (h, w)), 1.0)  # off the tangent plane
            z[rng.random((h, w)) < 0.05] = np.nan
            z[rng.random((h, w)) < 0.05] = np.inf
            sid[rng.random((h, w)) < 0.08] = -1  # misses next to hits
            my, mx = h // 2, w // 2  # and one of each kind for certain, side by side in the middle row
            nn[my, mx], sid[my, mx] = 0.0, abs(sid[my, mx])
            z[my, mx - 1], z[my, mx - 2], sid[my, mx + 1] = np.nan, np.inf, -1
        g["normal"] = nn.astype(np.float32)
        g["depth"] = z.astype(np.float32)
        g["surface"] = sid
        g["refl_prob"] = rng.choice(np.array([0.0, 0.7], np.float32), (h, w))  # no reflectance threshold: ignored
        out.append(g)
    return out[0], out[1]


def synthetic_frame(h, w, fmt, seed):
    rng = np.random.default_rng(seed)
    if fmt == 2:
        return rng.integers(0, 256, (h, w, 4)).astype(np.uint8)
    return (rng.random((h, w, 4)) * 1.5).astype(DT[fmt])  # alpha is not 1: a computed pixel's must be


@pytest.mark.parametrize("s", [3, 7])
def test_synthetic_gbuffers(rt4, tracer_lut, s):
    cw, ch = 11, 5
    u = rt4.make_uniforms(cw, ch, samples=1, reflections=1)
    gc, gw = synthetic(rt4, u, cw, ch, s, 7 + s)
    for g in (gc, gw):
        assert np.isnan(g["depth"]).any() and np.isposinf(g["depth"]).any() and (g["surface"] < 0).any()
        assert ((g["normal"] == 0).all(axis=2) & (g["surface"] >= 0)).any()
    assert (np.diff(gc["surface"][:, cw // 2:], axis=1) != 0).mean() > 0.5  # stripes one cell wide
    assert (gw["surface"] == 9).any() and not (gc["surface"] == 9).any()
    plan = None
    for fmt in (0, 1, 2):
        cells = synthetic_frame(ch, cw, fmt, 8 + fmt)
        plan = check(rt4, tracer_lut, u, s, cells, gc, gw, what=(s, fmt), plan=plan)
        got = tracer_lut.upscale_host(u, s, cells, gc, gw)
        one = 255 if fmt == 2 else 1
        assert (got[..., 3][plan["kept"]] == one).all()
        near = upscale_ref.nearest(cells, s)
        assert raw(got[~plan["kept"]]) == raw(near[~plan["kept"]])  # the fallback: the cell's bits, alpha included
    kept, bad_z = plan["kept"], ~np.isfinite(gw["depth"])
    assert not kept[(gw["surface"] == 9)].any()  # no cell has the surface
    assert not kept[bad_z & (gw["surface"] >= 0)].any()  # a hit with a non-finite depth has no counted tap
    assert kept[gw["surface"] < 0].any()  # misses interpolate among misses, whatever their depth and normal
    assert kept.any() and (~kept).any() and (plan["candidates"] > plan["counted"]).any()


def test_cos_min_exactly_and_one_ulp_below(rt4, tracer_lut):
    """Window row 0 taps cell row 0 only. Its pixels have the normal (1,0,0,0); the cells' normals alternate between
    x = cos_min exactly (the dot is cos_min: counts) and x one ulp below (dropped). plane_tol = +inf takes the plane
    test out of the way."""
    cw, ch, s = 11, 5, 3
    u = rt4.make_uniforms(cw, ch, samples=1, reflections=1)
    gc, gw = synthetic(rt4, u, cw, ch, s, 21, awkward=False)
    gc["surface"], gw["surface"] = 0, 0
    c = np.float32(0.9)
    below = np.nextafter(c, np.float32(0))
    exact = np.arange(cw) % 2 == 0
    gc["normal"][0] = 0
    gc["normal"][0, :, 0] = np.where(exact, c, below)
    gc["normal"][0, :, 1] = np.sqrt(np.float32(1) - c * c)
    gw["normal"][0] = (1, 0, 0, 0)
    p = rt4.upscale_params(cos_min=float(c), plane_tol=float("inf"))
    assert np.float32(p.cos_min) == c
    cells = synthetic_frame(ch, cw, 0, 22)
    plan = check(rt4, tracer_lut, u, s, cells, gc, gw, p, what="cos_min edge")
    x0, ax = upscale_ref.tap_positions(cw, s)
    want = np.zeros(cw * s, np.int32)
    for tx, k in ((0, 1 - ax), (1, ax)):
        q = x0 + tx
        inside = (q >= 0) & (q < cw) & (k > 0)
        want += inside & exact[np.clip(q, 0, cw - 1)]
    assert np.array_equal(plan["counted"][0], want) and (want == 0).any() and (want == 1).any()


def test_plane_distance_exactly_at_tol(rt4, tracer_lut):
    """A window pixel of depth 2 (so tol = 2 * plane_tol exactly) and one of its taps at the plane distance D > 0:
    plane_tol = D / 2 counts the tap, one ulp below drops it."""
    cw, ch, s = 11, 5, 3
    u = rt4.make_uniforms(cw, ch, samples=1, reflections=1)
    gc, gw = synthetic(rt4, u, cw, ch, s, 31, awkward=False)
    gc["surface"], gw["surface"] = 0, 0
    y, x = 8, 17  # both coordinates off their cell's centre: four taps with k > 0
    gw["depth"][y, x] = 2.0
    probe = upscale_ref.tap_plan(u, s, gc, gw, cos_min=-1.0, plane_tol=float("inf"))
    assert probe["counted"][y, x] == 4
    t, D = max(((t, probe["dist"][t][y, x]) for t in range(4)), key=lambda v: v[1])
    assert np.isfinite(D) and D > 0 and probe["taps"][t][3][y, x]
    tol_at = np.float32(D) / np.float32(2)
    assert tol_at * np.float32(2) == np.float32(D)
    cells = synthetic_frame(ch, cw, 0, 32)
    at = check(rt4, tracer_lut, u, s, cells, gc, gw, rt4.upscale_params(cos_min=-1.0, plane_tol=float(tol_at)), what="at tol")
    under = check(rt4, tracer_lut, u, s, cells, gc, gw,
                  rt4.upscale_params(cos_min=-1.0, plane_tol=float(np.nextafter(tol_at, np.float32(0)))), what="below tol")
    assert at["taps"][t][3][y, x] and not under["taps"][t][3][y, x]


# ------------------------------------------------------------------------------------------ 3. sizes and strides
@pytest.mark.parametrize("cw, ch, s", [(1, 1, 1), (1, 1, 7), (1, 1, 64), (5, 3, 2), (5, 3, 3), (9, 2, 10), (64, 1, 1), (3, 40, 5)])
def test_sizes_and_strides(rt4, tracer_lut, cw, ch, s):
    u = rt4.make_uniforms(cw, ch, samples=1, reflections=1)
    gc, gw = synthetic(rt4, u, cw, ch, s, 40 + cw + s, awkward=False)
    W, H = cw * s, ch * s
    plan = upscale_ref.tap_plan(u, s, gc, gw)
    assert plan["kept"].any()

    def padded(a, extra, filler):  # the image in the left columns of a wider array with other bytes in the padding
        out = filler[:, :a.shape[1] + extra].copy()
        out[:, :a.shape[1]] = a
        return np.ascontiguousarray(out)

    junk_c = synthetic(rt4, rt4.make_uniforms(cw + 2, ch, 1, 1), cw + 2, ch, 1, 1)[0]
    junk_w = synthetic(rt4, rt4.make_uniforms(W + 3, H, 1, 1), W + 3, H, 1, 2)[0]
    for fmt in (0, 1, 2):
        cells = synthetic_frame(ch, cw, fmt, 50 + fmt)
        want = upscale_ref.apply_plan(plan, s, cells)
        cp = padded(cells, 1, synthetic_frame(ch, cw + 1, fmt, 3))
        gcp, gwp = padded(gc, 2, junk_c), padded(gw, 3, junk_w)
        for mode, expect in ((GUIDED, want), (NEAREST, upscale_ref.nearest(cells, s))):
            out = synthetic_frame(H, W + 4, fmt, 5)
            out0 = out.copy()
            tracer_lut.upscale_host(u, s, cp, gcp, gwp, rt4.upscale_params(mode=mode), out=out, cells_w=cw)
            assert raw(out[:, :W]) == raw(expect), (cw, ch, s, fmt, mode)
            assert raw(out[:, W:]) == raw(out0[:, W:])


# ------------------------------------------------------------------------------------------ 4. parameter edges
def test_parameter_edges(rt4, tracer_lut, rendered):
    r = rendered["all_primitives"]
    tracer_lut.set_scene(rt4.Scene.named("all_primitives"))
    s = 3
    gw = window_gbuffer(rt4, tracer_lut, r["u"], s)
    u2 = rt4.make_uniforms(11, 5, samples=1, reflections=1)
    sc, sw = synthetic(rt4, u2, 11, 5, s, 61)
    cells2 = synthetic_frame(5, 11, 1, 62)
    hits = gw["surface"] >= 0
    for kw in (dict(plane_tol=0.0), dict(plane_tol=float("inf")), dict(plane_tol=float("nan")), dict(cos_min=-1.0),
               dict(cos_min=1.0), dict(cos_min=2.0)):
        plan = check(rt4, tracer_lut, r["u"], s, r["frames"][0], r["g"], gw, rt4.upscale_params(**kw), what=kw)
        if kw.get("cos_min") == 2.0 or "nan" in str(kw.get("plane_tol")):
            assert hits.any() and not plan["kept"][hits].any()  # every hit falls back to its cell
        else:
            assert plan["kept"][hits].any()
        check(rt4, tracer_lut, u2, s, cells2, sc, sw, rt4.upscale_params(**kw), what=("synthetic", kw))


# ------------------------------------------------------------------------------------------ 5. host and device
def to_gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_host_equals_device(rt4, tracer_lut, rendered, fmt):
    import torch

    r = rendered["sphere"]
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    s = 4
    gw = window_gbuffer(rt4, tracer_lut, r["u"], s)
    cells = r["frames"][fmt]
    W, H = CW * s, CH * s
    stream = torch.cuda.current_stream().cuda_stream
    for mode in (GUIDED, NEAREST):
        p = rt4.upscale_params(mode=mode)
        host = tracer_lut.upscale_host(u_cells=r["u"], scale=s, cells=cells, gcells=r["g"], gwin=gw, params=p)
        dc, dgc, dgw = to_gpu(cells), to_gpu(r["g"]), to_gpu(gw)
        out = torch.zeros(host.nbytes, dtype=torch.uint8, device="cuda")
        tracer_lut.upscale_device(r["u"], s, dc.data_ptr(), CW, dgc.data_ptr() if mode == GUIDED else 0, CW,
                                  dgw.data_ptr() if mode == GUIDED else 0, W, out.data_ptr(), W, fmt, CW, CH, p, stream)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == raw(host), (fmt, mode)


# ------------------------------------------------------------------------------------------ 6. errors
def test_argument_errors_write_nothing(rt4, tracer_lut):
    import torch

    cw, ch, s = 8, 4, 2
    W, H = cw * s, ch * s
    u = rt4.make_uniforms(cw, ch, samples=1, reflections=1)
    # one buffer of 16-B units: cells (fp32) 32 units, G_cells 64, G_win 256, out 128
    n_c, n_gc, n_gw, n_o = cw * ch, 2 * cw * ch, 2 * W * H, W * H
    buf = torch.full((n_c + n_gc + n_gw + n_o, 4), 0.25, dtype=torch.float32, device="cuda")
    buf[:n_c] = 0.5  # the cells differ from what the output holds
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    p0 = buf.data_ptr()
    c, gc, gw, o = p0, p0 + 16 * n_c, p0 + 16 * (n_c + n_gc), p0 + 16 * (n_c + n_gc + n_gw)
    ok = rt4.upscale_params()

    def call(uu=u, scale=s, c=c, gc=gc, gw=gw, o=o, fmt=0, ww=cw, hh=ch, p=ok, strides=(cw, cw, W, W)):
        try:
            tracer_lut.upscale_device(uu, scale, c, strides[0], gc, strides[1], gw, strides[2], o, strides[3], fmt, ww, hh, p, stream)
        except rt4.RT4Error as e:
            return e.status
        return 0

    for name in ("c", "gc", "gw", "o"):
        assert call(**{name: 0}) == ERR_ARG, name  # null pointers
    assert call(uu=None) == ERR_ARG
    assert call(fmt=9) == ERR_ARG and call(fmt=-1) == ERR_ARG  # unknown format
    assert call(p=rt4.upscale_params(mode=2)) == ERR_ARG and call(p=rt4.upscale_params(mode=-1)) == ERR_ARG  # unknown mode
    assert call(scale=0) == ERR_ARG and call(scale=65) == ERR_ARG and call(scale=-3) == ERR_ARG
    assert call(uu=rt4.make_uniforms(cw + 1, ch, 1, 1)) == ERR_ARG and call(uu=rt4.make_uniforms(cw, ch + 1, 1, 1)) == ERR_ARG
    assert call(ww=cw - 1) == ERR_ARG and call(hh=ch + 1) == ERR_ARG  # resolution != (cells_w, cells_h)
    for k, width in enumerate((cw, cw, W, W)):
        assert call(strides=tuple(width - 1 if q == k else v for q, v in enumerate((cw, cw, W, W)))) == ERR_ARG, k
    assert call(gc=gc + 4) == ERR_ARG and call(gw=gw + 8) == ERR_ARG  # alignment: G-buffers 16 B
    assert call(c=c + 4) == ERR_ARG and call(o=o + 8) == ERR_ARG  # fp32 frames 16 B
    assert call(c=c + 2, fmt=2) == ERR_ARG and call(o=o + 4, fmt=1) == ERR_ARG  # RGBA8 4 B, half 8 B
    # the output overlapping each input by one pixel, and in place
    assert call(o=c + 16 * n_c - 16) == ERR_ARG
    assert call(o=gc + 16 * n_gc - 16) == ERR_ARG
    assert call(o=gw + 16 * n_gw - 16) == ERR_ARG
    assert call(o=c) == ERR_ARG and call(c=o + 16 * n_o - 16) == ERR_ARG
    nearest = rt4.upscale_params(mode=NEAREST)
    assert call(p=nearest, c=0) == ERR_ARG and call(p=nearest, o=c) == ERR_ARG and call(p=nearest, scale=65) == ERR_ARG
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)
    # adjacent, not overlapping: accepted; NEAREST accepts NULL and anything else for both G-buffers
    assert call(p=nearest, gc=0, gw=0) == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:n_c + n_gc + n_gw]) == raw(before[:n_c + n_gc + n_gw])
    assert (after[n_c + n_gc + n_gw:] == 0.5).all()  # and the output was written
    buf[n_c + n_gc + n_gw:] = 0.25
    assert call(p=nearest, gc=gc + 4, gw=o) == 0
    # guided: every record of these G-buffers is the same hit with normals of length 0.5, so every dot is 0.25 and no
    # tap counts: the fallback
    assert call() == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:n_c + n_gc + n_gw]) == raw(before[:n_c + n_gc + n_gw]) and (after[n_c + n_gc + n_gw:] == 0.5).all()
    # the host variant's own checks
    cells = np.zeros((ch, cw, 4), np.float32)
    g1, g2 = np.zeros((ch, cw), rt4.GBUFFER_DTYPE), np.zeros((H, W), rt4.GBUFFER_DTYPE)
    with pytest.raises(rt4.RT4Error):
        tracer_lut.upscale_host(u, s, cells, None, g2)
    with pytest.raises(rt4.RT4Error):
        tracer_lut.upscale_host(u, 0, cells, g1, g2, out=np.zeros((H, W, 4), np.float32))
    with pytest.raises(rt4.RT4Error):
        tracer_lut.upscale_host(u, s, cells, g1, g2, out=np.zeros((H, W - 1, 4), np.float32))
    # rt4_window's
    with pytest.raises(rt4.RT4Error):
        rt4.Window(tracer_lut, cw, ch, 65)
    with pytest.raises(rt4.RT4Error):
        rt4.Window(tracer_lut, 1024, 16, 64)
    with pytest.raises(rt4.RT4Error):
        rt4.Window(tracer_lut, cw, ch, s, 9)
    win = rt4.Window(tracer_lut, cw, ch, s)
    try:
        with pytest.raises(rt4.RT4Error):
            win.present(rt4.make_uniforms(cw + 1, ch, 1, 1), c)
        with pytest.raises(rt4.RT4Error):
            win.present(u, 0)
    finally:
        win.close()


# ------------------------------------------------------------------------------------------ 7. rt4_window
def moved(rt4, u, dx):
    focus = list(u.focus)
    focus[0] = float(np.float32(focus[0] + dx))
    return rt4.make_uniforms(CW, CH, samples=4, reflections=4, seed=12345, focus=tuple(focus))


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_window_equals_the_stateless_calls(rt4, tracer_lut, rendered, fmt):
    import torch

    s = 4
    W, H = CW * s, CH * s
    r = rendered["sphere"]
    u, cells = r["u"], r["frames"][fmt]
    sphere, other = rt4.Scene.named("sphere"), rt4.Scene.named("all_primitives")
    tracer_lut.set_scene(sphere)
    dc = to_gpu(cells)
    win = rt4.Window(tracer_lut, CW, CH, s, fmt)
    try:
        assert (win.w, win.h) == (W, H)
        assert win.bytes() == W * H * (np.dtype(DT[fmt]).itemsize * 4 + 32) + CW * CH * 32
        # NEAREST renders nothing: the window G-buffer keeps the zeros of its creation
        win.present(u, dc.data_ptr(), params=rt4.upscale_params(mode=NEAREST))
        assert raw(win.image()) == raw(upscale_ref.nearest(cells, s)) and not raw(win.gbuffer()).strip(b"\0")
        # the first guided present renders both G-buffers
        gw = window_gbuffer(rt4, tracer_lut, u, s)
        want = tracer_lut.upscale_host(u, s, cells, r["g"], gw)
        win.present(u, dc.data_ptr())
        assert raw(win.gbuffer()) == raw(gw) and raw(win.image()) == raw(want)
        # a resting camera renders none: with another scene in the context and no reset, the G-buffers stay the sphere's
        tracer_lut.set_scene(other)
        win.present(rt4.Uniforms.from_buffer_copy(bytes(u)), dc.data_ptr(), CW, 0, CW, rt4.upscale_params(),
                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert raw(win.gbuffer()) == raw(gw) and raw(win.image()) == raw(want)
        # seed, samples and part are not the pose
        u_seed = rt4.Uniforms.from_buffer_copy(bytes(u))
        u_seed.seed, u_seed.samples, u_seed.part = 7, 1, 0.5
        win.present(u_seed, dc.data_ptr())
        assert raw(win.gbuffer()) == raw(gw) and raw(win.image()) == raw(want)
        # reset after set_scene: the other scene's G-buffers
        win.reset()
        win.present(u, dc.data_ptr())
        gw_o = window_gbuffer(rt4, tracer_lut, u, s)
        gc_o = tracer_lut.render_gbuffer_host(u, rt4.region(CW, CH))
        assert raw(gw_o) != raw(gw)
        assert raw(win.gbuffer()) == raw(gw_o) and raw(win.image()) == raw(tracer_lut.upscale_host(u, s, cells, gc_o, gw_o))
        # a changed pose re-renders
        tracer_lut.set_scene(sphere)
        win.reset()
        win.present(u, dc.data_ptr())
        um = moved(rt4, u, 0.3)
        win.present(um, dc.data_ptr())
        gw_m = window_gbuffer(rt4, tracer_lut, um, s)
        gc_m = tracer_lut.render_gbuffer_host(um, rt4.region(CW, CH))
        assert raw(gw_m) != raw(gw) and raw(win.gbuffer()) == raw(gw_m)
        assert raw(win.image()) == raw(tracer_lut.upscale_host(um, s, cells, gc_m, gw_m))
        # the caller's cell G-buffer instead of the owned one, then the owned one at the same pose
        dg = to_gpu(r["g"])  # the G-buffer of u, not of um: the result must use it
        win.present(um, dc.data_ptr(), gcells_ptr=dg.data_ptr())
        assert raw(win.image()) == raw(tracer_lut.upscale_host(um, s, cells, r["g"], gw_m))
        win.present(um, dc.data_ptr())
        assert raw(win.image()) == raw(tracer_lut.upscale_host(um, s, cells, gc_m, gw_m))
    finally:
        win.close()
        tracer_lut.set_scene(sphere)


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_window_composes_with_temporal_and_denoise(rt4, tracer_lut, fmt):
    """A moving temporal image presented through its own G-buffer, and the filtered image of the same frame: both
    equal the stateless upscale of what was read back."""
    import torch

    s = 3
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    base = rt4.make_uniforms(CW, CH, samples=2, reflections=4, seed=99)
    t = rt4.Temporal(tracer_lut, CW, CH, fmt)
    win = rt4.Window(tracer_lut, CW, CH, s, fmt)
    try:
        for n in range(1, 4):
            u = rt4.progressive_uniforms(moved(rt4, base, 0.05 * (n // 2)), n)
            t.frame(u)
            win.present(u, t.image_ptr(), CW, t.gbuffer_ptr(), CW)
            image, g = t.image(), t.gbuffer()
            gw = window_gbuffer(rt4, tracer_lut, u, s)
            assert raw(win.gbuffer()) == raw(gw), n
            assert raw(win.image()) == raw(tracer_lut.upscale_host(u, s, image, g, gw)), n
        # filter at cell resolution, then present the filtered frame
        dn = torch.zeros(image.nbytes, dtype=torch.uint8, device="cuda")
        tracer_lut.denoise_device(t.image_ptr(), CW, dn.data_ptr(), CW, fmt, CW, CH, t.gbuffer_ptr(), CW, rt4.denoise_params(levels=2))
        win.present(u, dn.data_ptr(), CW, t.gbuffer_ptr(), CW)
        filtered = tracer_lut.denoise_host(image, g, rt4.denoise_params(levels=2))
        assert raw(filtered) != raw(image)
        assert raw(win.image()) == raw(tracer_lut.upscale_host(u, s, filtered, g, gw))
        assert raw(win.image()) == raw(upscale_ref.upscale(u, s, filtered, g, gw))
    finally:
        win.close()
        t.close()


# ------------------------------------------------------------------------------------------ 8. rt4_render --window
def render_paths(rt4):
    lib_dir = os.path.dirname(rt4.LIB_PATH)
    return os.path.join(lib_dir, "rt4_render"), os.path.join(lib_dir, "..", "..", "properties.txt")


def ppm_size(path):
    with open(path, "rb") as f:
        assert f.readline() == b"P6\n"
        w, h = f.readline().split()
    return int(w), int(h)


def frame_seed(seed, n):
    return seed ^ ((n * 0x9E3779B9) & 0xFFFFFFFF)


def test_cpp_host_window_one_section(rt4, tracer_lut, tmp_path):
    """rt4_render --window on one section of 24 x 16 cells: plain, --window-nearest and --denoise; every _win image has
    the window's size and equals the same steps from Python."""
    import torch

    exe, props_path = render_paths(rt4)
    w, h, seed, frames, s = CW, CH, 4321, 3, 4
    common = [exe, "-p", props_path, "-s", "sphere", "-n", str(frames), "-W", str(w), "-H", str(h), "--seed", str(seed)]

    def run(tag, extra):
        pre = str(tmp_path / tag)
        r = subprocess.run(common + ["-o", pre] + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return pre

    guided, nearest, dn = run("g", ["--window", str(s)]), run("n", ["--window", str(s), "--window-nearest"]), \
        run("d", ["--denoise", "2", "--window", "3"])
    # the same frames from Python
    props = rt4.Properties(path=props_path)
    base = rt4.uniforms_from_properties(props, w, h)
    cam = rt4.Camera(props)
    tracer_lut.set_scene(rt4.Scene.builtin("sphere"))
    us = [cam.frame_uniforms(base, rt4.SECTION_YXZ, frame_seed(seed, n)) for n in range(1, frames + 1)]
    frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
    tracer_lut.render_frames_device(us, rt4.region(w, h), frame.data_ptr(), 0, w, 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    cells = frame.cpu().numpy()
    g = tracer_lut.render_gbuffer_host(us[-1], rt4.region(w, h))
    filtered = tracer_lut.denoise_host(cells, g, rt4.denoise_params(levels=2))
    dfilt = to_gpu(filtered)

    def same(image, path, size):
        py = str(tmp_path / "py.ppm")
        rt4.write_ppm(py, image)
        assert ppm_size(path) == size, path
        assert open(py, "rb").read() == open(path, "rb").read(), path

    win = rt4.Window(tracer_lut, w, h, s, 0)
    try:
        same(cells, guided + "_yxz.ppm", (w, h))
        win.present(us[-1], frame.data_ptr())
        same(win.image(), guided + "_yxz_win.ppm", (w * s, h * s))
        win.present(us[-1], frame.data_ptr(), params=rt4.upscale_params(mode=NEAREST))
        same(win.image(), nearest + "_yxz_win.ppm", (w * s, h * s))
        assert open(guided + "_yxz_win.ppm", "rb").read() != open(nearest + "_yxz_win.ppm", "rb").read()
    finally:
        win.close()
    win = rt4.Window(tracer_lut, w, h, 3, 0)
    try:
        same(filtered, dn + "_yxz_dn.ppm", (w, h))
        win.present(us[-1], dfilt.data_ptr())
        same(win.image(), dn + "_yxz_win.ppm", (w * 3, h * 3))
    finally:
        win.close()
    # refused combinations name the flag
    for extra in (["--window", "--gpus", "2"], ["--window", "0"], ["--window", "65"]):
        r = subprocess.run([exe, "-p", props_path, "-s", "sphere", "-W", "16", "-H", "8"] + extra, capture_output=True,
                           text=True, timeout=60)
        assert r.returncode != 0 and "--window" in r.stderr, extra


@pytest.mark.parametrize("extra", [[], ["--reproject", "--denoise", "2"]], ids=["plain", "reproject-denoise"])
def test_cpp_host_window_three_sections(rt4, tracer_lut, tmp_path, extra):
    """rt4_render -3 --window with a moving camera and the properties' sizes: every section's window image has
    cells * cell_size pixels (main for YXZ, additional for the others) and equals the same steps from Python; with
    --reproject --denoise the temporal image is filtered with the temporal G-buffer, then upscaled with it."""
    import torch

    exe, props_path = render_paths(rt4)
    pre, seed, frames = str(tmp_path / "s"), 99, 3
    r = subprocess.run([exe, "-p", props_path, "-s", "tiger", "-n", str(frames), "-3", "--seed", str(seed), "--keys", "W",
                        "--move-seconds", "0.02", "--window", "-o", pre] + extra, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    props = rt4.Properties(path=props_path)
    tracer_lut.set_scene(rt4.Scene.builtin("tiger"))
    sections = [(rt4.SECTION_YXZ, "yxz", "main"), (rt4.SECTION_YWZ, "ywz", "additional"), (rt4.SECTION_YXW, "yxw", "additional")]
    for sec, tag, window in sections:
        w, h = rt4.window_cells(props, window)
        s = props.getInt(f"window.{window}.cell_size")
        base = rt4.uniforms_from_properties(props, w, h, sec)
        cam = rt4.Camera(props)
        t = rt4.Temporal(tracer_lut, w, h, 0) if extra else None
        win = rt4.Window(tracer_lut, w, h, s, 0)
        frame = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        try:
            for n in range(1, frames + 1):
                u = cam.frame_uniforms(base, sec, frame_seed(seed, n))
                if t is not None:
                    t.frame(u)
                else:
                    tracer_lut.render_device_ex(u, rt4.region(w, h), frame.data_ptr(), 0, w)
                cam.move(rt4.KEY_FORWARD, 0.02)
            if t is not None:
                dn = torch.zeros(h * w * 16, dtype=torch.uint8, device="cuda")
                tracer_lut.denoise_device(t.image_ptr(), w, dn.data_ptr(), w, 0, w, h, t.gbuffer_ptr(), w, rt4.denoise_params(levels=2))
                win.present(u, dn.data_ptr(), w, t.gbuffer_ptr(), w)
            else:
                win.present(u, frame.data_ptr())
            image = win.image()
        finally:
            win.close()
            if t is not None:
                t.close()
        py = str(tmp_path / f"py_{tag}.ppm")
        rt4.write_ppm(py, image)
        assert ppm_size(f"{pre}_{tag}_win.ppm") == (w * s, h * s), tag
        assert open(py, "rb").read() == open(f"{pre}_{tag}_win.ppm", "rb").read(), tag


# ------------------------------------------------------------------------------------------ 9. it helps
def test_guided_is_closer_to_the_window_resolution_image(rt4, tracer_lut):
    """Sphere, 40 x 24 cells, scale 4: 64 progressive 4-spp frames at cell resolution presented guided and nearest,
    against 64 progressive frames rendered at 160 x 96 (another seed). No tolerance: guided must be closer, over all
    pixels and over the edge pixels (window pixels whose surface is not their own cell's)."""
    import torch

    cw, ch, s, frames = 40, 24, 4, 64
    W, H = cw * s, ch * s
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    stream = torch.cuda.current_stream().cuda_stream

    def progressive(w, h, seed):
        img = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda")
        base = rt4.make_uniforms(w, h, samples=4, reflections=4, seed=seed)
        tracer_lut.render_frames_device([rt4.progressive_uniforms(base, n) for n in range(1, frames + 1)], rt4.region(w, h),
                                        img.data_ptr(), 0, w, 0, stream)
        torch.cuda.synchronize()
        return base, img

    u, cells = progressive(cw, ch, 4242)
    _, truth = progressive(W, H, 777)
    truth = truth.cpu().numpy()[..., :3].astype(np.float64)
    win = rt4.Window(tracer_lut, cw, ch, s, 0)
    try:
        win.present(u, cells.data_ptr())
        guided, gw = win.image(), win.gbuffer()
        win.present(u, cells.data_ptr(), params=rt4.upscale_params(mode=NEAREST))
        near = win.image()
    finally:
        win.close()
    gc = tracer_lut.render_gbuffer_host(u, rt4.region(cw, ch))
    edge = gw["surface"] != upscale_ref.nearest(gc["surface"], s)
    assert edge.sum() > 100
    eg = ((guided[..., :3] - truth) ** 2).mean(axis=2)
    en = ((near[..., :3] - truth) ** 2).mean(axis=2)
    print(f"MSE against the window-resolution image: guided {eg.mean():.3e}, nearest {en.mean():.3e}; "
          f"on {edge.sum()} edge pixels: guided {eg[edge].mean():.3e}, nearest {en[edge].mean():.3e}")
    assert eg.mean() < en.mean()
    assert eg[edge].mean() < en[edge].mean()
