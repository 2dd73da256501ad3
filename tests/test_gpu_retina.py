"""The 3D retina view on the GPU (rt4.h rt4_retina_voxelize_device, rt4_retina_project_device, rt4_retina; rt4_render
--retina): the slices of an accumulated volume against the stateless renders they are made of, the two kernels against
their definition restated in numpy (retina_ref) bit for bit, host against device, the argument errors, the stateful
object against the stateless calls, and the command-line tool against the library path."""
import glob
import math
import os
import subprocess

import numpy as np
import pytest

import retina_ref
from denoise_ref import F32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
DT = {0: np.float32, 1: np.float16, 2: np.uint8}
FMT_IDS = ["f32", "f16", "rgba8"]
SIZES = [(16, 12, 5), (24, 16, 7)]
SAMPLES, BOUNCES, SEED = 2, 3, 4242


def raw(a):
    return np.ascontiguousarray(a).tobytes()


def same_bits(a, b):
    """Equal bit for bit, but a NaN matches any NaN (its payload is not defined)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype.kind != "f":
        return raw(a) == raw(b)
    nan = np.isnan(a)
    u = {2: np.uint16, 4: np.uint32}[a.dtype.itemsize]
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(u)[~nan], b.view(u)[~nan])


def view_of(rt4, w, h):
    """(u, w_drct, depth_size) of the default camera at w x h cells."""
    u = rt4.make_uniforms(w, h, samples=SAMPLES, reflections=BOUNCES, seed=SEED)
    return u, rt4.Orientation(0.0, 0.0, 0.0).w_drct, float(u.mtr_sizes[1])


@pytest.fixture(scope="module")
def volumes(rt4, tracer_lut):
    """{(scene, (w, h, d)): dict(u, w_drct, ds, light, gbuf)}: volumes accumulated once through rt4.Retina, 3 frames for
    the small sphere volume (the slices test takes it apart), 1 frame for the others."""
    out = {}
    for name in ("sphere", "all_primitives"):
        tracer_lut.set_scene(rt4.Scene.named(name))
        for (w, h, d) in SIZES:
            u, w_drct, ds = view_of(rt4, w, h)
            ret = rt4.Retina(tracer_lut, w, h, d)
            try:
                ret.accumulate(u, w_drct, ds, 3 if (name, w) == ("sphere", 16) else 1)
                out[(name, (w, h, d))] = dict(u=u, w_drct=w_drct, ds=ds, light=ret.light(), gbuf=ret.gbuffer(),
                                              frames=ret.frames_done())
            finally:
                ret.close()
    return out


# ------------------------------------------------------------------------------------------------------- 1. slices
def test_slices_are_the_stateless_renders(rt4, tracer_lut, volumes):
    w, h, d = SIZES[0]
    vol = volumes[("sphere", SIZES[0])]
    u, w_drct, ds = vol["u"], vol["w_drct"], vol["ds"]
    assert vol["frames"] == 3
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    reg = rt4.region(w, h)
    for s in range(d):
        su = rt4.retina_slice_uniforms(u, w_drct, d, ds, s)
        us = [rt4.progressive_uniforms(su, n) for n in (1, 2, 3)]
        light, _ = tracer_lut.render_light_host(us, reg)
        assert raw(vol["light"][s]) == raw(light), s
        assert raw(vol["gbuf"][s]) == raw(tracer_lut.render_gbuffer_host(su, reg)), s
    # the middle slice is the plain section
    plain, _ = tracer_lut.render_light_host([rt4.progressive_uniforms(u, n) for n in (1, 2, 3)], reg)
    assert raw(vol["light"][2]) == raw(plain)
    assert len({raw(vol["light"][s]) for s in range(d)}) == d  # and the slices differ
    # 1 + 2 frames are 3 frames
    ret = rt4.Retina(tracer_lut, w, h, d)
    try:
        assert ret.bytes() == w * h * d * (32 + 32 + 16) and ret.frames_done() == 0
        ret.accumulate(u, w_drct, ds, 1)
        assert ret.frames_done() == 1
        ret.accumulate(u, w_drct, ds, 2)
        assert ret.frames_done() == 3
        assert raw(ret.light()) == raw(vol["light"]) and raw(ret.gbuffer()) == raw(vol["gbuf"])
    finally:
        ret.close()


# ----------------------------------------------------------------------------------------------------- 2. voxelize
@pytest.mark.parametrize("size", SIZES, ids=["16x12x5", "24x16x7"])
@pytest.mark.parametrize("scene", ["sphere", "all_primitives"])
def test_voxelize_rendered_volumes(rt4, tracer_lut, volumes, scene, size):
    vol = volumes[(scene, size)]
    k = float(vol["u"].light_to_color_conversion_coefficient)
    for alphas in ((0.0, 1 / 32, 0.5), (0.125, 0.75, 1.0)):
        want, plan = retina_ref.voxelize(vol["light"], vol["gbuf"], k, *alphas)
        got = tracer_lut.retina_voxelize_host(vol["light"], vol["gbuf"], k,
                                              rt4.retina_params(alpha_sky=alphas[0], alpha_fill=alphas[1], alpha_edge=alphas[2]))
        assert same_bits(got, want)
    # no case is vacuous
    assert plan["edge"] > 0 and plan["fill"] > 0 and plan["surfaces"] >= 2, plan
    if scene == "sphere":
        assert plan["sky"] > 0, plan
    assert plan["edge"] + plan["fill"] + plan["sky"] == size[0] * size[1] * size[2]


@pytest.mark.parametrize("w,h,d", [(1, 1, 1), (1, 5, 1), (33, 9, 2)], ids=["1x1x1", "1x5x1", "33x9x2"])
def test_voxelize_synthetic_volumes(rt4, tracer_lut, w, h, d):
    rng = np.random.default_rng(w * 100 + h)
    rows, stride = h + 2, w + 3  # padded rows and slices
    light = np.zeros((d, rows, stride), rt4.LIGHT_DTYPE)
    gbuf = np.zeros((d, rows, stride), rt4.GBUFFER_DTYPE)
    light["mean"] = rng.random((d, rows, stride, 3), dtype=F32) * 4
    light["n"] = rng.integers(0, 3, (d, rows, stride))  # a third of the voxels empty
    special = np.array([np.nan, np.inf, -np.inf, -1.0, -0.5, 0.0], F32)
    pick = rng.random((d, rows, stride, 3)) < 0.2
    light["mean"][pick] = rng.choice(special, int(pick.sum()))
    # surfaces (-1, the sky, among them) in blocks of 3 x 6 through all slices, so that some voxels have no other
    # surface next to them, with one voxel in ten sprinkled at random
    blocks = rng.integers(-1, 3, (rows // 3 + 1, stride // 6 + 1))
    surface = np.broadcast_to(blocks[np.arange(rows)[:, None] // 3, np.arange(stride)[None, :] // 6], (d, rows, stride)).copy()
    sprinkle = rng.random((d, rows, stride)) < 0.1
    surface[sprinkle] = rng.integers(-1, 3, int(sprinkle.sum()))
    gbuf["surface"] = surface
    # what the padding holds must not matter: another surface there would make edges of the image's last voxels
    gbuf["surface"][:, h:, :] = 77
    gbuf["surface"][:, :, w:] = 78
    out = np.full((d, rows, stride, 4), -7.25, F32)  # the sentinel
    p = rt4.retina_params(alpha_sky=0.25, alpha_fill=0.5, alpha_edge=1.0)
    got = tracer_lut.retina_voxelize_host(light, gbuf, 1.5, p, out=out, w=w, h=h)
    want, plan = retina_ref.voxelize(light[:, :h, :w], gbuf[:, :h, :w], 1.5, 0.25, 0.5, 1.0)
    assert same_bits(got[:, :h, :w], want)
    pad = np.ones((d, rows, stride), bool)
    pad[:, :h, :w] = False
    assert (got[pad] == F32(-7.25)).all()
    if (w, h, d) == (33, 9, 2):
        assert plan["edge"] > 0 and plan["fill"] > 0 and plan["sky"] > 0
    if (w, h, d) == (1, 1, 1):
        assert plan["edge"] == 0  # no neighbour inside the volume


# ------------------------------------------------------------------------------------------------------ 3. project
OW_OH = [(1, 1), (33, 9), (40, 24)]
VIEWS = ["identity", "yaw30_pitch20", "yaw90", "yaw180", "inside", "far"]
T_CUT = 0.5


def make_view(rt4, name, size, box, ow, oh, step=1.0):
    w, h, d = size
    yaw, pitch, extent = {"identity": (0.0, 0.0, box[0]), "yaw30_pitch20": (math.radians(30), math.radians(20), 0.0),
                          "yaw90": (math.pi / 2, 0.0, 0.0), "yaw180": (math.pi, 0.0, box[0]),
                          "inside": (0.0, 0.0, 0.5 * box[0]),  # half the box: every ray inside it all the way
                          "far": (math.radians(30), math.radians(20), 2.0 * math.sqrt(sum(s * s for s in box)))}[name]
    return rt4.retina_view(w, h, d, box, yaw, pitch, extent, ow, oh, step)


def project_cases(name):
    """(ow, oh, step_voxels, t_min) of a view: every picture size at step 1, the other steps and the cut at 40 x 24."""
    return [(ow, oh, 1.0, 0.0) for (ow, oh) in OW_OH] + [(40, 24, 0.5, 0.0), (40, 24, 2.0, 0.0), (40, 24, 1.0, T_CUT)]


@pytest.fixture(scope="module")
def projections(rt4, volumes):
    """The voxel volume of the 24 x 16 x 7 all_primitives retina (the restatement's, which test_voxelize_rendered_volumes
    holds the kernel to) and, for every view and case, the restatement's colours and plan: computed once."""
    size = SIZES[1]
    vol = volumes[("all_primitives", size)]
    u = vol["u"]
    V, _ = retina_ref.voxelize(vol["light"], vol["gbuf"], float(u.light_to_color_conversion_coefficient), 0.0, 1 / 32, 0.5)
    box = (float(u.mtr_sizes[0]), float(u.mtr_sizes[1]), vol["ds"])
    bg = (0.25, 0.5, 0.75)
    ref = {}
    for name in VIEWS:
        for (ow, oh, step, t_min) in project_cases(name):
            view = make_view(rt4, name, size, box, ow, oh, step)
            ref[(name, ow, oh, step, t_min)] = (view,) + retina_ref.project_colours(V, view, ow, oh, t_min, bg)
    return dict(V=V, size=size, box=box, bg=bg, ref=ref)


@pytest.mark.parametrize("name", VIEWS)
def test_project_matches_the_restatement(rt4, tracer_lut, projections, name):
    V, bg = projections["V"], projections["bg"]
    for (ow, oh, step, t_min) in project_cases(name):
        view, colours, plan = projections["ref"][(name, ow, oh, step, t_min)]
        p = rt4.retina_params(t_min=t_min, background=bg)
        for fmt in (0, 1, 2):
            got = tracer_lut.retina_project_host(V, view, ow, oh, p, fmt)
            assert same_bits(got, retina_ref.store(colours, DT[fmt])), (name, ow, oh, step, t_min, fmt)


def test_project_plans_cover_the_cases(projections):
    ref = projections["ref"]
    total = lambda key, sel=lambda k: True: sum(ref[k][2][key] for k in ref if sel(k))
    assert total("inside") > 0 and total("partly") > 0 and total("outside") > 0
    assert total("never_entered") > 0 and total("never_entered", lambda k: k[0] == "far") > 0
    assert total("never_entered", lambda k: k[0] == "inside") == 0 and total("outside", lambda k: k[0] == "inside") == 0
    cut = lambda k: k[4] == T_CUT
    assert total("stopped", cut) > 0 and total("ran_out", cut) > 0
    assert total("stopped", lambda k: k[4] == 0.0) == 0  # t_min 0 stops no ray
    for name in VIEWS:  # every view shows something: its pictures are not the background alone
        view, colours, plan = ref[(name, 40, 24, 1.0, 0.0)]
        assert plan["inside"] + plan["partly"] > 0 and not (colours == np.array(projections["bg"], F32)).all(), name
    # the steps: half the step, twice the samples
    assert ref[("identity", 40, 24, 0.5, 0.0)][0].steps == 2 * ref[("identity", 40, 24, 1.0, 0.0)][0].steps


@pytest.mark.parametrize("fmt", [0, 1, 2], ids=FMT_IDS)
def test_project_views_that_see_nothing_give_the_background(rt4, tracer_lut, projections, fmt):
    V, bg = projections["V"], projections["bg"]
    want = retina_ref.store(np.broadcast_to(np.array(bg, F32), (9, 33, 3)).copy(), DT[fmt])
    views = dict(nan_origin=rt4.RetinaView((float("nan"),) * 3, (24.0, 0.0, 0.0), (0.0, -16.0, 0.0), (0.0, 0.0, 1.0), 7),
                 one_nan=rt4.RetinaView((12.0, float("nan"), -0.5), (24.0, 0.0, 0.0), (0.0, -16.0, 0.0), (0.0, 0.0, 1.0), 7),
                 miss=rt4.RetinaView((60.0, 8.0, -0.5), (24.0, 0.0, 0.0), (0.0, -16.0, 0.0), (0.0, 0.0, 1.0), 4096),
                 away=rt4.RetinaView((12.0, 8.0, -2.0), (24.0, 0.0, 0.0), (0.0, -16.0, 0.0), (0.0, 0.0, -1.0), 50),
                 inf_step=rt4.RetinaView((12.0, 8.0, -0.5), (24.0, 0.0, 0.0), (0.0, -16.0, 0.0), (0.0, 0.0, float("inf")), 9))
    p = rt4.retina_params(background=bg)
    for name, view in views.items():
        got = tracer_lut.retina_project_host(V, view, 33, 9, p, fmt)
        assert raw(got) == raw(want), name
        if view.steps <= 64:  # the restatement agrees (it walks every step: not the 4096 of `miss`)
            ref, plan = retina_ref.project(V, view, 33, 9, background=bg, dtype=DT[fmt])
            assert raw(ref) == raw(want) and plan["never_entered"] == 33 * 9, name


def test_project_hand_made_views_and_padded_volumes(rt4, tracer_lut, projections):
    """Views the helper does not make (sheared, non-uniform steps, rays that start inside and leave through a side) on a
    volume with padded rows and slices, into a frame with padded rows whose padding keeps its bytes."""
    V, bg = projections["V"], projections["bg"]
    d, h, w = V.shape[:3]
    padded = np.full((d, h + 1, w + 5, 4), 9.0, F32)  # the padding is opaque and bright: a load that strays shows
    padded[:, :h, :w] = V
    views = [rt4.RetinaView((11.3, 7.7, 2.2), (30.0, 3.0, 1.0), (2.0, -20.0, 0.5), (0.37, -0.21, 0.11), 90),
             rt4.RetinaView((-3.0, 20.0, 8.0), (9.0, 0.0, 0.0), (0.0, -9.0, 0.0), (0.9, -1.1, -0.4), 40),
             rt4.RetinaView((5.0, 5.0, 3.0), (24.0, 0.0, 0.0), (0.0, -16.0, 0.0), (0.0, 0.0, 0.0), 3)]
    p = rt4.retina_params(t_min=1 / 256, background=bg)
    for q, view in enumerate(views):
        want, plan = retina_ref.project(V, view, 33, 9, t_min=1 / 256, background=bg)
        assert plan["inside"] > 0, q
        out = np.full((9, 36, 4), -3.5, F32)
        got = tracer_lut.retina_project_host(padded, view, 33, 9, p, 0, out=out, w=w, h=h)
        assert same_bits(got[:, :33], want) and (got[:, 33:] == F32(-3.5)).all(), q


# -------------------------------------------------------------------------- 4. host against device, argument errors
def to_gpu(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def test_host_equals_device(rt4, tracer_lut, volumes, projections):
    import torch

    size = SIZES[1]
    w, h, d = size
    vol = volumes[("all_primitives", size)]
    k = float(vol["u"].light_to_color_conversion_coefficient)
    stream = torch.cuda.current_stream().cuda_stream
    dl, dg = to_gpu(vol["light"]), to_gpu(vol["gbuf"])
    dv = torch.zeros(w * h * d * 16, dtype=torch.uint8, device="cuda")
    p = rt4.retina_params(t_min=1 / 256, background=projections["bg"])
    tracer_lut.retina_voxelize_device(dl.data_ptr(), (w, w * h), dg.data_ptr(), (w, w * h), k, p, dv.data_ptr(), (w, w * h), w, h, d,
                                      stream)
    torch.cuda.synchronize()
    host_v = tracer_lut.retina_voxelize_host(vol["light"], vol["gbuf"], k, p)
    assert dv.cpu().numpy().tobytes() == raw(host_v)
    view = make_view(rt4, "yaw30_pitch20", size, projections["box"], 40, 24)
    for fmt in (0, 1, 2):
        host = tracer_lut.retina_project_host(host_v, view, 40, 24, p, fmt)
        out = torch.zeros(host.nbytes, dtype=torch.uint8, device="cuda")
        tracer_lut.retina_project_device(dv.data_ptr(), (w, w * h), w, h, d, view, p, out.data_ptr(), fmt, 40, 40, 24, stream)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == raw(host), fmt


def test_argument_errors_write_nothing(rt4, tracer_lut):
    import torch

    w, h, d, ow, oh = 8, 4, 3, 10, 6
    n = w * h * d
    # one buffer of 16-B units: light 2n, G-buffer 2n, voxels n, frame ow*oh (fp32)
    buf = torch.full((5 * n + ow * oh, 4), 0.25, dtype=torch.float32, device="cuda")
    before = buf.cpu().numpy().copy()
    stream = torch.cuda.current_stream().cuda_stream
    p0 = buf.data_ptr()
    L, G, V, Fr = p0, p0 + 32 * n, p0 + 64 * n, p0 + 80 * n
    ok = rt4.retina_params()
    st = (w, w * h)
    view = rt4.RetinaView((3.5, 1.5, -0.5), (8.0, 0.0, 0.0), (0.0, -4.0, 0.0), (0.0, 0.0, 1.0), 3)

    def status(f, *a):
        try:
            f(*a)
        except rt4.RT4Error as e:
            return e.status
        return 0

    def vox(L=L, G=G, V=V, p=ok, ls=st, gs=st, vs=st, ww=w, hh=h, dd=d):
        return status(tracer_lut.retina_voxelize_device, L, ls, G, gs, 1.0, p, V, vs, ww, hh, dd, stream)

    def proj(V=V, Fr=Fr, p=ok, vs=st, ww=w, hh=h, dd=d, vw=view, fmt=0, fs=ow, oww=ow, ohh=oh):
        return status(tracer_lut.retina_project_device, V, vs, ww, hh, dd, vw, p, Fr, fmt, fs, oww, ohh, stream)

    for name in ("L", "G", "V"):
        assert vox(**{name: 0}) == ERR_ARG, name  # null pointers
    assert proj(V=0) == ERR_ARG and proj(Fr=0) == ERR_ARG and proj(vw=None) == ERR_ARG
    assert vox(L=L + 4) == ERR_ARG and vox(G=G + 8) == ERR_ARG and vox(V=V + 4) == ERR_ARG  # volumes 16 B
    assert proj(V=V + 8) == ERR_ARG and proj(Fr=Fr + 4) == ERR_ARG  # fp32 frame 16 B
    assert proj(Fr=Fr + 4, fmt=1) == ERR_ARG and proj(Fr=Fr + 2, fmt=2) == ERR_ARG  # half 8 B, RGBA8 4 B
    assert proj(fmt=3) == ERR_ARG and proj(fmt=-1) == ERR_ARG
    # overlaps: the voxel volume with each input by one voxel, the frame with the volume by one pixel, in place
    assert vox(V=L + 32 * n - 16) == ERR_ARG and vox(V=G + 32 * n - 16) == ERR_ARG and vox(V=L) == ERR_ARG and vox(L=V) == ERR_ARG
    assert proj(Fr=V + 16 * n - 16) == ERR_ARG and proj(Fr=V) == ERR_ARG and proj(V=Fr + 16 * ow * oh - 16) == ERR_ARG
    # strides too small: row below the width, slice below a slice
    for name in ("ls", "gs", "vs"):
        assert vox(**{name: (w - 1, w * h)}) == ERR_ARG and vox(**{name: (w, w * h - 1)}) == ERR_ARG, name
    assert proj(vs=(w - 1, w * h)) == ERR_ARG and proj(vs=(w, w * h - 1)) == ERR_ARG and proj(fs=ow - 1) == ERR_ARG
    # sizes
    assert vox(dd=0) == ERR_ARG and vox(dd=257) == ERR_ARG and proj(dd=0) == ERR_ARG and proj(dd=257) == ERR_ARG
    assert vox(ww=0) == ERR_ARG and vox(hh=0) == ERR_ARG and proj(ww=0) == ERR_ARG and proj(hh=65536) == ERR_ARG
    assert proj(oww=0) == ERR_ARG and proj(ohh=0) == ERR_ARG and proj(oww=65536, fs=65536) == ERR_ARG
    # parameters: alphas in [0, 1], t_min in [0, 1), NaN in neither; both calls check all four
    for kw in (dict(alpha_sky=-0.01), dict(alpha_fill=1.5), dict(alpha_edge=float("nan")), dict(alpha_sky=float("inf")),
               dict(t_min=1.0), dict(t_min=-0.1), dict(t_min=float("nan"))):
        assert vox(p=rt4.retina_params(**kw)) == ERR_ARG and proj(p=rt4.retina_params(**kw)) == ERR_ARG, kw
    for steps in (0, 4097, -1):
        assert proj(vw=rt4.RetinaView((3.5, 1.5, -0.5), (8.0, 0.0, 0.0), (0.0, -4.0, 0.0), (0.0, 0.0, 1.0), steps)) == ERR_ARG
    torch.cuda.synchronize()
    assert raw(buf.cpu().numpy()) == raw(before)  # nothing was written
    # and the same buffers, adjacent but not overlapping, are accepted: voxels and frame are written, the inputs are not
    assert vox() == 0 and proj(vw=rt4.RetinaView((3.5, 1.5, -0.5), (8.0, 0.0, 0.0), (0.0, -4.0, 0.0), (0.0, 0.0, 1.0), 4096)) == 0
    torch.cuda.synchronize()
    after = buf.cpu().numpy()
    assert raw(after[:4 * n]) == raw(before[:4 * n]) and not (after[4 * n:] == 0.25).any()
    # the host variants' own checks, with sentinel-filled outputs
    light, gbuf = np.zeros((d, h, w), rt4.LIGHT_DTYPE), np.zeros((d, h, w), rt4.GBUFFER_DTYPE)
    out = np.full((d, h, w, 4), -7.0, F32)
    frame = np.full((oh, ow, 4), -7.0, F32)
    for call in (lambda: tracer_lut.retina_voxelize_host(light, gbuf, 1.0, rt4.retina_params(alpha_fill=2.0), out=out),
                 lambda: tracer_lut.retina_voxelize_host(light, gbuf, 1.0, ok, out=out, w=w + 1),
                 lambda: tracer_lut.retina_voxelize_host(np.zeros((257, 1, 1), rt4.LIGHT_DTYPE), np.zeros((257, 1, 1), rt4.GBUFFER_DTYPE),
                                                         1.0, ok, out=np.full((257, 1, 1, 4), -7.0, F32)),
                 lambda: tracer_lut.retina_project_host(out, view, ow, oh, rt4.retina_params(t_min=1.0), 0, out=frame),
                 lambda: tracer_lut.retina_project_host(out, view, ow + 1, oh, ok, 0, out=frame),
                 lambda: tracer_lut.retina_project_host(out, rt4.RetinaView(steps=0), ow, oh, ok, 0, out=frame)):
        with pytest.raises(rt4.RT4Error) as e:
            call()
        assert e.value.status == ERR_ARG
    assert (out == -7.0).all() and (frame == -7.0).all()
    # rt4_retina's
    for bad in ((0, 4, 3), (8192, 4, 3), (8, 8192, 3), (8, 4, 0), (8, 4, 257)):
        with pytest.raises(rt4.RT4Error) as e:
            rt4.Retina(tracer_lut, *bad)
        assert e.value.status == ERR_ARG, bad
    ret = rt4.Retina(tracer_lut, w, h, d)
    try:
        u, w_drct, ds = view_of(rt4, w, h)
        with pytest.raises(rt4.RT4Error):  # nothing accumulated yet
            ret.present(view, 1.0, Fr, 0, ow, oh)
        for call in (lambda: ret.accumulate(rt4.make_uniforms(w + 1, h, 1, 1), w_drct, ds, 1),
                     lambda: ret.accumulate(u, w_drct, ds, 0), lambda: ret.accumulate(u, w_drct, 0.0, 1),
                     lambda: ret.accumulate(u, w_drct, float("nan"), 1)):
            with pytest.raises(rt4.RT4Error) as e:
                call()
            assert e.value.status == ERR_ARG
        assert ret.frames_done() == 0
    finally:
        ret.close()


# ---------------------------------------------------------------------------------- 5. stateful against stateless
def test_retina_present_equals_the_stateless_calls(rt4, tracer_lut, volumes):
    import torch

    w, h, d = SIZES[0]
    vol = volumes[("sphere", SIZES[0])]
    u, w_drct, ds = vol["u"], vol["w_drct"], vol["ds"]
    k = float(u.light_to_color_conversion_coefficient)
    box = (float(u.mtr_sizes[0]), float(u.mtr_sizes[1]), ds)
    ow, oh = 40, 24
    view = rt4.retina_view(w, h, d, box, math.radians(30), math.radians(20), 0.0, ow, oh, 1.0)
    stream = torch.cuda.current_stream().cuda_stream
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    ret = rt4.Retina(tracer_lut, w, h, d)

    def shown(fmt, params=None, kk=k, v=view):
        out = torch.zeros(ow * oh * 4 * np.dtype(DT[fmt]).itemsize, dtype=torch.uint8, device="cuda")
        ret.present(v, kk, out.data_ptr(), fmt, ow, oh, params=params, stream=stream)
        torch.cuda.synchronize()
        return out.cpu().numpy().tobytes()

    try:
        ret.accumulate(u, w_drct, ds, 3, stream=stream)
        p = rt4.retina_params()
        vox = tracer_lut.retina_voxelize_host(vol["light"], vol["gbuf"], k, p)
        for fmt in (0, 1, 2):
            assert shown(fmt) == raw(tracer_lut.retina_project_host(vox, view, ow, oh, p, fmt)), fmt
        assert raw(ret.voxels()) == raw(vox)
        # the same parameters do not voxelize again: a voxel overwritten behind the object's back stays overwritten (a
        # 1 x 1 x 1 voxelize of a hit with mean 1 writes (0.75 * 0.5, .., 0.75) over the volume's first voxel)
        one_l, one_g = np.zeros((1, 1, 1), rt4.LIGHT_DTYPE), np.zeros((1, 1, 1), rt4.GBUFFER_DTYPE)
        one_l["mean"], one_l["n"] = 1.0, 1
        dl, dg = to_gpu(one_l), to_gpu(one_g)
        tracer_lut.retina_voxelize_device(dl.data_ptr(), (1, 1), dg.data_ptr(), (1, 1), 1.0, rt4.retina_params(alpha_fill=0.75),
                                          ret.voxels_ptr(), (1, 1), 1, 1, 1, stream)
        marked = vox.copy()
        marked[0, 0, 0] = (0.375, 0.375, 0.375, 0.75)
        other = rt4.retina_view(w, h, d, box, math.radians(200), math.radians(-10), 0.0, ow, oh, 1.0)
        # another view, t_min and background do not voxelize either
        p_bg = rt4.retina_params(t_min=0.25, background=(0.5, 0.5, 0.5))
        assert shown(0, p_bg, v=other) == raw(tracer_lut.retina_project_host(marked, other, ow, oh, p_bg, 0))
        assert raw(ret.voxels()) == raw(marked) and raw(marked) != raw(vox)
        # a changed alpha voxelizes again, and so does a changed k
        p2 = rt4.retina_params(alpha_fill=0.125)
        vox2 = tracer_lut.retina_voxelize_host(vol["light"], vol["gbuf"], k, p2)
        assert shown(0, p2) == raw(tracer_lut.retina_project_host(vox2, view, ow, oh, p2, 0)) and raw(ret.voxels()) == raw(vox2)
        vox3 = tracer_lut.retina_voxelize_host(vol["light"], vol["gbuf"], 2.5, p2)
        assert shown(0, p2, kk=2.5) == raw(tracer_lut.retina_project_host(vox3, view, ow, oh, p2, 0)) and raw(ret.voxels()) == raw(vox3)
        assert raw(vox3) != raw(vox2)
        # more frames voxelize again
        ret.accumulate(u, w_drct, ds, 1, stream=stream)
        assert ret.frames_done() == 4
        shown(0, p2, kk=2.5)
        assert raw(ret.voxels()) == raw(tracer_lut.retina_voxelize_host(ret.light(), ret.gbuffer(), 2.5, p2)) != raw(vox3)
        # a changed camera starts over
        focus = list(u.focus)
        focus[0] = 0.25
        u_moved = rt4.make_uniforms(w, h, samples=SAMPLES, reflections=BOUNCES, seed=SEED, focus=tuple(focus))
        ret.accumulate(u_moved, w_drct, ds, 1, stream=stream)
        assert ret.frames_done() == 1
        su = rt4.retina_slice_uniforms(u_moved, w_drct, d, ds, 0)
        light0, _ = tracer_lut.render_light_host([rt4.progressive_uniforms(su, 1)], rt4.region(w, h))
        assert raw(ret.light()[0]) == raw(light0)
        assert raw(ret.gbuffer()[0]) == raw(tracer_lut.render_gbuffer_host(su, rt4.region(w, h)))
        # so do another depth_size and a reset
        ret.accumulate(u_moved, w_drct, ds, 2, stream=stream)
        assert ret.frames_done() == 3
        ret.accumulate(u_moved, w_drct, 0.5 * ds, 1, stream=stream)
        assert ret.frames_done() == 1
        ret.accumulate(u_moved, w_drct, 0.5 * ds, 1, stream=stream)
        ret.reset()
        assert ret.frames_done() == 0
    finally:
        ret.close()


# ---------------------------------------------------------------------------------------------------------- 6. CLI
def test_render_cli_retina(rt4, tracer_lut, tmp_path):
    exe = os.path.join(os.path.dirname(rt4.LIB_PATH), "rt4_render")
    assert os.path.exists(exe), "lib/rt4_render not built"
    props_path = os.path.join(ROOT, "properties.txt")
    w, h, d, frames = 16, 12, 5, 2
    pre = str(tmp_path / "p")
    common = [exe, "-p", props_path, "-s", "sphere", "-W", str(w), "-H", str(h), "-n", str(frames), "--retina", str(d)]
    r = subprocess.run(common + ["-o", pre], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    assert sorted(os.path.basename(f) for f in glob.glob(pre + "*")) == ["p_yxz_retina.ppm"]
    # the library path
    props = rt4.Properties(props_path)
    scale = props.getInt("window.main.cell_size")
    ow, oh = w * scale, h * scale
    cam = rt4.Camera(props)
    u = cam.frame_uniforms(rt4.uniforms_from_properties(props, w, h), seed=12345)
    w_drct, ds = list(cam.s.orientation.w_drct), float(u.mtr_sizes[1])
    box = (float(u.mtr_sizes[0]), float(u.mtr_sizes[1]), ds)
    k = float(u.light_to_color_conversion_coefficient)
    tracer_lut.set_scene(rt4.Scene.named("sphere"))
    ret = rt4.Retina(tracer_lut, w, h, d)
    try:
        ret.accumulate(u, w_drct, ds, frames)
        vox = tracer_lut.retina_voxelize_host(ret.light(), ret.gbuffer(), k)
    finally:
        ret.close()

    def picture(yaw_deg, pitch_deg, path):
        rad = F32(3.14159265358979323846) / F32(180.0)
        view = rt4.retina_view(w, h, d, box, float(F32(yaw_deg) * rad), float(F32(pitch_deg) * rad), 0.0, ow, oh, 1.0)
        rt4.write_ppm(path, tracer_lut.retina_project_host(vox, view, ow, oh))
        return open(path, "rb").read()

    assert open(pre + "_yxz_retina.ppm", "rb").read() == picture(30.0, 20.0, str(tmp_path / "want.ppm"))
    # a turntable: three pictures of one volume, the first at yaw 0
    pre3 = str(tmp_path / "t")
    r = subprocess.run(common + ["-o", pre3, "--retina-turntable", "3", "--retina-view", "0", "10"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout, r.stderr)
    names = sorted(os.path.basename(f) for f in glob.glob(pre3 + "*"))
    assert names == ["t_yxz_retina_000.ppm", "t_yxz_retina_001.ppm", "t_yxz_retina_002.ppm"]
    shots = [open(os.path.join(str(tmp_path), n), "rb").read() for n in names]
    assert shots[0] == picture(0.0, 10.0, str(tmp_path / "want0.ppm"))
    assert shots[1] == picture(120.0, 10.0, str(tmp_path / "want1.ppm")) and len(set(shots)) == 3
