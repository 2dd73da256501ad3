"""The 3D retina view on the CPU: the host-only helpers of include/rt4.h (rt4_retina_slice_uniforms,
rt4_retina_params_default, rt4_retina_view_make) against tests/retina_ref.py and against exact expectations, and
independent checks of the restatement itself (no GPU needed; nothing here launches a kernel)."""
import ctypes
import math
import types

import numpy as np
import pytest

import retina_ref
from denoise_ref import F32

ERR_ARG = -1


def raw(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def view_u(rt4):
    u = rt4.make_uniforms(16, 12, samples=3, reflections=4, seed=-77, te=20.0, fi=35.0, psi=10.0)
    return u, rt4.Orientation(math.radians(35.0), math.radians(20.0), math.radians(10.0)).w_drct


# ------------------------------------------------------------------------------------------------- slice uniforms
@pytest.mark.parametrize("depth", [1, 2, 5, 8, 256])
def test_slice_uniforms_match_the_restatement(rt4, view_u, depth):
    u, w_drct = view_u
    for ds in (float(u.mtr_sizes[1]), 0.3):
        seeds = set()
        for s in range(depth):
            got = rt4.retina_slice_uniforms(u, w_drct, depth, ds, s)
            want = retina_ref.slice_uniforms(u, w_drct, depth, ds, s)
            assert bytes(got) == bytes(want), (depth, s)
            seeds.add(got.seed)
            # nothing but the matrix centre and the seed moves
            back = rt4.Uniforms.from_buffer_copy(bytes(got))
            back.seed = u.seed
            for c in range(4):
                back.vec_to_mtr[c] = u.vec_to_mtr[c]
            assert bytes(back) == bytes(u)
        assert len(seeds) == depth  # every slice its own noise


def test_middle_slice_is_the_plain_section(rt4, view_u):
    u, w_drct = view_u
    for depth in (1, 3, 5, 255):
        assert bytes(rt4.retina_slice_uniforms(u, w_drct, depth, 2.0, depth // 2)) == bytes(u)
    # and the slices step along w_drct by depth_size / depth
    a, b = (rt4.retina_slice_uniforms(u, w_drct, 5, 2.0, s) for s in (0, 4))
    step = (np.array(list(b.vec_to_mtr)) - np.array(list(a.vec_to_mtr))) / 4
    assert np.allclose(step, np.array(w_drct) * 2.0 / 5, atol=1e-6)


def test_slice_uniforms_argument_errors(rt4, view_u):
    u, w_drct = view_u
    out = rt4.Uniforms()
    wd = (ctypes.c_float * 4)(*w_drct)
    f = rt4.lib.rt4_retina_slice_uniforms

    def call(uu=ctypes.byref(u), w=wd, depth=5, ds=2.0, s=2, o=ctypes.byref(out)):
        return f(uu, w, depth, ds, s, o)

    assert call() == 0
    assert call(uu=None) == ERR_ARG and call(w=None) == ERR_ARG and call(o=None) == ERR_ARG
    assert call(depth=0) == ERR_ARG and call(depth=257) == ERR_ARG and call(depth=-1) == ERR_ARG
    assert call(s=-1) == ERR_ARG and call(s=5) == ERR_ARG
    for ds in (0.0, -1.0, float("inf"), float("nan")):
        assert call(ds=ds) == ERR_ARG, ds
    assert call(depth=256, s=255) == 0
    with pytest.raises(rt4.RT4Error):
        rt4.retina_slice_uniforms(u, w_drct, 5, 2.0, 5)


def test_params_default(rt4):
    p = rt4.retina_params()
    assert (p.alpha_sky, p.alpha_fill, p.alpha_edge, p.t_min, list(p.background)) == (0.0, 1 / 32, 0.5, 1 / 256, [0.0] * 3)
    d = retina_ref.DEFAULTS
    assert (d["alpha_sky"], d["alpha_fill"], d["alpha_edge"], d["t_min"]) == (p.alpha_sky, p.alpha_fill, p.alpha_edge, p.t_min)
    q = rt4.retina_params(alpha_fill=0.25, background=(0.5, 0.25, 1.0))
    assert q.alpha_fill == 0.25 and list(q.background) == [0.5, 0.25, 1.0] and q.alpha_edge == 0.5


# ---------------------------------------------------------------------------------------------------- view helper
def identity_view(rt4, **kw):
    args = dict(w=16, h=8, d=4, size=(4.0, 2.0, 1.0), yaw=0.0, pitch=0.0, extent=4.0, ow=16, oh=8, step_voxels=1.0)
    args.update(kw)
    return rt4.retina_view(**args)


def sample_positions(view, ow, oh, n):
    """f (oh, ow, 3) of sample n through the restatement's own arithmetic."""
    from denoise_ref import fma32

    a = (np.arange(ow).astype(F32) + F32(0.5)) / F32(ow) - F32(0.5)
    b = F32(0.5) - (np.arange(oh).astype(F32) + F32(0.5)) / F32(oh)
    out = np.empty((oh, ow, 3), F32)
    for c in range(3):
        base = fma32(b[:, None], F32(view.dv[c]), fma32(a[None, :], F32(view.du[c]), F32(view.origin[c])))
        out[..., c] = fma32(F32(n) + F32(0.5), F32(view.dt[c]), base)
    return out


def test_identity_view_is_exact(rt4):
    v = identity_view(rt4)
    assert v.steps == 4  # covers the box: slices 0..3
    jj, ii = np.meshgrid(np.arange(16), np.arange(8))
    for n in range(v.steps):
        f = sample_positions(v, 16, 8, n)
        assert np.array_equal(f[..., 0], jj) and np.array_equal(f[..., 1], ii) and (f[..., 2] == n).all()
    # half the step: twice the samples, the first a quarter voxel inside the box's front face
    v2 = identity_view(rt4, step_voxels=0.5)
    assert v2.steps == 8 and list(v2.dt) == [0.0, 0.0, 0.5] and v2.origin[2] == -0.5
    # extent 0: the box diagonal
    v0 = identity_view(rt4, extent=0.0)
    assert v0.du[0] == F32(math.sqrt(21.0) * 4.0) and v0.steps == 4


def test_yaw_90_swaps_x_and_z(rt4):
    v = identity_view(rt4, yaw=math.pi / 2)
    # the rays run along +x (4 voxels per scene unit), the picture's right is -z, up stays up
    step = 0.25  # the smallest voxel edge
    assert np.allclose(list(v.dt), [4.0 * step, 0.0, 0.0], atol=1e-6)
    assert np.allclose(list(v.du), [0.0, 0.0, -4.0 * 4.0], atol=1e-5)
    assert np.allclose(list(v.dv), [0.0, -2.0 * 4.0, 0.0], atol=1e-6)
    assert v.steps == 16 and abs(v.origin[0] - (-0.5)) < 1e-5  # across the box's 16 columns, from its side face
    # yaw 180: the rays run along -z, the last slice first
    v = identity_view(rt4, yaw=math.pi)
    assert np.allclose(list(v.dt), [0.0, 0.0, -1.0], atol=1e-6) and abs(v.origin[2] - 3.5) < 1e-5


@pytest.mark.parametrize("yaw,pitch", [(0.0, 0.0), (0.5235988, 0.3490659), (1.5707964, 0.0), (2.0, -1.0), (-0.7, 1.2)])
def test_view_axes_are_orthogonal(rt4, yaw, pitch):
    w, h, d, size = 24, 16, 7, (3.2, 2.0, 1.5)
    v = rt4.retina_view(w, h, d, size, yaw, pitch, 0.0, 40, 24, 1.0)
    unscale = np.array([size[0] / w, -size[1] / h, size[2] / d])  # voxel -> scene
    du, dv, dt = (np.array(list(x), np.float64) * unscale for x in (v.du, v.dv, v.dt))
    for p, q in ((du, dv), (du, dt), (dv, dt)):
        assert abs(np.dot(p, q)) / (np.linalg.norm(p) * np.linalg.norm(q)) < 1e-5
    diag = math.sqrt(sum(s * s for s in size))
    assert abs(np.linalg.norm(du) - diag) < 1e-4 and abs(np.linalg.norm(dv) - diag * 24 / 40) < 1e-4
    assert abs(np.linalg.norm(dt) - min(size[0] / w, size[1] / h, size[2] / d)) < 1e-6
    # the ray through the picture's centre passes through the box's centre half way
    mid = np.array(list(v.origin), np.float64) + 0.5 * v.steps * np.array(list(v.dt), np.float64)
    assert np.allclose(mid, [(w - 1) / 2, (h - 1) / 2, (d - 1) / 2], atol=1.0)
    assert 1 <= v.steps <= rt4.RETINA_MAX_STEPS


def test_view_argument_errors(rt4):
    ok = dict(w=16, h=8, d=4, size=(4.0, 2.0, 1.0), yaw=0.0, pitch=0.0, extent=4.0, ow=16, oh=8, step_voxels=1.0)
    rt4.retina_view(**ok)
    bad = [dict(w=0), dict(h=0), dict(d=0), dict(ow=0), dict(oh=-1), dict(size=(0.0, 2.0, 1.0)), dict(size=(4.0, -2.0, 1.0)),
           dict(size=(4.0, 2.0, float("nan"))), dict(yaw=float("inf")), dict(pitch=float("nan")), dict(extent=-1.0),
           dict(extent=float("inf")), dict(step_voxels=0.0), dict(step_voxels=float("nan")), dict(step_voxels=1e-4)]
    for kw in bad:
        with pytest.raises(rt4.RT4Error) as e:
            rt4.retina_view(**{**ok, **kw})
        assert e.value.status == ERR_ARG, kw


# ------------------------------------------------------------------------- independent checks of the restatement
def random_voxels(seed, d=4, h=8, w=16):
    rng = np.random.default_rng(seed)
    a = rng.choice(np.array([0.0, 1 / 32, 0.5, 1.0], F32), size=(d, h, w))
    V = np.empty((d, h, w, 4), F32)
    V[..., :3] = a[..., None] * rng.random((d, h, w, 3), dtype=F32)
    V[..., 3] = a
    return V


def test_identity_projection_is_plain_over(rt4):
    V = random_voxels(1)
    bg = (0.25, 0.5, 0.125)
    frame, plan = retina_ref.project(V, identity_view(rt4), 16, 8, t_min=0.0, background=bg)
    assert raw(frame[..., :3]) == raw(retina_ref.over(V, bg)) and (frame[..., 3] == 1).all()
    assert plan["outside"] == 0 and plan["inside"] + plan["partly"] == 16 * 8 * 4 and plan["stopped"] == 0
    # t_min only cuts rays short once they are nearly opaque: it moves no pixel by more than t_min
    cut, plan_cut = retina_ref.project(V, identity_view(rt4), 16, 8, t_min=0.5, background=bg)
    assert plan_cut["stopped"] > 0 and plan_cut["ran_out"] > 0
    assert np.abs(cut[..., :3] - frame[..., :3]).max() <= 0.5


def test_all_alphas_zero_is_the_background(rt4):
    V = np.zeros((4, 8, 16, 4), F32)
    bg = (0.3, 0.6, 0.9)
    for dtype in (np.float32, np.float16, np.uint8):
        frame, plan = retina_ref.project(V, identity_view(rt4), 16, 8, background=bg, dtype=dtype)
        want = np.empty((8, 16, 4), dtype)
        want[..., :3] = retina_ref.encode(np.array(bg, F32), np.dtype(dtype))
        want[..., 3] = 255 if dtype == np.uint8 else 1
        assert raw(frame) == raw(want) and plan["stopped"] == 0


def test_all_alphas_one_is_slice_zero(rt4):
    V = random_voxels(2)
    V[..., 3] = 1
    frame, plan = retina_ref.project(V, identity_view(rt4), 16, 8, background=(1.0, 1.0, 1.0))
    assert raw(frame[..., :3]) == raw(V[0, ..., :3]) and plan["stopped"] == 16 * 8
    # from behind (yaw 180) the last slice shows, mirrored left to right
    back, _ = retina_ref.project(V, identity_view(rt4, yaw=math.pi), 16, 8)
    assert np.allclose(back[..., :3], V[3, :, ::-1, :3], atol=1e-5)


def test_voxelize_restatement_on_a_hand_made_volume(rt4):
    light = np.zeros((2, 3, 4), rt4.LIGHT_DTYPE)
    gbuf = np.zeros((2, 3, 4), rt4.GBUFFER_DTYPE)
    light["mean"] = 1.0
    light["n"] = 1
    light["n"][0, 0, 0] = 0
    gbuf["surface"] = 3
    gbuf["surface"][1, 1, 2] = 5  # one voxel of another surface: it and its six neighbours inside are edges
    gbuf["surface"][0, 2, 0] = -1  # one sky voxel: its neighbours are edges, it is not
    V, plan = retina_ref.voxelize(light, gbuf, 1.0, 0.0, 0.25, 1.0)
    edge = {(1, 1, 2), (0, 1, 2), (1, 0, 2), (1, 2, 2), (1, 1, 1), (1, 1, 3), (0, 1, 0), (0, 2, 1), (1, 2, 0)}
    for s in range(2):
        for i in range(3):
            for j in range(4):
                a = 0.0 if (s, i, j) == (0, 2, 0) else 1.0 if (s, i, j) in edge else 0.25
                c = 0.0 if (s, i, j) == (0, 0, 0) else 0.5  # 1 - 1/(1*1 + 1)
                assert list(V[s, i, j]) == [a * c] * 3 + [a], (s, i, j)
    assert plan == dict(edge=9, fill=14, sky=1, surfaces=2)


def test_project_plan_counts_a_miss_and_nan(rt4):
    V = random_voxels(3)
    nan_view = types.SimpleNamespace(origin=[float("nan")] * 3, du=[16.0, 0.0, 0.0], dv=[0.0, -8.0, 0.0], dt=[0.0, 0.0, 1.0], steps=4)
    miss_view = types.SimpleNamespace(origin=[40.0, 3.5, -0.5], du=[16.0, 0.0, 0.0], dv=[0.0, -8.0, 0.0], dt=[0.0, 0.0, 1.0], steps=4)
    for view in (nan_view, miss_view):
        frame, plan = retina_ref.project(V, view, 5, 3, background=(0.5, 0.25, 0.75))
        assert plan["never_entered"] == 15 and plan["outside"] == 60 and plan["inside"] == plan["partly"] == 0
        assert (frame == np.array([0.5, 0.25, 0.75, 1.0], F32)).all()
