"""The sphere cull of the spheres, the cylinders and the unions' cylinders at its seams, on the GPU (pytest -m gpu):
rays of cull_ref's strata through rt4_debug_find_intersection and through rt4_debug_cull (the kernels' own
decision), renders of the silhouette from 50 radii away, and the derivation's sin(acos) figure on the device. The
oracle alone is test_cull_ref.py.

A cull the host switched off (r2m = +inf) makes every bitwise comparison pass trivially, so the probe is also asserted
to fire on every case here, and to keep to the shader's own early-out where the host must disable the margin test.
"""
import ctypes

import numpy as np
import pytest

import cull_ref as cr
import denoise_ref
import scene_builder
from test_gpu_parity import assert_bits, bits_equal
from test_gpu_random_scenes import perturb

pytestmark = pytest.mark.gpu

N = 20000  # rays per stratum and figure
NAMED = ["sphere", "room", "all_primitives", "cylinder4d"]
RUNTIME = ["all_2_3_2"]  # three spheres, two cylinders, a union: the runtime-count kernel
PERTURBED = [("all_primitives", 1), ("all_primitives", 2), ("cylinder4d", 1), ("cylinder4d", 2)]
# the object of each scene that takes the special radii
RADIUS_ON = {"sphere": ("sphere", 0), "all_primitives": ("sphere", 1), "cylinder4d": ("union", (0, 0))}
RADII = [f"{n}@{k}" for n in RADIUS_ON for k in range(1, len(cr.ENABLED_RADII))]
CASES = NAMED + RUNTIME + [f"{n}~{s}" for n, s in PERTURBED] + RADII
_cache = {}


def scene_desc(rt4, case):
    """(scene, the figures whose strata the case runs): all of them, or the one with the special radius."""
    if "@" in case:
        name, k = case.split("@")
        d = rt4.SceneDesc.from_buffer_copy(rt4.Scene.named(name).to_bytes())
        cr.set_radius(d, *RADIUS_ON[name], cr.ENABLED_RADII[int(k)])
        return d, [cr.figure_of(d, *RADIUS_ON[name])]
    if case in NAMED:
        d = rt4.Scene.named(case).desc
    elif case in RUNTIME:
        d = scene_builder.build_case(rt4, case)
    else:
        name, seed = case.split("~")
        d = perturb(rt4, name, int(seed)).desc
    return d, cr.figures(d)


def case_data(rt4, oracle, case):
    """(desc, [(figure, stratum, decision, figure-only oracle rows, slice into the rays)], all rays, oracle rows and
    colours of the whole scene), computed once per case."""
    if case not in _cache:
        d, figs = scene_desc(rt4, case)
        parts, rays, at = [], [], 0
        for k, fig in enumerate(figs):
            assert fig.enabled, f"{case}: the cull of {fig.kind} {fig.index} is one the host enables"
            alone = cr.figure_only(rt4, d, fig.kind, fig.index)
            for st in cr.strata(fig, 7 * len(case) + 1000 * k, N):
                out, _ = oracle.find_intersection(alone, st.rays)
                parts.append((fig, st, cr.decide(fig, st.rays), out, slice(at, at + N)))
                rays.append(st.rays)
                at += N
        rays = np.concatenate(rays)
        c, cc = oracle.find_intersection(d, rays)
        _cache[case] = (d, parts, rays, c, cc)
    return _cache[case]


def first_bad(parts, rays, eq):
    i = int(np.flatnonzero(~eq.all(axis=1))[0])
    fig, st, _, _, sl = next(p for p in parts if p[4].start <= i < p[4].stop)
    return f"ray {i} ({fig.kind} {fig.index}, stratum {st.label}, e = {st.e[i - sl.start]}): {rays[i].tolist()}"


def bit_of(mask, fig):
    return ((mask[:, fig.word] >> np.uint32(fig.bit)) & 1) != 0


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_find_intersection_bitwise(rt4, oracle, case, generic):
    """rt4_debug_find_intersection == the oracle, rows and colours, bit for bit, on every stratum: the specialised
    kernel, whose cull these rays aim at, and the generic one."""
    d, parts, rays, c, cc = case_data(rt4, oracle, case)
    t = rt4.Tracer(device=0, scene=rt4.Scene(d), flags=rt4.FLAG_GENERIC_KERNEL if generic else 0)
    try:
        g, gc = t.debug_find_intersection(rays)
    finally:
        t.close()
    eq = np.concatenate([bits_equal(g, c), bits_equal(gc, cc)], axis=1)
    assert eq.all(), f"{case}: {(~eq.all(axis=1)).sum()} of {len(rays)} rays differ, first: {first_bad(parts, rays, eq)}"


@pytest.mark.parametrize("case", CASES)
def test_probe_decision(rt4, oracle, case):
    """The kernels' own decision (rt4_debug_cull) on every stratum:
      * a ray whose bit is set gets no hit from the oracle on the scene that holds only that figure;
      * of the rays the float64 restatement puts clearly in the cull's region (outside; dp < 0 or a margin of 1e-4 and
        more), at least 99 % have the bit set (the count is printed; being cautious is no bug, a dead cull is);
      * among the rays within 1e-5 of the threshold both decisions occur, each on at least 25 % (pooled over the
        figure's strata; far out the direction's own rounding spreads the aimed rays over +-1e-2, so a radius below
        SMALL, whose every outside origin is far out, has some tens of them: at least 20);
      * overflow rays whose float32 P is not finite, and that do not take the early-out (dp < 0), are not culled;
      * every tangent stratum holds at least 50 hits of the figure.
      * the probe equals the numpy float32 restatement of the predicate (cull_ref.predicate32) on every ray: d2_out,
        r2m and K are then the host's to the bit wherever a ray comes near them."""
    d, parts, rays, c, cc = case_data(rt4, oracle, case)
    t = rt4.Tracer(device=0, scene=rt4.Scene(d))
    try:
        mask = t.debug_cull(rays)
    finally:
        t.close()
    n_clear = n_clear_set = 0
    near = {}
    for fig, st, dec, out, sl in parts:
        bit = bit_of(mask[sl], fig)
        hit = out[:, 0] > 0
        what = f"{case} {fig.kind} {fig.index} {st.label}"
        _, dp32, p32, _, _, fires = cr.predicate32(fig, st.rays)
        print(f"{what}: culled {int(bit.sum())} of {len(bit)}, clear {int(dec.clear.sum())}, of them set "
              f"{int((dec.clear & bit).sum())}, near {int(dec.near.sum())}, of them set {int((dec.near & bit).sum())}, "
              f"figure hits {int(hit.sum())}, differs from the float32 restatement on {int((fires != bit).sum())}")
        off = np.flatnonzero(fires != bit)
        assert off.size == 0, f"{what}: the probe differs from the float32 restatement on {off.size} rays, first: " \
                              f"ray {off[0]} {st.rays[off[0]].tolist()} (probe {bit[off[0]]}, margin {dec.margin[off[0]]})"
        bad = np.flatnonzero(bit & hit)
        assert bad.size == 0, f"{what}: {bad.size} culled rays hit, first: ray {bad[0]} {st.rays[bad[0]].tolist()} " \
                              f"(e = {st.e[bad[0]]}, dist {out[bad[0], 1]}, margin {dec.margin[bad[0]]})"
        n_clear += int(dec.clear.sum())
        n_clear_set += int((dec.clear & bit).sum())
        k = (fig.kind, fig.index)
        near[k] = (near.get(k, (0, 0))[0] + int(dec.near.sum()), near.get(k, (0, 0))[1] + int((dec.near & bit).sum()))
        if st.label == "overflow":
            with np.errstate(invalid="ignore"):
                nonfinite = ~np.isfinite(p32) & ~(dp32 < 0)
            assert nonfinite.sum() >= 50, what
            assert not (bit & nonfinite).any(), f"{what}: culled with a non-finite P"
        if st.label == "tangent":
            assert hit.sum() >= 50, f"{what}: {int(hit.sum())} figure hits"
    for k, (n, n_set) in near.items():
        print(f"{case} {k}: {n} rays at the threshold, culled share {n_set / max(n, 1):.3f}")
        assert n >= 20 and 0.25 <= n_set / n <= 0.75, (case, k)
    print(f"{case}: {n_clear_set} of {n_clear} clearly cullable rays culled ({n_clear_set / n_clear:.4f})")
    assert n_clear_set >= 0.99 * n_clear


def test_probe_zero_where_the_host_disables(rt4, oracle):
    """For every radius the host must disable (below 1e-15, above 1e15, 0, negative, NaN, inf) the margin test never
    fires, on any stratum of the figure's own radius: the bit is 0 on every ray but those of the shader's own
    early-out (:206: outside, len_po >= max(r, SMALL), and dp < 0), which needs none of the host's margin and which
    find_pre and sphere_culled take whatever r2m is; a NaN radius is never outside, so its bit is 0 throughout. And
    find_intersection still equals the oracle, on the specialised and on the generic kernel."""
    for name, (kind, index) in RADIUS_ON.items():
        base = rt4.Scene.named(name).desc
        own = cr.figure_of(base, kind, index)
        strata = cr.strata(own, 99, 4000)
        rays = np.concatenate([st.rays for st in strata])
        t = rt4.Tracer(device=0, scene=rt4.Scene(base))
        try:
            assert bit_of(t.debug_cull(rays), own).mean() > 0.2, name  # the same rays do cull at the scene's own radius
        finally:
            t.close()
        own_dec = cr.decide(own, rays)
        for r in cr.DISABLED_RADII:
            d = rt4.SceneDesc.from_buffer_copy(bytes(base))
            cr.set_radius(d, kind, index, r)
            fig = cr.figure_of(d, kind, index)
            assert not fig.enabled and fig.r2m == np.inf
            dec = cr.decide(fig, rays)
            c, cc = oracle.find_intersection(d, rays)
            for generic in (False, True):
                t = rt4.Tracer(device=0, scene=rt4.Scene(d), flags=rt4.FLAG_GENERIC_KERNEL if generic else 0)
                try:
                    g, gc = t.debug_find_intersection(rays)
                    bit = bit_of(t.debug_cull(rays), fig)
                finally:
                    t.close()
                assert_bits(g, c, f"{name} r={r} generic={generic}")
                assert_bits(gc, cc, f"{name} r={r} colour generic={generic}")
            # dp clearly not negative: above the float32 dot's rounding, 4 u |po| |d|
            rays64 = rays.astype(np.float64)
            dlen = np.sqrt((rays64[:, 4:] ** 2).sum(1)) if fig.a1 is None else 1.0
            with np.errstate(all="ignore"):
                ahead = ~(dec.dp < 1e-6 * np.sqrt(dec.d2) * dlen)
                d2_32 = dec.d2.astype(np.float32)  # +inf where the float32 d2 overflows: outside of any radius
            wrong = np.flatnonzero(bit & (ahead | (d2_32 < fig.d2_out * (1 - 1e-6))))
            would = own_dec.clear & ~(own_dec.dp < 0) & ahead
            print(f"{name} r={r}: bit set on {int(bit.sum())} rays (early-out), 0 of the {int(would.sum())} that the "
                  f"margin test culls at the scene's own radius")
            assert wrong.size == 0, f"{name} r={r}: ray {wrong[0]} {rays[wrong[0]].tolist()}"
            assert would.sum() >= 300 and not (bit & would).any()
            if r != r:
                assert not bit.any()


# ------------------------------------------------------------------------------------------ through the trace kernels
RENDER = {"sphere": ("sphere", 0), "room": ("sphere", 0), "all_primitives": ("sphere", 0), "cylinder4d": ("union", (0, 0))}
KERNELS = {"lut": lambda rt4: rt4.FLAG_SAMPLER_LUT, "inline": lambda rt4: 0,
           "reuse": lambda rt4: rt4.FLAG_SAMPLER_LUT | rt4.FLAG_PRIMARY_REUSE,
           "generic": lambda rt4: rt4.FLAG_GENERIC_KERNEL}
RENDER_CASES = [("sphere", k) for k in KERNELS] + [(n, "lut") for n in ("room", "all_primitives", "cylinder4d")]
_views = {}


def views(rt4, oracle, name):
    """[(small_indent, uniforms, oracle frame, oracle count)] of the scene's seam view, with the usual indent and with
    none (then every bounce starts on the `outside` seam of the surface it left)."""
    if name not in _views:
        d = rt4.Scene.named(name).desc
        fig = cr.figure_of(d, *RENDER[name])
        reg = rt4.region(64, 40)
        _views[name] = []
        for indent in (0.005, 0.0):
            u = cr.seam_view(rt4, fig, small_indent=indent)
            _views[name].append((indent, u) + tuple(oracle.render(d, u, reg)[:2]))
    return _views[name]


@pytest.mark.parametrize("name,kernel", RENDER_CASES)
def test_seam_renders(rt4, oracle, name, kernel):
    """A 64 x 40 view of the figure's silhouette from 50 radii away, zoomed to r (1 +- 4 m) (cull_ref.seam_view): the
    probe culls 0.25 .. 0.75 of the primary rays; 2 samples and 3 reflections render bit-equal to the oracle, image and
    intersection count, with small_indent 0.005 and 0; for `sphere` and `all_primitives` (sampler table) three
    progressive frames pipelined in one render_frames_device call do too (the deferred-sphere and deferred-tiger
    kernels' pipelined path)."""
    scene = rt4.Scene.named(name)
    fig = cr.figure_of(scene.desc, *RENDER[name])
    reg = rt4.region(64, 40)
    t = rt4.Tracer(device=0, scene=scene, flags=KERNELS[kernel](rt4))
    try:
        for indent, u, fc, nc in views(rt4, oracle, name):
            share = bit_of(t.debug_cull(denoise_ref.primary_rays(u, reg).reshape(-1, 8)), fig).mean()
            print(f"{name} {kernel} indent {indent}: primary rays culled {share:.3f}")
            assert 0.25 <= share <= 0.75, f"{name} indent {indent}"
            fg = np.zeros((40, 64, 4), np.float32)
            ng = t.render_host(u, reg, fg)
            assert ng == nc, f"{name} {kernel} indent {indent}: {ng} intersections, oracle {nc}"
            assert_bits(fg, fc, f"{name} {kernel} indent {indent}")
        if kernel == "lut" and name in ("sphere", "all_primitives"):
            import torch

            for indent, u, _, _ in views(rt4, oracle, name):
                us = [rt4.progressive_uniforms(u, n) for n in range(1, 4)]
                fr = torch.zeros((40, 64, 4), dtype=torch.float32, device="cuda")
                cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
                t.render_frames_device(us, reg, fr.data_ptr(), rt4.FRAME_RGBA32F, 64, cnt.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream)
                torch.cuda.synchronize()
                cpu3, m3 = np.zeros((40, 64, 4), np.float32), 0
                for uf in us:
                    _, k = oracle.render_fmt(scene.desc, uf, reg, rt4.FRAME_RGBA32F, frame=cpu3)
                    m3 += k
                assert int(cnt.item()) == m3, f"{name} indent {indent}: pipelined frames' intersections"
                assert_bits(fr.cpu().numpy(), cpu3, f"{name} indent {indent} pipelined frames")
    finally:
        t.close()


def test_sin_acos_premise(rt4, oracle, tracer):
    """The derivation's cited figure on the device: sin_(acos_(c)) through rt4_debug_eval over every float of [0.5, 1)
    and every 64th of [0, 0.5) is bit-equal to the oracle's and within 1.75e-7 (relative) of sqrt(1 - c^2)."""
    c = cr.sweep_inputs()
    a, _ = tracer.debug_eval(rt4.EVAL_ACOS, c)
    s, _ = tracer.debug_eval(rt4.EVAL_SIN, a)
    ca, _ = oracle.eval_array(rt4.EVAL_ACOS, c)
    cs, _ = oracle.eval_array(rt4.EVAL_SIN, ca)
    assert np.array_equal(a.view(np.uint32), ca.view(np.uint32))
    assert np.array_equal(s.view(np.uint32), cs.view(np.uint32))
    worst, at = cr.sin_acos_error(c, s)
    print(f"device sin(acos(c)) over {len(c)} floats: largest relative error {worst:.4e} at c = 0x{at:08X}")
    assert worst <= cr.SIN_ACOS_BOUND


def test_argument_errors_write_nothing(rt4):
    t = rt4.Tracer(device=0, scene=rt4.Scene.named("sphere"))
    empty = rt4.Tracer(device=0)
    try:
        rays = np.ones((4, 8), np.float32)
        out = np.full((4, 2), 0xABCDEF01, np.uint32)
        err = ctypes.create_string_buffer(256)
        call = rt4.lib.rt4_debug_cull
        rp, op = ctypes.c_void_p(rays.ctypes.data), ctypes.c_void_p(out.ctypes.data)
        assert call(None, rp, op, 4, err, len(err)) == -1
        assert call(t._h, None, op, 4, err, len(err)) == -1
        assert call(t._h, rp, None, 4, err, len(err)) == -1
        assert call(t._h, rp, op, -1, err, len(err)) == -1 and err.value
        assert call(empty._h, rp, op, 4, err, len(err)) == -1 and b"scene" in err.value
        assert call(empty._h, rp, op, 4, None, 0) == -1
        assert (out == 0xABCDEF01).all()
        assert call(t._h, rp, op, 0, err, len(err)) == 0 and (out == 0xABCDEF01).all()
        m = t.debug_cull(rays)
        assert m.shape == (4, 2) and m.dtype == np.uint32
        assert (m[:, 0] & ~np.uint32(3)).max() == 0 and m[:, 1].max() == 0  # two spheres, nothing else
    finally:
        empty.close()
        t.close()
