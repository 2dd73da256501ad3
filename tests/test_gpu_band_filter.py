"""The band filters of the union and the tiger at their seams and at special radii, on the GPU (pytest -m gpu):
band_filter_ref's strata through rt4_debug_find_intersection on the specialised and the generic kernel, each radius a
threshold is made from set to special values on its own, and renders zoomed in on a seam until neighbouring pixels
differ by about an ulp in direction (the trace kernels' tiger_quarter and deferred tiger). Bit-exact parity with the
oracle everywhere. Whether a case can show a wrong filter is asserted on the oracle alone (band_filter_ref,
test_band_filter_ref.py), never on the kernels' output.
"""
import numpy as np
import pytest

import band_filter_ref as bf
import scene_builder
from test_gpu_parity import assert_bits, bits_equal

pytestmark = pytest.mark.gpu

N_PER_E = 2000  # rays per offset e and seam kind, shared among the scene's figures of that kind
NAMED = ["tiger", "tiger_two_mirrors", "cylinder4d", "all_primitives"]
# the runtime-count and generic composed cases whose group list tests a union or a tiger
COMPOSED = [n for n, (_, kw) in scene_builder.CASES.items() if kw is not None and (kw.get("unions") or kw.get("tigers"))]
ROTATED = ["rotated_tiger", "rotated_union", "union_unequal"]
CASES = NAMED + COMPOSED + ROTATED
_cache = {}


def scene_desc(rt4, case):
    if case in NAMED:
        return rt4.Scene.named(case).desc
    if case in COMPOSED:
        return scene_builder.build_case(rt4, case)
    if case == "rotated_tiger":
        return scene_builder.compose(rt4, tigers=1, seed=3)
    d = scene_builder.compose(rt4, unions=1, seed=4)
    if case == "union_unequal":  # both filters use cylinder2.r: the one of face 2 is not its own radius
        d.unions[0].cylinder1.r = float(np.float32(1.3 * d.unions[0].cylinder2.r))
    return d


def case_data(rt4, oracle, case):
    """(desc, [(seam, stratum, slice)], rays, oracle rows, oracle colours), once per case: for every figure and seam
    kind the aimed strata of every e, and the exact stratum where the figure is axis-aligned."""
    if case not in _cache:
        d = scene_desc(rt4, case)
        parts, rays, at = [], [], 0
        figures = [("union", i) for i in range(d.n_unions)] + [("tiger", i) for i in range(d.n_tigers)]
        for kind, i in figures:
            n = N_PER_E // (d.n_unions if kind == "union" else d.n_tigers)
            for k, sm in enumerate(bf.seams(d, union=i, tiger=i)):
                if sm.kind != kind:
                    continue
                strata = [bf.aimed_all(sm, 1000 * i + 101 * k + 7 * len(case), n)]
                if bf.axis_aligned(sm):
                    strata.append(bf.exact(sm)[0])
                for st in strata:
                    parts.append((sm, st, slice(at, at + len(st.rays))))
                    rays.append(st.rays)
                    at += len(st.rays)
        rays = np.concatenate(rays)
        c, cc = oracle.find_intersection(d, rays)
        _cache[case] = (d, parts, rays, c, cc)
    return _cache[case]


def first_bad(parts, rays, eq):
    i = int(np.flatnonzero(~eq.all(axis=1))[0])
    sm, st, sl = next(p for p in parts if p[2].start <= i < p[2].stop)
    return f"ray {i} ({sm.name}, {st.label}, e or q = {st.e[i - sl.start]!r}): {rays[i].tolist()}"


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_seam_rays_bitwise(rt4, oracle, case, generic):
    """rt4_debug_find_intersection == the oracle, rows and colours, bit for bit, on the aimed strata of every e and the
    exact stratum of every seam kind of the scene. Printed per seam: the rays inside the rounding noise whose aimed hit
    the oracle keeps and drops (on the whole scene, where other objects may stand in front)."""
    d, parts, rays, c, cc = case_data(rt4, oracle, case)
    if not generic:
        for sm, st, sl in parts:
            if st.label == "aimed":
                noise = np.abs(st.e) <= bf.E_NOISE
                keep = bf.aimed_hit(sm, st, c[sl], cc[sl])
                print(f"{case} {sm.name}: |e| <= 2^-22: {int((keep & noise).sum())} kept, {int((~keep & noise).sum())} not, "
                      f"of {len(st.rays)} aimed rays")
            else:
                print(f"{case} {sm.name}: exact stratum {len(st.rays)} rays, {int((c[sl][:, 0] > 0).sum())} hits")
    t = rt4.Tracer(device=0, scene=rt4.Scene(d), flags=rt4.FLAG_GENERIC_KERNEL if generic else 0)
    try:
        g, gc = t.debug_find_intersection(rays)
    finally:
        t.close()
    eq = np.concatenate([bits_equal(g, c), bits_equal(gc, cc)], axis=1)
    assert eq.all(), f"{case}: {(~eq.all(axis=1)).sum()} of {len(rays)} rays differ, first: {first_bad(parts, rays, eq)}"


SPECIAL = [(f, r) for f in bf.FIELDS for r in bf.SPECIAL_RADII]
# The masked combinations, (radius field, value): the filter cannot show on rays of generic direction, because the
# value is also a face's radius and that face's NaN-distance hit wins every closest(). The table and why are
# band_filter_ref.MASKED; special_case_checked asserts, here and in test_band_filter_ref.py, that exactly these are
# masked and that their exact strata still depend on the radius.
MASKED = bf.MASKED


@pytest.mark.parametrize("field,radius", SPECIAL, ids=[f"{f}={r!r}" for f, r in SPECIAL])
def test_special_radius_alone(rt4, oracle, field, radius):
    """One radius a threshold is made from set to a special value, the others as they are: find_intersection == the
    oracle bit for bit on the specialised and the generic kernel, for 20 000 random rays, the exact stratum of that
    threshold and rays spread across the filtered faces. special_case_checked asserts first, on the oracle alone, that
    the case counts (band_filter_ref.MASKED, MIN_DEPENDENT)."""
    d, rays, c, cc, info, _ = bf.special_case_checked(rt4, oracle, field, radius)
    print(f"{field} = {radius!r}: {info}" + (" (masked)" if (field, repr(radius)) in MASKED else ""))
    for flags in (0, rt4.FLAG_GENERIC_KERNEL):
        t = rt4.Tracer(device=0, scene=rt4.Scene(d), flags=flags)
        try:
            g, gc = t.debug_find_intersection(rays)
        finally:
            t.close()
        eq = np.concatenate([bits_equal(g, c), bits_equal(gc, cc)], axis=1).all(axis=1)
        bad = np.flatnonzero(~eq)
        assert bad.size == 0, (f"{field} = {radius!r} flags {flags}: {bad.size} of {len(rays)} rays differ ({int((bad >= 20000).sum())} "
                               f"of them past the random rays), first: ray {bad[0]} {rays[bad[0]].tolist()}: "
                               f"{g[bad[0]].tolist()} / oracle {c[bad[0]].tolist()}")


# ------------------------------------------------------------------------------------------ through the trace kernels
@pytest.mark.parametrize("name", NAMED)
def test_seam_zoom_renders(rt4, oracle, name):
    """render_host == oracle.render, image and intersection count, for views zoomed in on a seam point of every kind
    (64 x 40, 2 samples, 2 reflections, matrix heights 2^-14, 2^-18, 2^-20): the primary rays of neighbouring pixels
    sweep q across the threshold. The LUT sampler, with primary reuse, and the generic kernel."""
    scene = rt4.Scene.named(name)
    reg = rt4.region(64, 40)
    cases = bf.zoom_cases(rt4, oracle, name)  # asserts the two pixel classes on the oracle's frame
    ref = [oracle.render(scene.desc, u, reg)[:2] for _, u, _ in cases]
    for flags in (rt4.FLAG_SAMPLER_LUT, rt4.FLAG_SAMPLER_LUT | rt4.FLAG_PRIMARY_REUSE, rt4.FLAG_GENERIC_KERNEL):
        t = rt4.Tracer(device=0, scene=scene, flags=flags)
        try:
            for (label, u, _), (fc, nc) in zip(cases, ref):
                fg = np.zeros((40, 64, 4), np.float32)
                ng = t.render_host(u, reg, fg)
                assert ng == nc, f"{name} flags {flags} {label}: {ng} intersections, oracle {nc}"
                assert_bits(fg, fc, f"{name} flags {flags} {label}")
        finally:
            t.close()


def test_seam_zoom_pipelined_frames(rt4, oracle):
    """The tiger's zoomed views as three progressive frames through render_frames_device: the pipelined instantiation
    of the trace kernel."""
    import torch

    scene = rt4.Scene.named("tiger")
    reg = rt4.region(64, 40)
    t = rt4.Tracer(device=0, scene=scene, flags=rt4.FLAG_SAMPLER_LUT)
    try:
        for label, u, _ in bf.zoom_cases(rt4, oracle, "tiger"):
            us = [rt4.progressive_uniforms(u, n) for n in range(1, 4)]
            fr = torch.zeros((40, 64, 4), dtype=torch.float32, device="cuda")
            cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
            t.render_frames_device(us, reg, fr.data_ptr(), rt4.FRAME_RGBA32F, 64, cnt.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            fc, nc = np.zeros((40, 64, 4), np.float32), 0
            for uf in us:
                nc += oracle.render_fmt(scene.desc, uf, reg, rt4.FRAME_RGBA32F, frame=fc)[1]
            assert int(cnt.item()) == nc, f"tiger {label}: {int(cnt.item())} intersections, oracle {nc}"
            assert_bits(fr.cpu().numpy(), fc, f"tiger {label} pipelined")
    finally:
        t.close()
