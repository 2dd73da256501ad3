"""The bounding-ball skips of the tiger, the union and the hypercube at their boundaries, on the GPU (pytest -m gpu):
rays of bound_ball_ref's strata through rt4_debug_find_intersection and through rt4_debug_bound_skip (the kernels'
own decision), and renders from a camera on the ball's surface. The oracle alone is test_bound_ball_ref.py.

A ball the host disabled (r2m = +inf) makes every bitwise comparison pass trivially, so the probe is also asserted
to fire on every scene here and to stay zero where the host must disable the ball.
"""
import numpy as np
import pytest

import bound_ball_ref as bb
import denoise_ref
import scene_builder
from test_gpu_parity import assert_bits, bits_equal
from test_gpu_random_scenes import SPECIAL_RADII, perturb

pytestmark = pytest.mark.gpu

N_STRATUM = {1: 8000, 3: 16000}  # rays per stratum by the scene's number of figures: 40k rays for one figure;
# the three figures of the all-primitives scenes get more, their tangent strata yield a hit in ~150 rays
BIT = {"union": 1, "tiger": 2, "hypercube": 4}
NAMED = ["tiger", "tiger_two_mirrors", "cylinder4d", "hypercube", "all_primitives"]
RUNTIME = ["tiger_2", "union_2", "hypercube_2", "all_2_2_1"]
PERTURBED = [("tiger", 1), ("tiger", 2), ("cylinder4d", 1), ("cylinder4d", 2)]
CASES = NAMED + RUNTIME + [f"{n}~{s}" for n, s in PERTURBED]
_cache = {}


def scene_desc(rt4, case):
    if case in NAMED:
        return rt4.Scene.named(case).desc
    if case in RUNTIME:
        return scene_builder.build_case(rt4, case)
    name, seed = case.split("~")
    return perturb(rt4, name, int(seed)).desc


def case_data(rt4, oracle, case):
    """(desc, [(kind, ball, stratum, decision, figure-only oracle rows, slice into the rays)], all rays, oracle rows
    and colours of the whole scene), computed once per case."""
    if case not in _cache:
        d = scene_desc(rt4, case)
        balls = bb.balls(d)
        n = N_STRATUM[len(balls)]
        parts, rays, at = [], [], 0
        for kind, ball in balls.items():
            assert ball.enabled, f"{case}: the {kind}'s ball is one the host enables"
            alone = bb.figure_only(rt4, d, kind)
            for st in bb.strata(ball, 7 * len(case) + 31 * BIT[kind], n):
                out, _ = oracle.find_intersection(alone, st.rays)
                parts.append((kind, ball, st, bb.decide(ball, st.rays), out, slice(at, at + n)))
                rays.append(st.rays)
                at += n
        rays = np.concatenate(rays)
        c, cc = oracle.find_intersection(d, rays)
        _cache[case] = (d, parts, rays, c, cc)
    return _cache[case]


def first_bad(parts, rays, eq):
    i = int(np.flatnonzero(~eq.all(axis=1))[0])
    kind, _, st, _, _, sl = next(p for p in parts if p[5].start <= i < p[5].stop)
    return f"ray {i} ({kind}, stratum {st.label}, e = {st.e[i - sl.start]}): {rays[i].tolist()}"


@pytest.mark.parametrize("generic", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_find_intersection_bitwise(rt4, oracle, case, generic):
    """rt4_debug_find_intersection == the oracle, bit for bit, on every stratum: the specialised kernel, whose skips
    these rays aim at, and the generic one."""
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
    """The kernels' own decision (rt4_debug_bound_skip) on every stratum:
      * a ray whose skip bit is set (hypercube: all eight cells rejected) gets no hit from the oracle on the scene
        that holds only that figure;
      * of the rays the float64 restatement puts clearly in the skip region, at least 99 % have the bit set (the
        count is printed; being conservative is no bug, a dead skip is);
      * the boundary is straddled: among the tangent and behind rays within |e| <= 1e-4 both decisions occur, each
        on at least 10 % of them; so they do among the band rays within a factor two of the band's edge
        (|e| >= 5e-3) that pass the ball test from within ten ball radii, and among the hyper_parallel rays whose
        line clears the ball (all cells rejected or not);
      * every stratum holds at least 50 hits of the figure."""
    d, parts, rays, c, cc = case_data(rt4, oracle, case)
    t = rt4.Tracer(device=0, scene=rt4.Scene(d))
    try:
        mask = t.debug_bound_skip(rays)
    finally:
        t.close()
    n_clear = n_clear_set = 0
    for kind, ball, st, dec, out, sl in parts:
        m = mask[sl]
        bit = (m & BIT[kind]) != 0
        skipped = bit if kind != "hypercube" else ((m >> 8) & 0xFF) == 0xFF
        hit = out[:, 0] > 0
        bad = np.flatnonzero(skipped & hit)
        what = f"{case} {kind} {st.label}"
        print(f"{what}: skipped {int(skipped.sum())} of {len(m)}, clear {int(dec.clear.sum())}, of them set "
              f"{int((dec.clear & bit).sum())}, figure hits {int(hit.sum())}")
        assert bad.size == 0, f"{what}: {bad.size} skipped rays hit, first: ray {bad[0]} {st.rays[bad[0]].tolist()} " \
                              f"(e = {st.e[bad[0]]}, dist {out[bad[0], 1]}, margin {dec.margin[bad[0]]})"
        if kind == "hypercube":  # the far flag rejects exactly the faces that are not nearly parallel
            far_rej = ((m >> 8) & 0xFF)[dec.clear & bit]
            assert (far_rej == 0xFF).all(), what
        n_clear += int(dec.clear.sum())
        n_clear_set += int((dec.clear & bit).sum())
        assert hit.sum() >= 50, f"{what}: {int(hit.sum())} figure hits"
        if st.label in ("tangent", "behind"):
            near = np.abs(st.e) <= 1e-4
        elif st.label == "band":
            # where the band's edge decides: the ball test passed, and the slack 8e-6 a is below the band's width
            near = (np.abs(st.e) >= 5e-3) & dec.past_ball & (dec.a <= 100.0 * ball.r2m)
        elif st.label == "hyper_parallel":
            near, bit = bit, skipped
        else:
            continue
        share = bit[near].mean()
        print(f"{what}: {int(near.sum())} rays at the boundary, skip share {share:.3f}")
        assert near.sum() >= 50 and 0.1 <= share <= 0.9, what
    print(f"{case}: {n_clear_set} of {n_clear} clearly skippable rays skipped ({n_clear_set / n_clear:.4f})")
    assert n_clear_set >= 0.99 * n_clear


def probe_of(rt4, desc, rays):
    t = rt4.Tracer(device=0, scene=rt4.Scene(desc))
    try:
        return t.debug_bound_skip(rays)
    finally:
        t.close()


def test_probe_zero_where_the_host_disables(rt4):
    """Identically zero for a tiger whose second pair's point is shifted by 1e-3 (perturb's seed % 3 == 0), for axes
    skewed by 1e-5, for radii outside [1e-15, 1e15]; a scene without the figure has zero in its bits."""
    base = rt4.Scene.named("tiger").desc
    rays = np.concatenate([st.rays for st in bb.strata(bb.balls(base)["tiger"], 5, 4000)])
    assert (probe_of(rt4, base, rays) & 2).any()
    assert (probe_of(rt4, base, rays) & ~np.uint32(2)).max() == 0  # no union, no hypercube
    shifted = perturb(rt4, "tiger", 3).desc
    assert not bb.balls(shifted)["tiger"].enabled
    assert probe_of(rt4, shifted, rays).max() == 0
    skewed = rt4.SceneDesc.from_buffer_copy(bytes(base))
    skewed.tigers[0].inner_cyl1.axis1[1] += 1e-5
    assert probe_of(rt4, skewed, rays).max() == 0
    for r in SPECIAL_RADII:
        if 1e-15 <= r <= 1e15:
            continue
        d = rt4.SceneDesc.from_buffer_copy(bytes(base))
        d.tigers[0].inner_cyl1.r = r
        assert probe_of(rt4, d, rays).max() == 0, r
    ubase = rt4.Scene.named("cylinder4d").desc
    urays = np.concatenate([st.rays for st in bb.strata(bb.balls(ubase)["union"], 6, 4000)])
    assert (probe_of(rt4, ubase, urays) & 1).any()
    for r in SPECIAL_RADII:
        if 1e-15 <= r <= 1e15:
            continue
        d = rt4.SceneDesc.from_buffer_copy(bytes(ubase))
        d.unions[0].cylinder1.r = r
        assert probe_of(rt4, d, urays).max() == 0, r


# ------------------------------------------------------------------------------------------ through the trace kernels
RENDER_SCENES = {"tiger": "tiger", "tiger_two_mirrors": "tiger", "all_primitives": "tiger", "cylinder4d": "union"}


def surface_views(rt4, ball, seed):
    """Uniforms of a camera whose focus lies on the inflated ball's surface, a = R2m (1 + e) for e in +-{1e-6, 1e-4},
    at a point outside every band: one view tangent to the ball (b changes sign across the frame), one looking away
    from it. 64x40, 3 spp, 4 bounces."""
    rng = np.random.default_rng(seed)
    while True:
        u = rng.normal(size=4)
        u /= np.linalg.norm(u)
        p = (ball.centre + np.sqrt(ball.r2m) * u).astype(np.float32)
        probe_ray = np.concatenate([p, -u.astype(np.float32)])[None]
        dec = bb.decide(ball, probe_ray)
        if dec.band_e[0] > 0.05 and np.hypot(u[0], u[1]) > 0.3:
            break
    views = []
    for e in (1e-6, -1e-6, 1e-4, -1e-4):
        focus = tuple(float(x) for x in (ball.centre + np.sqrt(ball.r2m * (1.0 + e)) * u).astype(np.float32))
        for name, fi in (("tangent", np.degrees(np.arctan2(-u[1], u[0]))), ("away", np.degrees(np.arctan2(u[0], u[1])))):
            views.append((e, name, rt4.make_uniforms(64, 40, samples=3, reflections=4, seed=int(1000 + 1e7 * abs(e)),
                                                     focus=focus, fi=float(fi))))
    return views


@pytest.mark.parametrize("name", list(RENDER_SCENES))
def test_render_from_the_ball_surface(rt4, oracle, name):
    """Renders (the LUT and the inline sampler, and the primary-reuse path) == the oracle, images and intersection
    counts, with the camera on the ball's surface; the frame's primary rays take both decisions in the probe."""
    scene = rt4.Scene.named(name)
    kind = RENDER_SCENES[name]
    ball = bb.balls(scene.desc)[kind]
    reg = rt4.region(64, 40)
    views = surface_views(rt4, ball, 11)
    ref = [oracle.render(scene.desc, u, reg)[:2] for _, _, u in views]
    for flags in (rt4.FLAG_SAMPLER_LUT, 0, rt4.FLAG_SAMPLER_LUT | rt4.FLAG_PRIMARY_REUSE):
        t = rt4.Tracer(device=0, scene=scene, flags=flags)
        try:
            for (e, view, u), (fc, nc) in zip(views, ref):
                fg = np.zeros((40, 64, 4), np.float32)
                ng = t.render_host(u, reg, fg)
                assert ng == nc, f"{name} flags {flags} e {e} {view}: {ng} intersections, oracle {nc}"
                assert_bits(fg, fc, f"{name} flags {flags} e {e} {view}")
            if flags == 0:
                for e, view, u in views:
                    m = t.debug_bound_skip(denoise_ref.primary_rays(u, reg).reshape(-1, 8))
                    share = ((m & BIT[kind]) != 0).mean()
                    print(f"{name} e {e} {view}: primary rays skipped {share:.3f}")
                    if e < 4e-6:  # a (1 - 4e-6) <= R2m: inside the inflated ball for the kernel, nothing is skipped
                        assert share == 0.0, f"{name} e {e} {view}"
                    elif view == "tangent":
                        assert 0.0 < share < 1.0, f"{name} e {e}: the tangent view takes both decisions"
                    else:
                        assert share > 0.0, f"{name} e {e}: looking away from outside the ball"
        finally:
            t.close()
