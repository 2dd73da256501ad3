"""The premises of the sphere cull (rt4_aux.h SphereCull; rt4_fast.h find_pre, sphere_culled) against the CPU oracle
alone: no GPU. A flaw in the derivation or in its margin shows here; what the kernels decide is test_gpu_cull.py.

Figure-only scenes (scene_builder.compose with one sphere, one cylinder or one union, off-origin centres and tilted
axes), every enabled radius of cull_ref.ENABLED_RADII in place of the figure's own, 20k rays per stratum of cull_ref.
"""
import numpy as np
import pytest

import cull_ref as cr
import scene_builder

N = 20000
FIGURES = {"sphere": (dict(spheres=1), "sphere", 0), "cylinder": (dict(cylinders=1), "cylinder", 0),
           "union": (dict(unions=1), "union", (0, 1))}
CASES = [(k, i) for k in FIGURES for i in range(len(cr.ENABLED_RADII))]
MARGIN_SHARE_CAP = 0.25  # the derivation's own figure is 1/13; thinning K or the 1e-4 of r2m trips this


def test_sin_acos_figure(rt4, oracle):
    """The figure the derivation cites: the oracle's sin_(acos_(c)) is within 1.75e-7 (relative) of sqrt(1 - c^2) in
    float64, over every float of [0.5, 1) and every 64th of [0, 0.5). Measured: 1.7461e-7 at 0x3F7DE737."""
    c = cr.sweep_inputs()
    a, _ = oracle.eval_array(rt4.EVAL_ACOS, c)
    s, _ = oracle.eval_array(rt4.EVAL_SIN, a)
    worst, at = cr.sin_acos_error(c, s)
    print(f"sin(acos(c)) over {len(c)} floats: largest relative error {worst:.4e} at c = 0x{at:08X}")
    assert worst <= cr.SIN_ACOS_BOUND


@pytest.mark.parametrize("kind,ri", CASES)
def test_premise(rt4, oracle, kind, ri):
    """Per figure and enabled radius, with the predicate stated in numpy float32 (cull_ref.predicate32):
      * no ray the predicate culls is a hit of the oracle on the figure-only scene;
      * among the rays within 1e-5 of the threshold (cull_ref.decide: near) it fires on 0.25 .. 0.75 of them;
      * the tangent stratum holds at least 50 hits and 50 misses. Not for r = 1e-15: from any origin that is outside
        (len_po >= SMALL, 3e11 radii away) no float32 direction resolves such a sphere; a ray aimed at it has
        cos_opa = 1 and hits, whatever e is, so the stratum has no misses to offer (the counts are printed);
      * the share of the margin a hit used, (P - r^2) / (T - r^2) over the hits from outside, is at most 0.25. For a
        cylinder P and T are those of the projected ray as the exact test receives it (float32 projection)."""
    kw, fkind, index = FIGURES[kind]
    d = scene_builder.compose(rt4, seed=3, **kw)
    r = cr.ENABLED_RADII[ri]
    if r is not None:
        cr.set_radius(d, fkind, index, r)
    fig = cr.figure_of(d, fkind, index)
    assert fig.enabled
    alone = cr.figure_only(rt4, d, fkind, index)
    n_near = n_fire = 0
    share = 0.0
    for st in cr.strata(fig, 100 * ri + 7, N):
        out, _ = oracle.find_intersection(alone, st.rays)
        hit = out[:, 0] > 0
        dec = cr.decide(fig, st.rays)
        d2, dp, _, _, _, fires = cr.predicate32(fig, st.rays)
        bad = np.flatnonzero(fires & hit)
        what = f"{kind} r={fig.r!r} {st.label}"
        asked = hit & dec.outside & ~dec.miss & (dec.dp >= 0)
        with np.errstate(all="ignore"):
            if fig.a1 is None:
                used = (dec.P - fig.r ** 2) / (dec.T - fig.r ** 2)
            else:  # of the ray the exact test is given: projected in float32 (far along the axes that differs from
                # the exact projection by more than the whole margin), then in float64
                d2, dp = d2.astype(np.float64), dp.astype(np.float64)
                used = (d2 - dp * dp - fig.r ** 2) / (cr.K * d2 + fig.r2m - fig.r ** 2)
        s = float(used[asked].max()) if asked.any() else 0.0
        share = max(share, s)
        print(f"{what}: hits {int(hit.sum())}, culled {int(fires.sum())}, near {int(dec.near.sum())} "
              f"(fired {int((fires & dec.near).sum())}), margin share of the hits {s:.4f}")
        assert bad.size == 0, f"{what}: {bad.size} culled rays hit, first: ray {bad[0]} {st.rays[bad[0]].tolist()} " \
                              f"(e = {st.e[bad[0]]}, dist {out[bad[0], 1]}, margin {dec.margin[bad[0]]})"
        n_near += int(dec.near.sum())
        n_fire += int((fires & dec.near).sum())
        if st.label == "tangent" and fig.r >= 1e-4:
            assert hit.sum() >= 50 and (~hit).sum() >= 50, what
    print(f"{kind} r={fig.r!r}: fired on {n_fire} of {n_near} near rays ({n_fire / max(n_near, 1):.3f}), "
          f"largest margin share {share:.4f}")
    assert n_near >= 20 and 0.25 <= n_fire / n_near <= 0.75
    assert share <= MARGIN_SHARE_CAP


def test_constants(rt4):
    """constants(r) against the host where the two overlap (rt4_debug_sqrt_thresholds: q < lt <=> sqrt(q) < r, so
    d2_out, the smallest q with sqrt(q) >= max(r, SMALL), is lt of that), and the enable limits at both ends."""
    for r in [x for x in cr.ENABLED_RADII if x is not None] + cr.DISABLED_RADII + [1.0, 0.5, 0.7, 37.5, 1e-3, 1e20]:
        d2_out, r2m, enabled = cr.constants(r)
        r32 = np.float32(r)
        if np.isnan(r32):
            assert np.isnan(d2_out) and r2m == np.inf and not enabled
            continue
        m = max(r32, np.float32(cr.SMALL))
        _, lt = rt4.debug_sqrt_thresholds(float(m))
        assert d2_out == lt, (r, d2_out, lt)
        below = np.nextafter(np.float32(d2_out), np.float32(0))
        assert np.sqrt(np.float32(d2_out)) >= m and np.sqrt(below) < m, r
        assert enabled == bool(np.float32(1e-15) <= r32 <= np.float32(1e15)), r
        assert np.isfinite(r2m) == enabled, r
        if enabled:
            assert r2m == float(np.float32(float(r32) ** 2 * (1.0 + 1e-4)))
    assert cr.constants(1e-15)[2] and not cr.constants(cr.next_down32(1e-15))[2]
    assert cr.constants(1e15)[2] and not cr.constants(cr.next_up32(1e15))[2]
    assert cr.constants(1e-15)[0] == cr.constants(cr.SMALL)[0]  # below SMALL the seam is SMALL's
