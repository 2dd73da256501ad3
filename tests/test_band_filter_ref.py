"""The band filters' thresholds against their definition, the library's own searches against it, and the non-vacuity
of band_filter_ref's strata by the oracle alone (no GPU). The kernels are test_gpu_band_filter.py."""
import numpy as np
import pytest

import band_filter_ref as bf
import bound_ball_ref as bb
import scene_builder
from test_gpu_parity import bits_equal

NAMED_RADII = [0.9, 1.0, 1.4]
SEEDED_RADII = [float(r) for r in np.exp(np.random.default_rng(2024).uniform(np.log(0.05), np.log(50.0), 50)).astype(np.float32)]
EDGE_RADII = [float("nan"), 0.0, -0.0, -0.5, 1e-23, 1e-20, 2e-4, 3e-4, 1e20, float("inf")]
RADII = NAMED_RADII + SEEDED_RADII + EDGE_RADII


def same32(a, b):
    return bool(bits_equal(np.array([a], np.float32), np.array([b], np.float32)).all())


def assert_definition(r, g, l, what):
    q = bf.probes(r)
    ok_gt, ok_lt = bf.holds(r, g, l, q)
    assert ok_gt.all(), f"{what}: gt({r!r}) = {g!r} decides q = {q[~ok_gt].tolist()} unlike sqrt(q) > r"
    assert ok_lt.all(), f"{what}: lt({r!r}) = {l!r} decides q = {q[~ok_lt].tolist()} unlike sqrt(q) < r"


@pytest.mark.parametrize("r", RADII, ids=repr)
def test_thresholds_meet_their_definition(r):
    """(q > gt) == (RN(sqrt(q)) > r) and (q < lt) == (RN(sqrt(q)) < r) at every float within 4 ulp of either
    threshold and at +0, the smallest denormal, FLT_MAX, +inf and NaN; RN(sqrt) is monotonic, so that is all q."""
    assert_definition(r, bf.gt(r), bf.lt(r), "band_filter_ref")


@pytest.mark.parametrize("r", RADII, ids=repr)
def test_library_thresholds(rt4, r):
    """rt4_debug_sqrt_thresholds, the searches set_scene runs, gives the definition's values."""
    g, l = rt4.debug_sqrt_thresholds(r)
    assert_definition(r, g, l, "librt4")
    assert same32(g, bf.gt(r)) and same32(l, bf.lt(r)), (r, g, l, float(bf.gt(r)), float(bf.lt(r)))


def _plain_search(r):
    """The search the bounding balls were made with before it became total."""
    r = np.float32(r)
    lo, hi = 0, 0x7F800000
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if np.sqrt(np.array(mid, np.uint32).view(np.float32)) <= r:
            lo = mid
        else:
            hi = mid
    return float(np.array(lo, np.uint32).view(np.float32))


@pytest.mark.parametrize("r", RADII, ids=repr)
def test_bound_ball_ref_in_step(r):
    """bound_ball_ref's restatement of the host's search follows it; for the radii of an enabled ball, [1e-15, 1e15],
    its value is what it was."""
    assert same32(bb.sqrt_gt_threshold(r), bf.gt(r))
    if 1e-15 <= r <= 1e15:
        assert bb.sqrt_gt_threshold(r) == _plain_search(r)


def test_enabled_balls_unchanged(rt4):
    for name in ("tiger", "cylinder4d", "all_primitives"):
        for kind, ball in bb.balls(rt4.Scene.named(name).desc).items():
            if kind != "hypercube":
                assert ball.enabled and np.isfinite(ball.r2m), (name, kind)
    t = rt4.Scene.named("tiger").desc.tigers[0]
    r_in, r_out = float(t.inner_cyl1.r), float(t.outer_cyl1.r)
    assert bb.balls(rt4.Scene.named("tiger").desc)["tiger"].r2 == r_out * r_out + _plain_search(r_out) and r_in < r_out
    for r in (float("nan"), float("inf"), -0.5):  # g = +inf or negative: the ball stays off
        d = rt4.SceneDesc.from_buffer_copy(bytes(rt4.Scene.named("tiger").desc))
        d.tigers[0].outer_cyl1.r = r
        ball = bb.balls(d)["tiger"]
        assert not ball.enabled and ball.r2m == np.inf, r


# ------------------------------------------------------------------------------------------- the strata
def figure_scenes(rt4):
    """name -> scene: the two axis-aligned reference figures and two rotated, off-origin ones (the union's radii
    unequal)."""
    return {"tiger": rt4.Scene.named("tiger").desc, "cylinder4d": rt4.Scene.named("cylinder4d").desc,
            "rotated_tiger": scene_builder.compose(rt4, tigers=1, seed=3),
            "rotated_union": scene_builder.compose(rt4, unions=1, seed=4)}


@pytest.mark.parametrize("name", ["tiger", "cylinder4d", "rotated_tiger", "rotated_union"])
def test_aimed_strata_are_not_vacuous(rt4, oracle, name):
    """By the oracle alone, on the scene that holds only the figure, for every seam kind:
      * every stratum of a signed e with |e| <= E_NOISE = 2^-22 keeps the aimed hit for 15 % to 85 % of its rays: both
        outcomes occur inside the rounding noise, on either side of the threshold;
      * e = +1e-3 outside an outer radius and e = -1e-3 inside an inner one keep none, the other side some."""
    d = figure_scenes(rt4)[name]
    u = d.unions[0] if d.n_unions else None
    assert u is None or name != "rotated_union" or u.cylinder1.r != u.cylinder2.r
    for sm in bf.seams(d):
        alone = bb.figure_only(rt4, d, sm.kind)
        for e in [e for e in bf.E_OCTAVES if abs(e) <= bf.E_NOISE]:
            st = bf.aimed(sm, 11, 10000, e)
            out, col = oracle.find_intersection(alone, st.rays)
            share = float(bf.aimed_hit(sm, st, out, col).mean())
            print(f"{name} {sm.name} e = {e}: kept {share:.3f}")
            assert 0.15 <= share <= 0.85, f"{name} {sm.name} e = {e}: kept {share:.3f}"
        wrong = bf.E_CLEAR if sm.rel == "gt" else -bf.E_CLEAR
        for e in (wrong, -wrong):
            st = bf.aimed(sm, 12, 10000, e)
            out, col = oracle.find_intersection(alone, st.rays)
            n = int(bf.aimed_hit(sm, st, out, col).sum())
            print(f"{name} {sm.name} e = {e}: kept {n} of 10000")
            assert (n == 0) if e == wrong else (n >= 1500), f"{name} {sm.name} e = {e}: kept {n}"


@pytest.mark.parametrize("name", ["tiger", "cylinder4d"])
def test_exact_stratum(rt4, oracle, name):
    """Every target q of the exact stratum is reached (q as the kernel's op order gives it, in exactly rounded
    float32), the oracle's answer on the figure alone is the definition's for every ray, and each seam's stratum holds
    both answers: q on the threshold and one float past it decide differently."""
    d = figure_scenes(rt4)[name]
    for sm in bf.seams(d):
        st, table = bf.exact(sm)
        missed = [label for label, _, ok in table if not ok]
        print(f"{name} {sm.name}: {len(table) - len(missed)} of {len(table)} targets reached, {len(st.rays)} rays")
        assert not missed, f"{name} {sm.name}: {missed}"
        out, col = oracle.find_intersection(bb.figure_only(rt4, d, sm.kind), st.rays)
        hit = (out[:, 0] > 0) & (col == np.array(sm.faces[-1].color, np.float32)).all(1)
        want = bf.exact_kept(sm, d, st)
        assert (hit == want).all(), f"{name} {sm.name}: q = {st.e[hit != want].tolist()}"
        assert hit.any() and not hit.all()


CASES = [(f, r) for f in bf.FIELDS for r in bf.SPECIAL_RADII]


@pytest.mark.parametrize("field,radius", CASES, ids=[f"{f}={r!r}" for f, r in CASES])
def test_special_radius_cases_count(rt4, oracle, field, radius):
    """special_case_checked's conditions, by the oracle alone; every target of the changed threshold's exact stratum
    that is a value of dot(v, v) is reached."""
    d, rays, c, cc, info, parts = bf.special_case_checked(rt4, oracle, field, radius)
    print(f"{field} = {radius!r}: {info}")
    for sm, _, table in parts:
        for label, q, ok in table:
            assert ok or q is None, (sm.name, label, q)  # None: below +0 or above +inf, no value of dot(v, v)


@pytest.mark.parametrize("name", ["tiger", "tiger_two_mirrors", "all_primitives", "cylinder4d"])
def test_zoom_views_show_the_seam(rt4, oracle, name):
    """zoom_cases' condition, by the oracle alone: every seam kind of the scene has a view, and at each zoom the
    frame without reflections has two pixel values of at least 20 % of the pixels each."""
    cases = bf.zoom_cases(rt4, oracle, name)
    d = rt4.Scene.named(name).desc
    assert len(cases) == 3 * len(bf.seams(d))
    for label, u, share in cases:
        print(f"{name} {label}: smaller class {share:.3f}")
