"""The bounding-ball skips of the tiger, the cylinders union and the hypercube (rt4_fast.h far_from,
hypercube_cand; rt4_aux.h BoundBall), restated in float64 from the scene description alone, and rays aimed at the
boundaries of those skips. A plain helper, not a fixture: test_bound_ball_ref.py (CPU, against the oracle) and
test_gpu_bound_ball.py (against the kernels and their probe, rt4_debug_bound_skip) use it.

balls(desc) follows the host's construction (rt4_trace.hip: the `bound` lambda and the hyper_bound block). The
stored floats (centre, axes, R2m, band edges) are rounded as the host rounds them; everything a ray is measured
with afterwards is float64.

The decision of a ray (decide()):
  pc = c - p, a = |pc|^2, b = pc.d, l2 = |d|^2
  tiger, union:  skip  <=>  not in a band  and  a < 1e30  and  1e-30 < l2 < 1e30  and
                            (a - 4e-6 a - R2m) l2 > max(b, 0)^2
                 (b > 0: the line clears the inflated ball; b <= 0: the origin is outside it, the ball behind)
                 in a band: d + 8e-6 a >= lo and d - 8e-6 a <= hi for one of the four [lo, hi] = r^2 [0.99, 1.01],
                 d = a - dB for the two radii around plane A, dB = (pc.a1)^2 + (pc.a2)^2 for those around plane B
  hypercube:     far   <=>  the same without the bands and without the clamp of b (the line test only; the faces
                            that look away are rejected by h < 0 || cos_dn < 0 anyhow)
margin = ((a - 4e-6 a - R2m) l2 - max(b, 0)^2) / (a l2): the decision's distance from its boundary, relative to the
size of the terms the fp32 test subtracts (a l2 and b^2 <= a l2), which is what its rounding error scales with.

Every generator takes (ball, seed, n) and returns a Stratum: float32 rays (point, direction; directions are not all
of unit length), the stratum's name and the nominal relative offset e each ray was built with (NaN where a ray has
none). The rays are rounded to float32, so a nominal |e| below ~1e-7 only scatters them across the boundary.
"""
import collections

import numpy as np

Ball = collections.namedtuple(
    "Ball", "kind centre a1 a2 b1 b2 r2 r2m band radii enabled norms points")
Stratum = collections.namedtuple("Stratum", "rays label e")

F32 = np.float32
CLEAR = 1e-6          # "clearly": the margin above, or a relative distance from a band edge / cosine bound
COS2_MIN = 1e-12      # hypercube_cand: faces with cos_dn^2 < 1e-12 l2 keep the exact test
BAND_SLACK = 8e-6     # far_from: each band is widened by this times a (rt4_fast.h BAND_SLACK)


def _f64(v, n=4):
    return np.array([float(v[i]) for i in range(n)], np.float64)


def _next_up32(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def sqrt_gt_threshold(r):
    """The host's sqrt_gt_threshold: the largest float32 x >= 0 with RN(sqrt(x)) <= r; +inf for a NaN or infinite r
    and -1 for a negative one (no q = dot(v, v) is above the former, every q is above the latter). The definition it
    serves and its tests are band_filter_ref.gt and test_band_filter_ref.py."""
    r = F32(r)
    if np.isnan(r) or r == F32(np.inf):
        return float("inf")
    if r < 0:
        return -1.0
    lo, hi = 0, 0x7F800000
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if np.sqrt(np.array(mid, np.uint32).view(F32)) <= r:
            lo = mid
        else:
            hi = mid
    return float(np.array(lo, np.uint32).view(F32))


def _orthonormal(vs, tol=1e-6):
    for i in range(len(vs)):
        for j in range(i, len(vs)):
            d = float(np.dot(vs[i], vs[j]))
            if not np.isfinite(d) or abs(d - (1.0 if i == j else 0.0)) > tol:
                return False
    return True


def _pair_ball(kind, c1, c2, r2, r_a, r_b):
    """The `bound` lambda: cylinders c1 (plane A) and c2 (plane B), R^2 = r2, the radii around each plane."""
    centre, p2 = _f64(c1.point), _f64(c2.point)
    ax = [_f64(c1.axis1), _f64(c1.axis2), _f64(c2.axis1), _f64(c2.axis2)]
    radii = [float(F32(r)) for r in (r_a[0], r_a[1], r_b[0], r_b[1])]
    band = []
    with np.errstate(over="ignore", invalid="ignore"):  # a huge radius rounds to +inf, as on the host
        for r in radii:
            band += [float(F32(r * r * 0.99)), float(F32(r * r * 1.01))]
    ok = bool((centre == p2).all()) and bool(np.isfinite(r2))
    ok = ok and all(F32(r) >= F32(1e-15) and F32(r) <= F32(1e15) for r in radii)
    ok = ok and _orthonormal(ax)
    ok = ok and bool(np.isfinite(centre).all() and (np.abs(centre) < float(F32(1e15))).all())
    r2m = _next_up32(r2 * (1.0 + 1e-3)) if ok and r2 < 1e30 else np.inf
    return Ball(kind, centre, ax[0], ax[1], ax[2], ax[3], r2, r2m, np.array(band), radii, bool(np.isfinite(r2m)),
                None, None)


def _hyper_ball(h):
    pts = np.array([_f64(c.point) for c in h.cubes])
    c = np.zeros(4)
    for k in range(8):
        c += pts[k] / 8.0
    r2, cmax, ok = 0.0, 0.0, True
    for k in range(8):
        if not ok:
            break
        cu = h.cubes[k]
        ok = _orthonormal([_f64(cu.norm), _f64(cu.x), _f64(cu.y), _f64(cu.z)])
        if not ok:
            break
        r = float(cu.r)
        r2 = max(r2, float(((pts[k] - c) ** 2).sum()) + 3.0 * r * r)
        cmax = max(cmax, float(np.abs(pts[k]).max()))
        ok = bool(np.isfinite(r)) and r >= 0.0 and cmax < 1e15
    centre = c.astype(F32).astype(np.float64)
    r2m = _next_up32(r2 * (1.0 + 1e-3) + 1e-10 * cmax * cmax) if ok else np.inf
    eye = np.eye(4)
    return Ball("hypercube", centre, eye[0], eye[1], eye[2], eye[3], r2, r2m, np.zeros(0), [], bool(np.isfinite(r2m)),
                np.array([_f64(cu.norm) for cu in h.cubes]), pts)


def balls(desc):
    """{'union' | 'tiger' | 'hypercube': Ball} of figure 0 of each kind the scene has (the kernels' balls)."""
    out = {}
    if desc.n_unions > 0:
        u = desc.unions[0]
        g = sqrt_gt_threshold(u.cylinder2.r)
        r1, r2 = float(u.cylinder1.r), float(u.cylinder2.r)
        out["union"] = _pair_ball("union", u.cylinder1, u.cylinder2, max(r1 * r1, r2 * r2) + g,
                                  (u.cylinder1.r, u.cylinder1.r), (u.cylinder2.r, u.cylinder2.r))
    if desc.n_tigers > 0:
        t = desc.tigers[0]
        g1, g2 = sqrt_gt_threshold(t.outer_cyl2.r), sqrt_gt_threshold(t.outer_cyl1.r)
        o1 = max(abs(float(t.inner_cyl1.r)), abs(float(t.outer_cyl1.r)))
        o2 = max(abs(float(t.inner_cyl2.r)), abs(float(t.outer_cyl2.r)))
        out["tiger"] = _pair_ball("tiger", t.inner_cyl1, t.inner_cyl2, max(o1 * o1 + g1, o2 * o2 + g2),
                                  (t.inner_cyl1.r, t.outer_cyl1.r), (t.inner_cyl2.r, t.outer_cyl2.r))
    if desc.n_hypercubes > 0:
        out["hypercube"] = _hyper_ball(desc.hypercubes[0])
    return out


Decision = collections.namedtuple(
    "Decision", "a b l2 line2 d_a d_b band_e in_band guards past_ball skip margin clear cos2 rejected")


def decide(ball, rays):
    """The float64 restatement of the decision for float32 rays (n, 8); see the module docstring.
    line2: squared distance of the ray's LINE to the centre. band_e: the smallest |d^2 / r^2 - 1| over the four
    radii, d the origin's distance to the cylinder's axes plane as the exact test projects it (inf for the
    hypercube); in_band: the kernel's band test; past_ball: the ball part of the decision alone (guards and line
    test). clear: in the skip region with margin > CLEAR, farther than
    CLEAR (relative, and CLEAR a for the fp32 dots) from every widened band edge, and for the hypercube no face
    cosine with cos^2 < COS2_MIN (1 + 1e-5)^2 l2. cos2 (n, 8), rejected (n, 8): the hypercube's faces (None otherwise)."""
    rays = np.asarray(rays, F32).astype(np.float64)
    p, d = rays[:, :4], rays[:, 4:]
    with np.errstate(all="ignore"):
        pc = ball.centre - p
        a, b, l2 = (pc * pc).sum(1), (pc * d).sum(1), (d * d).sum(1)
        guards = (a < float(F32(1e30))) & (l2 > float(F32(1e-30))) & (l2 < float(F32(1e30)))
        line2 = a - b * b / l2
        bp = np.maximum(b, 0.0) if ball.kind != "hypercube" else b
        s = (a - 4e-6 * a - ball.r2m) * l2 - bp * bp
        margin = s / (a * l2)
        n = len(rays)
        if ball.kind == "hypercube":
            d_a = d_b = np.full(n, np.nan)
            band_e, in_band, off_edges = np.full(n, np.inf), np.zeros(n, bool), np.ones(n, bool)
            vec_n = -ball.norms  # (8, 4)
            h = ((ball.points[None] - p[:, None]) * vec_n[None]).sum(2)
            cos = (d[:, None] * vec_n[None]).sum(2)
            cos2 = cos * cos
            skip = guards & (s > 0)
            rejected = (h < 0) | (cos < 0) | (skip[:, None] & (cos2 >= COS2_MIN * l2[:, None]))
            clear = skip & (margin > CLEAR) & (cos2 >= COS2_MIN * (1 + 1e-5) ** 2 * l2[:, None]).all(1)
        else:
            u1, u2 = (pc * ball.a1).sum(1), (pc * ball.a2).sum(1)
            d_b = u1 * u1 + u2 * u2  # the kernel's squared distance to plane B: the coordinates in plane A
            d_a = a - d_b
            # what the exact test measures: the rest of pc after each plane's own axes are projected out. With axes
            # orthonormal to eps that differs from d_a, d_b by up to ~4 eps a: first order in eps, times a, not r^2.
            v1, v2 = (pc * ball.b1).sum(1), (pc * ball.b2).sum(1)
            perp = [((pc - u1[:, None] * ball.a1 - u2[:, None] * ball.a2) ** 2).sum(1),
                    ((pc - v1[:, None] * ball.b1 - v2[:, None] * ball.b2) ** 2).sum(1)]
            sl = BAND_SLACK * a
            band_e, in_band, off_edges = np.full(n, np.inf), np.zeros(n, bool), np.ones(n, bool)
            for q in range(4):
                dist = d_a if q < 2 else d_b
                lo, hi, r2 = ball.band[2 * q], ball.band[2 * q + 1], ball.radii[q] ** 2
                in_band |= (dist + sl >= lo) & (dist - sl <= hi)
                band_e = np.minimum(band_e, np.abs(perp[q // 2] / r2 - 1.0))
                off_edges &= (dist + sl + CLEAR * a < lo * (1 - CLEAR)) | (dist - sl - CLEAR * a > hi * (1 + CLEAR))
            skip = ~in_band & guards & (s > 0)
            clear = skip & (margin > CLEAR) & off_edges
            cos2 = rejected = None
        if not ball.enabled:
            skip, clear = np.zeros(n, bool), np.zeros(n, bool)
    return Decision(a, b, l2, line2, d_a, d_b, band_e, in_band, guards, guards & (s > 0), skip, margin, clear, cos2,
                    rejected)


# ------------------------------------------------------------------------------------------------- generators
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _perp(rng, u):
    """A random unit vector orthogonal to each row of u (unit rows)."""
    v = rng.normal(size=u.shape)
    v -= (v * u).sum(1, keepdims=True) * u
    return _unit(v)


def _signed_e(rng, n, lo, hi, zero_share):
    e = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(lo, hi, n)
    if zero_share:
        e[: n // zero_share] = 0.0
    return e


def _lengths(rng, n):
    """Direction lengths: half of them 1, the others 1/4 .. 4."""
    return np.where(rng.random(n) < 0.5, 1.0, np.exp(rng.uniform(np.log(0.25), np.log(4.0), n)))[:, None]


def _redirect(p32, c, target_b_over_pc, v):
    """Directions from the ROUNDED origins: unit d with pc.d / |pc| = beta, the rest along v (made orthogonal)."""
    pc = c - p32.astype(np.float64)
    u = _unit(pc)
    v = v - (v * u).sum(1, keepdims=True) * u
    v = _unit(v)
    beta = target_b_over_pc[:, None]
    return beta * u + np.sqrt(np.maximum(1.0 - beta * beta, 0.0)) * v


def _corner_dirs(ball, rng, n):
    """Unit vectors from the centre towards the figure's outermost points (both planes' coordinates at their
    largest radius): where the figure comes closest to the ball's surface."""
    if ball.kind == "hypercube":  # its vertices
        return _unit(np.where(rng.random((n, 4)) < 0.5, -1.0, 1.0))
    al, be = rng.uniform(0, 2 * np.pi, (n, 1)), rng.uniform(0, 2 * np.pi, (n, 1))
    ra, rb = max(ball.radii[:2]), max(ball.radii[2:])
    if ball.kind == "union":  # both of its filters use cylinder2's radius: R^2 = max(r1, r2)^2 + r2^2
        ra = max(ra, rb)
    return _unit(rb * (np.cos(al) * ball.a1 + np.sin(al) * ball.a2) + ra * (np.cos(be) * ball.b1 + np.sin(be) * ball.b2))


def tangent(ball, seed, n):
    """Origins at a = k R2m, k log-uniform over [1.2, 1e8] (at the upper end the 4e-6 a term dominates); the line
    passes the centre at distance^2 (R2m + 4e-6 a)(1 + e), |e| log-uniform over 1e-8..1e-2, both signs, a
    sixteenth with e = 0; the ball is ahead."""
    rng = np.random.default_rng(seed)
    k = np.exp(rng.uniform(np.log(1.2), np.log(1e8), n))
    e = _signed_e(rng, n, -8, -2, 16)
    # w: the direction from the centre to the line's nearest point; three quarters of the lines graze the ball where
    # the figure comes nearest to its surface, so that the ones just inside it (e < -1e-3) hit the figure
    w = _unit(rng.normal(size=(n, 4)))
    w[n // 4:] = _corner_dirs(ball, rng, n - n // 4)
    a = k * ball.r2m
    rho2 = (ball.r2m + 4e-6 * a) * (1.0 + e)
    p32 = (ball.centre + np.sqrt(rho2)[:, None] * w - np.sqrt(a - rho2)[:, None] * _perp(rng, w)).astype(F32)
    a = ((ball.centre - p32.astype(np.float64)) ** 2).sum(1)  # of the rounded origin; the direction follows it
    sin2 = np.minimum((ball.r2m + 4e-6 * a) * (1.0 + e) / a, 1.0)
    d = _redirect(p32, ball.centre, np.sqrt(1.0 - sin2), w)
    return Stratum(np.concatenate([p32, (d * _lengths(rng, n)).astype(F32)], axis=1), "tangent", e)


def behind(ball, seed, n):
    """Origins on the inflated ball's surface, a = R2m (1 + e) / (1 - 4e-6) with tangent's e; directions with
    b = +-|pc| |d| 10^U(-9, -1), an eighth with b = +-0 exactly (the origin displaced along one coordinate axis,
    that component of the direction +-0). Where b < 0 and b^2 / l2 > a - R2m the line passes through the ball
    behind the origin. Half of the origins lie where the figure comes nearest to the ball's surface."""
    rng = np.random.default_rng(seed)
    e = _signed_e(rng, n, -8, -2, 16)
    rng.shuffle(e)
    a = ball.r2m * (1.0 + e) / (1.0 - 4e-6)
    u = _unit(rng.normal(size=(n, 4)))
    u[n // 2:] = _corner_dirs(ball, rng, n - n // 2)
    n0 = n // 8
    axis = rng.integers(0, 4, n0)
    u[:n0] = 0.0
    u[np.arange(n0), axis] = np.where(rng.random(n0) < 0.5, -1.0, 1.0)
    p = ball.centre + np.sqrt(a)[:, None] * u
    p[:n0] = np.where(u[:n0] != 0.0, p[:n0], ball.centre.astype(F32).astype(np.float64))
    p32 = p.astype(F32)
    beta = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-9, -1, n)
    d = _redirect(p32, ball.centre, beta, rng.normal(size=(n, 4))) * _lengths(rng, n)
    d32 = d.astype(F32)
    d0 = rng.normal(size=(n0, 4)).astype(F32)
    d0[np.arange(n0), axis] = np.where(rng.random(n0) < 0.5, F32(-0.0), F32(0.0))
    d32[:n0] = d0
    return Stratum(np.concatenate([p32, d32], axis=1), "behind", e)


def _figure_points(ball, rng, n):
    """Points on or near the figure's surfaces."""
    if ball.kind == "hypercube":
        r = float(np.abs(ball.points - ball.centre).max())
        q = rng.uniform(-1.0, 1.0, (n, 4))
        k = rng.integers(0, 4, n)
        q[np.arange(n), k] = np.where(rng.random(n) < 0.5, -1.0, 1.0)
        return ball.centre + r * q
    al, be = rng.uniform(0, 2 * np.pi, (n, 1)), rng.uniform(0, 2 * np.pi, (n, 1))
    ra = np.array(ball.radii[:2])[rng.integers(0, 2, n)][:, None]
    rb = np.array(ball.radii[2:])[rng.integers(0, 2, n)][:, None]
    # distance ra from plane A's axes (coordinates in plane B), rb from plane B's axes
    mix = rng.uniform(0.0, 1.0, (n, 1))
    return (ball.centre + ra * (np.cos(be) * ball.b1 + np.sin(be) * ball.b2)
            + rb * mix * (np.cos(al) * ball.a1 + np.sin(al) * ball.a2))


def inside(ball, seed, n):
    """Origins inside the inflated ball, a quarter of them on its surface, and lines through the figure: the
    stratum where the skip must not fire and the figure's hits are plentiful."""
    rng = np.random.default_rng(seed)
    rad = np.sqrt(ball.r2m) * rng.uniform(0, 1, (n, 1)) ** 0.25
    rad[: n // 4] = np.sqrt(ball.r2m)
    p32 = (ball.centre + rad * _unit(rng.normal(size=(n, 4)))).astype(F32)
    d = _unit(_figure_points(ball, rng, n) - p32.astype(np.float64) + rng.normal(0, 1e-3, (n, 4)))
    return Stratum(np.concatenate([p32, (d * _lengths(rng, n)).astype(F32)], axis=1), "inside",
                   np.full(n, np.nan))


def band(ball, seed, n):
    """Origins whose squared distance to an axes plane is r^2 (1 + e) for each of the four radii, |e| log-uniform
    over 1e-7..2e-2 with both signs (it straddles the band edges 0.99 and 1.01 and the cylinder itself), 2..400
    ball radii out along that plane's axes; random directions, pointing away included, but for half of the origins
    within ten ball radii, which look at the figure. Not for the hypercube."""
    rng = np.random.default_rng(seed)
    e = _signed_e(rng, n, -7, np.log10(2e-2), 0)
    q = rng.integers(0, 4, n)
    r = np.array(ball.radii)[q][:, None]
    plane_a = (q < 2)[:, None]  # radii 0, 1: cylinders around plane A; the distance lies in plane B
    th, ph = rng.uniform(0, 2 * np.pi, (n, 1)), rng.uniform(0, 2 * np.pi, (n, 1))
    across = np.where(plane_a, np.cos(th) * ball.b1 + np.sin(th) * ball.b2, np.cos(th) * ball.a1 + np.sin(th) * ball.a2)
    along = np.where(plane_a, np.cos(ph) * ball.a1 + np.sin(ph) * ball.a2, np.cos(ph) * ball.b1 + np.sin(ph) * ball.b2)
    out = np.sqrt(ball.r2m) * np.exp(rng.uniform(np.log(2.0), np.log(400.0), (n, 1)))
    p32 = (ball.centre + r * np.sqrt(1.0 + e)[:, None] * across + out * along).astype(F32)
    d = _unit(rng.normal(size=(n, 4)))
    # every other ray within ten ball radii looks at the figure instead: finite hits from these origins too (from
    # farther out the exact test's own fp32 distance no longer resolves the figure to the ball's 1e-3)
    aimed = (np.arange(n) % 2 == 1) & (out[:, 0] <= 10.0 * np.sqrt(ball.r2m))
    d[aimed] = _unit(_figure_points(ball, rng, n) - p32.astype(np.float64))[aimed]
    return Stratum(np.concatenate([p32, (d * _lengths(rng, n)).astype(F32)], axis=1), "band", e)


def guards(ball, seed, n):
    """The range guards of the fp32 test: directions scaled so that l2 runs over 1e-32..1e32, a quarter within a
    few ulp of 1e-30 and 1e30; a quarter of the origins with a either side of 1e30. The rays point at the figure
    or past the ball, so both a hit and a skip depend on the guard."""
    rng = np.random.default_rng(seed)
    base = tangent(ball, seed + 1, n).rays.astype(np.float64)
    aim = inside(ball, seed + 2, n).rays.astype(np.float64)
    k = np.exp(rng.uniform(np.log(1.5), np.log(50.0), (n, 1)))
    aim[:, :4] = ball.centre + np.sqrt(k * ball.r2m) * _unit(rng.normal(size=(n, 4)))
    aim[:, 4:] = _unit(_figure_points(ball, rng, n) - aim[:, :4])
    rays = np.where((np.arange(n) % 2 == 0)[:, None], base, aim)
    d = _unit(rays[:, 4:])
    l2 = 10.0 ** rng.uniform(-32, 32, n)
    edge = np.where(rng.random(n) < 0.5, 1e-30, 1e30) * (1.0 + rng.integers(-4, 5, n) * 2.0 ** -23)
    l2 = np.where(rng.random(n) < 0.25, edge, l2)
    rays[:, 4:] = d * np.sqrt(l2)[:, None]
    far = np.arange(n) % 4 == 3
    a_far = 1e30 * (1.0 + rng.integers(-4, 5, n) * 2.0 ** -23) * np.where(rng.random(n) < 0.5, 1.0, 10.0 ** rng.uniform(-1, 1, n))
    rays[far, :4] = ball.centre - d[far] * np.sqrt(a_far[far])[:, None]  # the ball straight ahead, from far away
    return Stratum(rays.astype(F32), "guards", np.full(n, np.nan))


def hyper_parallel(ball, seed, n):
    """Hypercube only: tangent and behind rays whose direction has one face cosine at +-1e-6 (1 + e2) |d|,
    |e2| over 1e-7..1e-1 with both signs, the two sides of the nearly-parallel carve-out; an eighth with that
    component +0 or -0."""
    rng = np.random.default_rng(seed)
    t, bh = tangent(ball, seed + 1, n - n // 2), behind(ball, seed + 2, n // 2)
    rays = np.concatenate([t.rays, bh.rays]).astype(np.float64)
    e = np.concatenate([t.e, bh.e])
    k = rng.integers(0, 4, n)
    e2 = _signed_e(rng, n, -7, -1, 0)
    cos = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 1e-6 * (1.0 + e2)
    d = rays[:, 4:]
    d[np.arange(n), k] = 0.0
    length = np.linalg.norm(d, axis=1)
    d[np.arange(n), k] = cos * length  # |d|^2 changes by 1e-12 relative: below the cosine's own rounding
    zero = rng.random(n) < 0.125
    d[zero, k[zero]] = np.where(rng.random(int(zero.sum())) < 0.5, -0.0, 0.0)
    return Stratum(rays.astype(F32), "hyper_parallel", e)


def strata(ball, seed, n):
    """Every stratum that applies to the ball's kind, n rays each."""
    gens = [tangent, behind, inside, guards] + ([hyper_parallel] if ball.kind == "hypercube" else [band])
    return [g(ball, seed + 10 * i, n) for i, g in enumerate(gens)]


def figure_only(rt4, desc, kind):
    """A copy of the scene with figure 0 of `kind` as its only object and only group: what the skipped test alone
    would report."""
    d = rt4.SceneDesc.from_buffer_copy(bytes(desc))
    keep = {"union": "n_unions", "tiger": "n_tigers", "hypercube": "n_hypercubes"}[kind]
    for f in ("n_spaces", "n_spheres", "n_cylinders", "n_unions", "n_hypercubes", "n_tigers"):
        setattr(d, f, 1 if f == keep else 0)
    gk = {"union": rt4.GROUP_CYLINDERS_UNION, "tiger": rt4.GROUP_TIGER, "hypercube": rt4.GROUP_HYPERCUBE}[kind]
    d.n_groups = 1
    g = d.groups[0]
    g.kind, g.first, g.count, g.outer, g.new_first = gk, 0, 1, (1 if kind == "union" else 0), 1
    return d
