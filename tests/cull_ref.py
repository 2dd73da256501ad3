"""The sphere cull of the spheres, the cylinders and the unions' cylinders (rt4_aux.h SphereCull; rt4_fast.h find_pre,
sphere_culled, cyl_cand_cull), restated from the derivation and from shader.frag:197-267, and rays aimed at its
seams. A plain helper, not a fixture: test_cull_ref.py (CPU, against the oracle) and test_gpu_cull.py (against the
kernels and their probe, rt4_debug_cull) use it.

The cull of a ray, in the quantities of sphere_intersection (po = centre - point, for a cylinder of the ray projected
onto its 2-plane with the direction normalised there):
  d2 = po.po, dp = po.drct, P = d2 - dp^2, T = K d2 + r2m, K = 4e-6
  culled  <=>  d2 >= d2_out  and  (dp < 0  or  P > T)
d2 >= d2_out is len_po >= max(r, SMALL) without the square root; dp < 0 is the shader's own early-out (:206), P > T
the margin test whose exactness rt4_aux.h derives. A cylinder whose projection misses (:253, :257) is never asked.

constants(r)      d2_out, r2m and the enabled flag as the host must make them.
decide(fig, rays) the decision in float64 on the float32 rays as given.
predicate32(..)   the predicate in float32 with the kernels' fused dots, op for op (numpy).
strata(..)        labelled strata of rays on the seams.
"""
import collections

import numpy as np

from denoise_ref import dot4, fma32

F32 = np.float32
SMALL = float(F32(0.0003))           # SMALL_FLOAT, shader.frag:24
K = float(F32(4e-6))                 # SPHERE_CULL_K
R_MIN, R_MAX = F32(1e-15), F32(1e15)  # the host's enable limits

Figure = collections.namedtuple("Figure", "kind index word bit centre a1 a2 r d2_out r2m enabled")
Stratum = collections.namedtuple("Stratum", "rays label e")
Decision = collections.namedtuple("Decision", "d2 dp P T margin outside miss clear near tangent_margin")


def next_up32(x):
    return float(np.nextafter(F32(x), F32(np.inf)))


def next_down32(x):
    return float(np.nextafter(F32(x), F32(-np.inf)))


ENABLED_RADII = [None, 1e-15, 2e-4, 3e-4, next_up32(3e-4), float(F32(1.0) / F32(3.0)), 1e3, 1e15]  # None: the scene's own
DISABLED_RADII = [next_down32(1e-15), next_up32(1e15), 0.0, -0.5, float("nan"), float("inf")]


def constants(r):
    """(d2_out, r2m, enabled) of a radius: d2_out the smallest float32 whose correctly rounded sqrt is >= max(r, SMALL)
    (NaN for a NaN radius), r2m = RN(r^2 (1 + 1e-4)) iff 1e-15 <= r <= 1e15 and +inf otherwise."""
    r = F32(r)
    if np.isnan(r):
        return float("nan"), float("inf"), False
    m = max(r, F32(SMALL))
    lo, hi = 0, 0x7F800000  # sqrt(+0) < m <= sqrt(+inf)
    while hi - lo > 1:
        mid = lo + (hi - lo) // 2
        if np.sqrt(np.array(mid, np.uint32).view(F32)) >= m:
            hi = mid
        else:
            lo = mid
    d2_out = float(np.array(hi, np.uint32).view(F32))
    enabled = bool(R_MIN <= r <= R_MAX)
    r2m = float(F32(float(r) * float(r) * (1.0 + 1e-4))) if enabled else float("inf")
    return d2_out, r2m, enabled


def _f64(v):
    return np.array([float(v[i]) for i in range(4)], np.float64)


def _figure(kind, index, word, bit, centre, a1, a2, r):
    d2_out, r2m, enabled = constants(r)
    return Figure(kind, index, word, bit, _f64(centre), None if a1 is None else _f64(a1),
                  None if a2 is None else _f64(a2), float(F32(r)), d2_out, r2m, enabled)


def figures(desc):
    """Every figure of the scene that the cull serves, with its place in rt4_debug_cull's output (word, bit)."""
    out = []
    for i in range(desc.n_spheres):
        s = desc.spheres[i]
        out.append(_figure("sphere", i, 0, i, s.center, None, None, s.r))
    for i in range(desc.n_cylinders):
        c = desc.cylinders[i]
        out.append(_figure("cylinder", i, 1, i, c.point, c.axis1, c.axis2, c.r))
    for u in range(desc.n_unions):
        for k, c in enumerate((desc.unions[u].cylinder1, desc.unions[u].cylinder2)):
            out.append(_figure("union", (u, k), 1, 16 + 2 * u + k, c.point, c.axis1, c.axis2, c.r))
    return out


def figure_of(desc, kind, index):
    return next(f for f in figures(desc) if f.kind == kind and f.index == index)


def set_radius(desc, kind, index, r):
    """Puts the radius r on one object of the scene (in place)."""
    if kind == "sphere":
        desc.spheres[index].r = r
    elif kind == "cylinder":
        desc.cylinders[index].r = r
    else:
        (desc.unions[index[0]].cylinder1 if index[1] == 0 else desc.unions[index[0]].cylinder2).r = r


def figure_only(rt4, desc, kind, index):
    """A copy of the scene with that figure as its only object and group: what the culled test alone would report.
    A union's cylinder stands alone as a plain cylinder (shader.frag:285, :289 call cylinder_intersection with
    outer = true on it; the union's filter comes after, and the other cylinder's hit is not the culled test's)."""
    d = rt4.SceneDesc.from_buffer_copy(bytes(desc))
    for f in ("n_spaces", "n_spheres", "n_cylinders", "n_unions", "n_hypercubes", "n_tigers"):
        setattr(d, f, 0)
    d.n_groups = 1
    g = d.groups[0]
    if kind == "sphere":
        d.n_spheres = 1
        d.spheres[0] = desc.spheres[index]
        g.kind = rt4.GROUP_SPHERES
    else:
        d.n_cylinders = 1
        d.cylinders[0] = (desc.cylinders[index] if kind == "cylinder" else
                          (desc.unions[index[0]].cylinder1, desc.unions[index[0]].cylinder2)[index[1]])
        g.kind = rt4.GROUP_CYLINDERS
    g.first, g.count, g.outer, g.new_first = 0, 1, 1, 1
    return d


# --------------------------------------------------------------------------------------------------- float64
def _project64(fig, p, d):
    """(po, drct, miss, ell) of sphere_intersection's ray in float64: the ray itself for a sphere, for a cylinder the
    ray projected as shader.frag:252-258 does it (the axes as they are), the direction normalised in the plane; ell is
    the in-plane share of the direction's length (1 for a sphere)."""
    if fig.a1 is None:
        return fig.centre - p, d, np.zeros(len(p), bool), np.ones(len(p))
    with np.errstate(all="ignore"):
        p1 = p + fig.a1 * ((fig.centre - p) @ fig.a1)[:, None]
        d1 = d - fig.a1 * (d @ fig.a1)[:, None]
        p12 = p1 + fig.a2 * ((fig.centre - p1) @ fig.a2)[:, None]
        e = d1 - fig.a2 * (d1 @ fig.a2)[:, None]
        l1, ln = np.sqrt((d1 * d1).sum(1)), np.sqrt((e * e).sum(1))
        return fig.centre - p12, e / ln[:, None], ~(l1 >= SMALL) | ~(ln >= SMALL), ln / np.sqrt((d * d).sum(1))


U = 2.0 ** -24  # float32 unit roundoff


def decide(fig, rays):
    """The float64 restatement for float32 rays (n, 8); see the module docstring. margin = P / T - 1 (-1 where the host
    disables the cull: T = +inf). near: |margin| <= 1e-5 with dp >= 0, outside, no projection miss: the margin test
    alone decides, and its own float32 rounding is far above the offset. tangent_margin = P / r^2 - 1.

    clear: outside, not a projection miss, and dp < 0 or margin >= 1e-4, each by more than the float32 evaluation can
    move it: the kernels must cull nearly all of these. The float32 P carries up to 3u d2 of rounding (rt4_aux.h; 4u d2
    here with T's own), which is 4.5e-2 of T where K d2 dominates it, so a margin of 1e-4 alone is not clear far out:
    clear asks P - T >= 1e-4 T + noise, noise = 4u d2, and dp <= -8u |po| |d|. A cylinder's po and direction are
    themselves projected in float32 first: po moves by up to ~8u D (D the origin's distance to the cylinder's point
    in 4D, far larger than |po| for an origin far along the axes) and the unit in-plane direction by ~8u / ell (ell
    the in-plane share of the direction's length), so noise gains 64u |po| (D + |po| / ell) and the bound on dp 16u
    (D + |po| / ell). `outside` must hold by 4u d2 (a cylinder: + 32u |po| D) too, and d2 and dp^2 must be finite in
    float32: where they overflow P is inf or NaN and the margin test, rightly, does not fire."""
    rays = np.asarray(rays, F32).astype(np.float64)
    po, dn, miss, ell = _project64(fig, rays[:, :4], rays[:, 4:])
    with np.errstate(all="ignore"):
        d2, dp = (po * po).sum(1), (po * dn).sum(1)
        P = d2 - dp * dp
        T = K * d2 + fig.r2m
        margin = P / T - 1.0
        outside = d2 >= fig.d2_out
        len_po, len_d = np.sqrt(d2), np.sqrt((dn * dn).sum(1))
        noise, dp_noise = 4.0 * U * d2, 8.0 * U * len_po * len_d
        if fig.a1 is not None:
            D = np.sqrt(((fig.centre - rays[:, :4]) ** 2).sum(1))
            noise = noise + 64.0 * U * len_po * (D + len_po / ell)
            dp_noise = dp_noise + 16.0 * U * (D + len_po / ell)
        out_noise = 4.0 * U * d2
        if fig.a1 is not None:
            out_noise = out_noise + 32.0 * U * len_po * D
        representable = d2 * (1.0 + len_d * len_d) < 1e38  # d2 and dp^2 stay finite in float32
        clear = (d2 >= fig.d2_out + out_noise) & representable & ~miss & \
                ((dp < -dp_noise) | (P - T >= 1e-4 * T + noise))
        near = outside & ~miss & (np.abs(margin) <= 1e-5) & (dp >= 0)
        tm = P / (fig.r * fig.r) - 1.0
    return Decision(d2, dp, P, T, margin, outside, miss, clear, near, tm)


# --------------------------------------------------------------------------------------------------- float32
def _mad32(a, s, b):
    return fma32(a, s[..., None], b)


def predicate32(fig, rays):
    """The kernels' predicate in numpy float32, op for op (rt4_device_math.h dot: one product, three fma; mad: fma;
    correctly rounded sqrt and division; fma(K, d2, r2m)): (d2, dp, P, T, miss, fires) with
    fires = not miss and d2 >= d2_out and (dp < 0 or P > T)."""
    rays = np.ascontiguousarray(rays, F32)
    p, d = rays[:, :4], rays[:, 4:]
    c = fig.centre.astype(F32)
    with np.errstate(all="ignore"):
        if fig.a1 is None:
            po, dn, miss = c - p, d, np.zeros(len(p), bool)
        else:
            a1, a2 = fig.a1.astype(F32), fig.a2.astype(F32)
            p1 = _mad32(a1, dot4(c - p, a1), p)          # point_in_space
            d1 = _mad32(a1, -dot4(d, a1), d)             # vec_in_space
            p12 = _mad32(a2, dot4(c - p1, a2), p1)
            e = _mad32(a2, -dot4(d1, a2), d1)
            l1, ln = np.sqrt(dot4(d1, d1)), np.sqrt(dot4(e, e))
            miss = (l1 < F32(SMALL)) | (ln < F32(SMALL))
            po, dn = c - p12, e / ln[:, None]
        d2, dp = dot4(po, po), dot4(po, dn)
        P = d2 - dp * dp
        T = fma32(F32(K), d2, F32(fig.r2m))
        fires = ~miss & (d2 >= F32(fig.d2_out)) & ((dp < 0) | (P > T))
    return d2, dp, P, T, miss, fires


# ------------------------------------------------------------------------------------------------ generators
def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _signed_e(rng, n):
    """Both signs, |e| log-uniform over [1e-8, 1e-2], one in 16 exactly 0."""
    e = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-8, -2, n)
    e[::16] = 0.0
    return e


def _basis(fig):
    """Orthonormal (float64) vectors of the subspace the test lives in: all four axes for a sphere, the complement of
    the cylinder's axes otherwise; and of the axes' own span."""
    if fig.a1 is None:
        return np.eye(4), np.zeros((0, 4))
    q = np.linalg.qr(np.stack([fig.a1, fig.a2, *np.eye(4)]).T)[0].T
    return q[2:4], q[0:2]


def _in(rng, n, basis):
    """Random unit vectors of the span of basis."""
    return _unit(rng.normal(size=(n, len(basis)))) @ basis


def _scale(fig):
    return fig.r if np.isfinite(fig.r) and fig.r > 0 else 1.0


def _origins(fig, rng, n, dist, shift=None, aligned=False):
    """float32 origins at distance dist (n,) from the centre (a cylinder: from its axes plane), optionally moved
    along the cylinder's axes by shift (n, 2). aligned: every fourth origin is displaced along one basis vector of
    the subspace alone, the one along which the centre's coordinate is smallest, and not along the axes: where that
    vector is a coordinate axis and the coordinate 0, the rounded origin's distance is dist's own float32 value."""
    sub, ax = _basis(fig)
    u = _in(rng, n, sub)
    s = (shift if shift is not None else rng.normal(0, 2.0 * _scale(fig), (n, 2))) if len(ax) else None
    if aligned:
        k = int(np.argmin(np.abs(sub @ fig.centre)))
        u[::4] = sub[k] * np.where(rng.random(len(u[::4])) < 0.5, -1.0, 1.0)[:, None]
        if s is not None:
            s = s.copy()
            s[::4] = 0.0
    p = fig.centre + dist[:, None] * u
    if s is not None:
        p = p + s @ ax
    with np.errstate(over="ignore"):
        return p.astype(F32)


def _aim(fig, rng, p32, rho2_of, ell=None):
    """float64 directions from the ROUNDED origins whose line passes the centre (the axes plane) at squared distance
    rho2_of(d2) in the test's subspace, the figure ahead. A cylinder: the in-plane part has length ell (default
    uniform over [0.3, 1]) and the rest of a unit vector lies along the axes."""
    n = len(p32)
    sub, ax = _basis(fig)
    p = p32.astype(np.float64)
    po = _project64(fig, p, np.ones((n, 4)))[0]
    po = (po @ sub.T) @ sub  # exactly in the subspace (the stored axes are orthonormal to ~1e-7 only)
    with np.errstate(all="ignore"):
        d2 = (po * po).sum(1)
        sin2 = np.clip(rho2_of(d2) / d2, 0.0, 1.0)
        u = po / np.sqrt(d2)[:, None]
        v = _in(rng, n, sub)
        v = _unit(v - (v * u).sum(1, keepdims=True) * u)
        g = np.sqrt(1.0 - sin2)[:, None] * u + np.sqrt(sin2)[:, None] * v
    if len(ax):
        ell = rng.uniform(0.3, 1.0, n) if ell is None else ell
        g = ell[:, None] * g + np.sqrt(np.maximum(1.0 - ell * ell, 0.0))[:, None] * _in(rng, n, ax)
    return g


def _rays(p32, d):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.concatenate([p32, d.astype(F32)], axis=1)


def _far(fig, rng, n):
    """Distances L = m 10^U over L / m in [1.0001, 1e6] (cylinders: 1e5), log-uniform; m = max(r, SMALL), the
    distance from which a ray is outside (below SMALL the shader takes its len_po < SMALL branch whatever r is)."""
    hi = 1e6 if fig.a1 is None else 1e5
    return max(_scale(fig), SMALL) * np.exp(rng.uniform(np.log(1.0001), np.log(hi), n))


def _T(fig):
    r2m = fig.r2m if np.isfinite(fig.r2m) else _scale(fig) ** 2 * (1.0 + 1e-4)  # a disabled figure: as if enabled
    return lambda d2: K * d2 + r2m


def cull_seam(fig, seed, n, label="cull_seam", shift=None, ell=None):
    """The line's squared distance is T (1 + e), T = K d2 + r2m of the rounded origin: the cull's own threshold."""
    rng = np.random.default_rng(seed)
    e = _signed_e(rng, n)
    p32 = _origins(fig, rng, n, _far(fig, rng, n), shift)
    T = _T(fig)
    return Stratum(_rays(p32, _aim(fig, rng, p32, lambda d2: T(d2) * (1.0 + e), ell)), label, e)


def tangent(fig, seed, n):
    """P = r^2 (1 + e): the geometric boundary at those distances; about half of these rays hit."""
    rng = np.random.default_rng(seed)
    e = _signed_e(rng, n)
    p32 = _origins(fig, rng, n, _far(fig, rng, n))
    r2 = _scale(fig) ** 2
    return Stratum(_rays(p32, _aim(fig, rng, p32, lambda d2: r2 * (1.0 + e) + 0.0 * d2)), "tangent", e)


def _any_direction(fig, rng, p32):
    """A third of the directions uniform, a third nearly perpendicular to po (dp = +-|po| 10^U(-9, -1)), a third
    aimed at the figure; lengths 1 or 1/4 .. 4."""
    n = len(p32)
    sub, _ = _basis(fig)
    beta = np.where(rng.random(n) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-9, -1, n)
    perp = _aim(fig, rng, p32, lambda d2: d2 * (1.0 - beta * beta)) * np.sign(beta)[:, None]
    at = _aim(fig, rng, p32, lambda d2: rng.uniform(0, 1, n) * min(_scale(fig) ** 2, 1e30) + 0.0 * d2)
    d = np.where((np.arange(n) % 3 == 0)[:, None], _unit(rng.normal(size=(n, 4))),
                 np.where((np.arange(n) % 3 == 1)[:, None], perp, at))
    d = np.where(np.isfinite(d), d, _unit(rng.normal(size=(n, 4))))
    return d * np.where(rng.random(n) < 0.5, 1.0, np.exp(rng.uniform(np.log(0.25), np.log(4.0), n)))[:, None]


def surface(fig, seed, n):
    """Origins at |p - c| = r (1 + j 2^-24), j in -8..8, any direction: `outside` (len_po >= r) with the sign of dp,
    and the flip seam len_po > r. e is j 2^-24. Every fourth origin along one basis vector (_origins: aligned)."""
    rng = np.random.default_rng(seed)
    j = rng.integers(-8, 9, n)
    p32 = _origins(fig, rng, n, _scale(fig) * (1.0 + j * 2.0 ** -24), aligned=True)
    return Stratum(_rays(p32, _any_direction(fig, rng, p32)), "surface", j * 2.0 ** -24)


def centre(fig, seed, n):
    """Origins at |p - c| = SMALL (1 + j 2^-20), j in -8..8, any direction: the len_po < SMALL branch, and where
    d2_out comes from SMALL for radii below it. e is j 2^-20. Every fourth origin along one basis vector."""
    rng = np.random.default_rng(seed)
    j = rng.integers(-8, 9, n)
    p32 = _origins(fig, rng, n, SMALL * (1.0 + j * 2.0 ** -20), aligned=True)
    return Stratum(_rays(p32, _any_direction(fig, rng, p32)), "centre", j * 2.0 ** -20)


def outside_seam(fig, seed, n):
    """Origins whose float32 d2 is d2_out + j ulp, j in -2..2 (e is j): the `outside` seam to the bit. Two steps
    along two basis vectors of the subspace: a coarse one of 0.3 .. 0.9 of the distance, rounded, then the rest of
    the target along the vector on which the centre's coordinate is smallest, where a float32 is finest. Exact
    where those vectors are coordinate axes (the named scenes), within an ulp or two of the target elsewhere."""
    rng = np.random.default_rng(seed)
    sub, _ = _basis(fig)
    j = rng.integers(-2, 3, n)
    t32 = np.full(n, fig.d2_out if np.isfinite(fig.d2_out) else 1.0, F32)
    for step in (1, 2):
        t32 = np.where(j >= step, np.nextafter(t32, F32(np.inf)), np.where(j <= -step, np.nextafter(t32, F32(0)), t32))
    target = t32.astype(np.float64)
    k1 = int(np.argmin(np.abs(sub @ fig.centre)))
    k0 = (k1 + 1) % len(sub)
    sign = lambda: np.where(rng.random(n) < 0.5, -1.0, 1.0)[:, None]
    first = (fig.centre + (np.sqrt(target) * rng.uniform(0.3, 0.9, n))[:, None] * sub[k0] * sign()).astype(F32)
    rest = target - ((fig.centre - first.astype(np.float64)) @ sub[k0]) ** 2
    p32 = (first.astype(np.float64) + np.sqrt(np.maximum(rest, 0.0))[:, None] * sub[k1] * sign()).astype(F32)
    return Stratum(_rays(p32, _any_direction(fig, rng, p32)), "outside", j.astype(np.float64))


def non_unit(fig, seed, n):
    """cull_seam with the direction scaled by 2^k, k in -3..3 (the derivation is in d2 and dp alone, whatever the
    direction's length). Every other ray of a sphere is aimed anew so that d2 - dp^2 of the SCALED direction lies
    on the seam, where a direction can do that (a cylinder's in-plane direction is normalised by the test itself)."""
    rng = np.random.default_rng(seed)
    st = cull_seam(fig, seed + 1, n)
    k = rng.integers(-3, 4, n)
    rays = st.rays.astype(np.float64)
    if fig.a1 is None:
        T, s2 = _T(fig), 4.0 ** k
        again = _aim(fig, rng, st.rays[:, :4], lambda d2: d2 - np.clip((d2 - T(d2) * (1.0 + st.e)) / s2, 0.0, d2))
        po = fig.centre - rays[:, :4]
        d2 = (po * po).sum(1)
        ok = (np.arange(n) % 2 == 1) & ((d2 - T(d2) * (1.0 + st.e)) / s2 < d2) & np.isfinite(again).all(1)
        rays[ok, 4:] = again[ok].astype(F32)
    rays[:, 4:] *= (2.0 ** k)[:, None]
    return Stratum(rays.astype(F32), "non_unit", st.e)


def overflow(fig, seed, n):
    """cull_seam from origins so far away that d2 lies in [2^120, +inf]: there the fp32 P is inf or NaN."""
    rng = np.random.default_rng(seed)
    e = _signed_e(rng, n)
    p32 = _origins(fig, rng, n, 2.0 ** rng.uniform(60.0, 64.4, n), shift=rng.normal(0, 2.0, (n, 2)))
    T = _T(fig)
    d = _aim(fig, rng, p32, lambda d2: T(d2) * (1.0 + e))
    back = rng.random(n) < 0.125  # an eighth look away: the early-out with an infinite d2
    d[back] = -d[back]
    return Stratum(_rays(p32, d), "overflow", e)


def axial(fig, seed, n):
    """Cylinders: cull_seam with the origin moved up to 1e4 r along the axes."""
    rng = np.random.default_rng(seed)
    s = np.where(rng.random((n, 2)) < 0.5, -1.0, 1.0) * _scale(fig) * 10.0 ** rng.uniform(-1, 4, (n, 2))
    return cull_seam(fig, seed + 1, n, "axial", shift=s)


def flat(fig, seed, n):
    """Cylinders: cull_seam with the in-plane part of the direction short: half of the rays with a length log-uniform
    over [1.5e-4, 1] (below SMALL the projection misses), the others within 1e-3 relative of SMALL, both sides."""
    rng = np.random.default_rng(seed)
    ell = np.exp(rng.uniform(np.log(1.5e-4), 0.0, n))
    ell[1::2] = SMALL * (1.0 + rng.uniform(-1e-3, 1e-3, len(ell[1::2])))
    return cull_seam(fig, seed + 1, n, "flat", ell=ell)


def strata(fig, seed, n):
    """Every stratum that applies to the figure, n rays each."""
    gens = [cull_seam, tangent, surface, centre, non_unit, overflow, outside_seam] + \
           ([axial, flat] if fig.a1 is not None else [])
    return [g(fig, seed + 10 * i, n) for i, g in enumerate(gens)]


# ------------------------------------------------------------------------------------- the derivation's cited figure
SIN_ACOS_BOUND = 1.75e-7  # rt4_aux.h: sin_(acos_(c)) is within this (relative) of sqrt(1 - c^2) on [0, 1)


def sweep_inputs():
    """Every float32 of [0.5, 1) and every 64th of [0, 0.5)."""
    lo = np.arange(0, 0x3F000000, 64, dtype=np.uint32)
    hi = np.arange(0x3F000000, 0x3F800000, dtype=np.uint32)
    return np.concatenate([lo, hi]).view(F32)


def sin_acos_error(c, s):
    """(largest relative error of s against sqrt((1 - c)(1 + c)) in float64, the bit pattern of the c it falls on)."""
    c64 = c.astype(np.float64)
    exact = np.sqrt((1.0 - c64) * (1.0 + c64))
    rel = np.abs(s.astype(np.float64) - exact) / exact
    i = int(np.argmax(rel))
    return float(rel[i]), int(c[i:i + 1].view(np.uint32)[0])


# --------------------------------------------------------------------------------------------- a view of the seam
def seam_view(rt4, fig, small_indent=0.005, samples=2, reflections=3, seed=4242, w=64, h=40, dist=50.0):
    """Uniforms of a camera dist radii from the figure that looks along +y past its silhouette: the central ray is
    tangent, and the matrix is zoomed so that the image spans a perpendicular distance of r (1 +- 4 m) across (a
    sphere; along x) or upwards (a cylinder whose plane holds y and z), m = sqrt(T) / r - 1 the cull margin's
    relative width at that distance. So the image holds the geometric silhouette and, m further out, the cull's seam."""
    sub, _ = _basis(fig)
    inplane = lambda v: float(np.linalg.norm(sub @ v))
    ex, ey, ez = np.eye(4)[0], np.eye(4)[1], np.eye(4)[2]
    assert inplane(ey) > 0.999999, "the view direction lies in the figure's plane"
    side, across = (ex, True) if inplane(ex) > 0.999999 else (ez, False)
    assert inplane(side) > 0.999999
    L = dist * fig.r
    m = np.sqrt(K * L * L + fig.r2m) / fig.r - 1.0
    focus = fig.centre - side * fig.r - ey * np.sqrt(L * L - fig.r * fig.r)
    u = rt4.make_uniforms(w, h, samples=samples, reflections=reflections, seed=seed, small_indent=small_indent,
                          focus=tuple(float(F32(x)) for x in focus))
    f = float(np.linalg.norm([u.vec_to_mtr[i] for i in range(4)]))
    half = f * 4.0 * m / dist  # half the matrix's size along `side`: an angle of 4 m r / L
    if across:
        u.mtr_sizes[0], u.mtr_sizes[1] = 2.0 * half, 2.0 * half * h / w
    else:
        u.mtr_sizes[0], u.mtr_sizes[1] = 2.0 * half * w / h, 2.0 * half
    return u
