"""The band filters of the cylinders union and the tiger (rt4_fast.h union_cand, tiger_pair, tiger_quarter), restated
from the scene description alone, and rays aimed at their seams. A plain helper, not a fixture:
test_band_filter_ref.py (CPU, against the oracle and the library's host code) and test_gpu_band_filter.py (against
the kernels) use it.

A cylinder face of the union or the tiger is kept only where the hit point's distance d to the OTHER axes pair lies
in a band: the oracle tests d > r_out and d < r_in with d = RN(sqrt(q)), q = dot(v, v). The specialised kernels compare
q itself with thresholds the host makes from the radii (rt4_trace.hip sqrt_gt_threshold, sqrt_lt_threshold). What
the tests hold the kernels to is the definition, not the host's search:

  gt(r): (q > gt(r)) == (RN(sqrt(q)) > r)     lt(r): (q < lt(r)) == (RN(sqrt(q)) < r)

for every float32 q that dot(v, v) can give: +0, denormals, normals, +inf, NaN.

The six seam kinds (seams()): a face of radius rA around its own axes pair, filtered by the radius rB of the other
pair. Its points are
  x = c + rA (cos al . o1 + sin al . o2) + rB (1 + e) (cos be . s1 + sin be . s2),
(s1, s2) the face's own axes, (o1, o2) the other pair's: the face's circle lives in the complement of its own axes,
and the filter's distance in the span of them.
  union_f1         face cylinder1                    at cylinder2.r   (>)
  union_f2         face cylinder2                    at cylinder2.r   (>; shader.frag:290 uses cylinder2.r here too)
  tiger_a_outer    faces inner_cyl1, outer_cyl1      at outer_cyl2.r  (>)
  tiger_a_inner    faces inner_cyl1, outer_cyl1      at inner_cyl2.r  (<)
  tiger_b_outer    faces inner_cyl2, outer_cyl2      at outer_cyl1.r  (>)
  tiger_b_inner    faces inner_cyl2, outer_cyl2      at inner_cyl1.r  (<)

Two strata of rays:
  aimed(): rays x - t d -> d through a seam point, t in [0.5, 3], random d drawn towards the filter's direction
    (see aimed()), for a nominal relative offset e of the filter's distance. The rays are rounded to float32 and
    the hit point is computed in float32, so |e| <= 2^-22 only scatters q across the threshold.
  exact(): for axis-aligned figures, rays whose direction has zero components along the filter's two coordinates.
    The hit point's offset there is the origin's (fma(0, dist, p) = p), so q is a float32 the generator chooses: the
    thresholds themselves, their neighbours, +0, the smallest denormal, FLT_MAX and +inf. q is computed by
    axes_dist_sq_f32(), the kernel's op order in exactly rounded float32 arithmetic.

Further down: the views zoomed in on a seam (zoom_view, pick_view, zoom_cases) and the special-radius cases
(special_case, special_case_checked, MASKED). Whatever decides that a case can show a wrong filter is computed
here from the oracle and this restatement, never from a kernel's output.
"""
import collections
from fractions import Fraction

import numpy as np

F32 = np.float32
FLT_MAX = float(np.finfo(F32).max)
DENORM_MIN = float(np.nextafter(F32(0), F32(1)))
INF = float("inf")

Seam = collections.namedtuple("Seam", "name kind rel field centre own other faces filter_r")
Face = collections.namedtuple("Face", "r color")
Stratum = collections.namedtuple("Stratum", "rays t face e label")

# e of the aimed strata: 0, then +-2^-24 .. +-2^-10 in octaves; every signed e with |e| <= E_NOISE is inside the
# rounding noise of q: the oracle keeps 15 % to 85 % of its aimed hits (asserted in test_band_filter_ref.py)
E_OCTAVES = [0.0] + [s * 2.0 ** -k for k in range(24, 9, -1) for s in (1.0, -1.0)]
E_NOISE = 2.0 ** -22
E_CLEAR = 1e-3
# the radii the thresholds are made from, in the order of the special-radius cases
FIELDS = ["cylinder2", "outer_cyl1", "outer_cyl2", "inner_cyl1", "inner_cyl2"]


# ------------------------------------------------------------------------------------------------ thresholds
def sqrt32(q):
    """Correctly rounded float32 square root (numpy's)."""
    with np.errstate(invalid="ignore"):
        return np.sqrt(np.asarray(q, F32))


def _up(x):
    with np.errstate(over="ignore"):
        return F32(np.nextafter(F32(x), F32(np.inf)))


def _down(x):
    return F32(np.nextafter(F32(x), F32(-np.inf)))


def gt(r):
    """The float32 g with (q > g) == (RN(sqrt(q)) > r) for every q >= +0, +inf and NaN included."""
    r = F32(r)
    if np.isnan(r) or r == F32(np.inf):
        return F32(np.inf)  # no q is above r, q = +inf included
    if r < 0:
        return F32(-1.0)  # every q >= +0 is above r; NaN > g stays false
    x = F32(min(float(r) * float(r), FLT_MAX))  # near the largest x with RN(sqrt(x)) <= r; RN(sqrt) is monotonic
    while x < F32(FLT_MAX) and sqrt32(_up(x)) <= r:
        x = _up(x)
    while x > 0 and sqrt32(x) > r:
        x = _down(x)
    return x


def lt(r):
    """The float32 l with (q < l) == (RN(sqrt(q)) < r) for every q >= +0, +inf and NaN included."""
    r = F32(r)
    if not r > 0:
        return F32(0.0)  # NaN, zero, negative: no q is below r
    if r == F32(np.inf):
        return F32(np.inf)  # every finite q is
    x = F32(min(float(r) * float(r), FLT_MAX))  # near the smallest x with RN(sqrt(x)) >= r
    while x < F32(np.inf) and sqrt32(x) < r:
        x = _up(x)
    while x > 0 and sqrt32(_down(x)) >= r:
        x = _down(x)
    return x


def neighbours(x, k=4):
    """The floats within k ulp of x that dot(v, v) can give (>= +0, up to +inf)."""
    x = F32(x)
    if np.isnan(x):
        return np.zeros(0, F32)
    if x == F32(np.inf):
        bits = np.arange(0x7F800000 - k, 0x7F800001, dtype=np.int64)
    else:
        b = int(np.array(max(float(x), 0.0), F32).view(np.uint32))
        bits = np.arange(max(b - k, 0), min(b + k, 0x7F800000) + 1, dtype=np.int64)
    return bits.astype(np.uint32).view(F32)


def probes(r, k=4):
    """The q at which a threshold of radius r is tested: within k ulp of gt(r) and lt(r), and the ends of the range."""
    ends = np.array([0.0, DENORM_MIN, FLT_MAX, np.inf, np.nan], F32)
    return np.concatenate([neighbours(gt(r), k), neighbours(lt(r), k), ends])


def holds(r, g, l, q):
    """(gt part, lt part): where thresholds g, l meet the definition for radius r at the values q."""
    r, q = F32(r), np.asarray(q, F32)
    with np.errstate(invalid="ignore"):
        d = sqrt32(q)
        return (q > F32(g)) == (d > r), (q < F32(l)) == (d < r)


def kept(q, r_out, r_in=None):
    """The oracle's band decision for q = dot(v, v): not (d > r_out or d < r_in)."""
    with np.errstate(invalid="ignore"):
        d = sqrt32(q)
        out = ~(d > F32(r_out))
        return out if r_in is None else out & ~(d < F32(r_in))


# --------------------------------------------------------------------------------------------------- seams
def _f64(v):
    return np.array([float(v[i]) for i in range(4)], np.float64)


def _color(m):
    return tuple(float(np.float32(x)) for x in m.color)


def seams(desc, union=0, tiger=0):
    """The seam kinds of union `union` and tiger `tiger` of the scene (those it has), see the module docstring."""
    out = []
    if desc.n_unions > union:
        u = desc.unions[union]
        ax1, ax2 = (_f64(u.cylinder1.axis1), _f64(u.cylinder1.axis2)), (_f64(u.cylinder2.axis1), _f64(u.cylinder2.axis2))
        f1, f2 = Face(float(u.cylinder1.r), _color(u.cylinder1.material)), Face(float(u.cylinder2.r), _color(u.cylinder2.material))
        rb = float(u.cylinder2.r)
        out.append(Seam("union_f1", "union", "gt", "cylinder2", _f64(u.cylinder1.point), ax1, ax2, [f1], rb))
        out.append(Seam("union_f2", "union", "gt", "cylinder2", _f64(u.cylinder2.point), ax2, ax1, [f2], rb))
    if desc.n_tigers > tiger:
        t = desc.tigers[tiger]
        ax1, ax2 = (_f64(t.inner_cyl1.axis1), _f64(t.inner_cyl1.axis2)), (_f64(t.inner_cyl2.axis1), _f64(t.inner_cyl2.axis2))
        fa = [Face(float(c.r), _color(c.material)) for c in (t.inner_cyl1, t.outer_cyl1)]
        fb = [Face(float(c.r), _color(c.material)) for c in (t.inner_cyl2, t.outer_cyl2)]
        c1, c2 = _f64(t.inner_cyl1.point), _f64(t.inner_cyl2.point)
        out.append(Seam("tiger_a_outer", "tiger", "gt", "outer_cyl2", c1, ax1, ax2, fa, float(t.outer_cyl2.r)))
        out.append(Seam("tiger_a_inner", "tiger", "lt", "inner_cyl2", c1, ax1, ax2, fa, float(t.inner_cyl2.r)))
        out.append(Seam("tiger_b_outer", "tiger", "gt", "outer_cyl1", c2, ax2, ax1, fb, float(t.outer_cyl1.r)))
        out.append(Seam("tiger_b_inner", "tiger", "lt", "inner_cyl1", c2, ax2, ax1, fb, float(t.inner_cyl1.r)))
    return out


def radius_field(desc, field, union=0, tiger=0):
    """The cylinder whose radius one of FIELDS names."""
    return getattr(desc.unions[union] if field == "cylinder2" else desc.tigers[tiger], field)


def seam_points(seam, face_r, al, be, e):
    """Float64 points on the face of radius face_r whose distance to the other axes pair is filter_r (1 + e)."""
    al, be, e = (np.asarray(v, np.float64)[:, None] for v in (al, be, e))
    face_r = np.asarray(face_r, np.float64)[:, None]
    return (seam.centre + face_r * (np.cos(al) * seam.other[0] + np.sin(al) * seam.other[1])
            + seam.filter_r * (1.0 + e) * (np.cos(be) * seam.own[0] + np.sin(be) * seam.own[1]))


D_BIAS = (0.5, 4.0)  # aimed(): the weight of the filter's own direction in a ray's direction, uniform per ray


def aimed(seam, seed, n, e):
    """n rays x - t d -> d through seam points of offset e (a number or n of them): random al, be, t uniform over
    [0.5, 3], the face alternating between the seam's faces. The aimed hit is at distance t.

    d is a random unit vector plus D_BIAS times the unit vector along which the filter measures (the seam point's
    offset within the face's own axes pair, either sign), normalised: 14 to 60 degrees off that direction. The
    rounding error of the hit distance moves the hit point along d, so these are the rays whose q it moves most.
    With an isotropic d the oracle keeps the aimed hit on the wrong side of |e| = 2^-22 for 6 to 9 % of the rays
    (tiger), with this d for 20 % and more: every signed e up to E_NOISE lies inside the rounding noise of q, which
    test_band_filter_ref.py asserts. d's sign then brings the ray to the face from its open side."""
    rng = np.random.default_rng(seed)
    face = np.arange(n) % len(seam.faces)
    face_r = np.array([f.r for f in seam.faces])[face]
    e = np.broadcast_to(np.asarray(e, np.float64), (n,)).copy()
    al, be = rng.uniform(0, 2 * np.pi, n), rng.uniform(0, 2 * np.pi, n)
    x = seam_points(seam, face_r, al, be, e)
    d = rng.normal(size=(n, 4))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    normal = np.cos(al)[:, None] * seam.other[0] + np.sin(al)[:, None] * seam.other[1]  # the face's
    along = np.cos(be)[:, None] * seam.own[0] + np.sin(be)[:, None] * seam.own[1]  # the filter's direction
    d += rng.uniform(D_BIAS[0], D_BIAS[1], n)[:, None] * np.where((d * along).sum(1) < 0, -1.0, 1.0)[:, None] * along
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # towards the face from its open side, so that fewer aimed hits lie behind another face: the figure's body is
    # inside the union's cylinders and between the tiger's radii
    inward = (seam.kind == "tiger") & (face == 0)
    d *= np.where(((d * normal).sum(1) > 0) == inward, 1.0, -1.0)[:, None]
    t = rng.uniform(0.5, 3.0, n)
    rays = np.concatenate([x - t[:, None] * d, d], axis=1).astype(F32)
    return Stratum(rays, t, face, e, "aimed")


def aimed_all(seam, seed, n, es=None):
    """The aimed strata of every e of E_OCTAVES and of +-E_CLEAR, n rays each, as one Stratum."""
    es = list(E_OCTAVES) + [E_CLEAR, -E_CLEAR] if es is None else es
    parts = [aimed(seam, seed + 17 * i, n, e) for i, e in enumerate(es)]
    return Stratum(np.concatenate([p.rays for p in parts]), np.concatenate([p.t for p in parts]),
                   np.concatenate([p.face for p in parts]), np.concatenate([p.e for p in parts]), "aimed")


def aimed_hit(seam, st, out, col):
    """Where find_intersection's result (rows out, colours col) is the stratum's aimed hit: a hit of the aimed face's
    colour at the distance t the ray was built with (to 1e-4: another face of that colour is farther off)."""
    colors = np.array([f.color for f in seam.faces], F32)[st.face]
    with np.errstate(invalid="ignore"):
        return (out[:, 0] > 0) & (np.asarray(col, F32) == colors).all(axis=1) & (np.abs(out[:, 1] - st.t) <= 1e-4)


# ------------------------------------------------------------------------------- exactly rounded float32, in Python
def _rn32(x):
    """A Fraction rounded to the nearest float32 (ties to even, overflow to inf), as a Python float."""
    if x == 0:
        return 0.0
    with np.errstate(over="ignore"):
        f = F32(float(x))
    best = None
    for c in (_down(f), f, _up(f)):
        if np.isnan(c):
            continue
        c = float(c)
        val = Fraction(c) if np.isfinite(c) else Fraction(2) ** 128 * (1 if c > 0 else -1)  # the next binade's start
        key = (abs(val - x), int(np.array(c, F32).view(np.uint32)) & 1)  # an infinity's mantissa is even
        if best is None or key < best[0]:
            best = (key, c)
    return best[1]


def _fma(a, b, c):
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        with np.errstate(all="ignore"):
            return float(F32(np.float64(a) * np.float64(b) + np.float64(c)))
    return _rn32(Fraction(a) * Fraction(b) + Fraction(c))


def _dot(a, b):
    return _fma(a[3], b[3], _fma(a[2], b[2], _fma(a[1], b[1], _fma(a[0], b[0], 0.0))))


def _mad(a, s, c):
    return [_fma(a[i], s, c[i]) for i in range(4)]


def _sub(a, b):
    return [_fma(1.0, a[i], -b[i]) for i in range(4)]


def _point_in_space(p, sp, n):
    return _mad(n, _dot(_sub(sp, p), n), p)


def axes_dist_sq_f32(dist, ray, cp, a1, a2):
    """rt4_fast.h axes_dist_sq (the oracle's dist_to_axes_plane before its sqrt) in exactly rounded float32."""
    ray = [float(v) for v in np.asarray(ray, F32)]
    cp, a1, a2 = ([float(F32(v)) for v in w] for w in (cp, a1, a2))
    p = _mad(ray[4:], float(F32(dist)), ray[:4])
    p12 = _point_in_space(_point_in_space(p, cp, a1), cp, a2)
    v = _sub(cp, p12)
    return _dot(v, v)


# --------------------------------------------------------------------------------------------------- exact
def _axis_index(a):
    nz = np.flatnonzero(a)
    return int(nz[0]) if len(nz) == 1 and abs(a[nz[0]]) == 1.0 else None


def axis_aligned(seam):
    return all(_axis_index(a) is not None for a in seam.own + seam.other)


def exact_targets(seam):
    """[(label, q)]: the values of q the exact stratum aims at for the seam's threshold; q is None where the label
    names no value dot(v, v) can give (a negative threshold, the float above +inf)."""
    thr = gt(seam.filter_r) if seam.rel == "gt" else lt(seam.filter_r)
    rows = [(seam.rel, float(thr)), (seam.rel + " up", float(_up(thr)) if thr < F32(np.inf) else None),
            (seam.rel + " down", float(_down(thr))), ("+0", 0.0), ("denorm min", DENORM_MIN), ("FLT_MAX", FLT_MAX),
            ("+inf", INF)]
    return [(label, q if q is not None and q >= 0.0 else None) for label, q in rows]


def _steps(x, ks):
    out = []
    for k in ks:
        y = F32(x)
        for _ in range(abs(k)):
            y = _up(y) if k > 0 else _down(y)
        out.append(float(y))
    return out


def _reach(target, q_of, s_cands):
    """Offsets (m, s) along the filter's two coordinates with q_of(m, s) == target, or None. m carries the bulk,
    s^2 the last ulps: RN(m^2) alone reaches about half of the floats. s_cands(s0): the offsets near s0 to try."""
    if target == 0.0:
        return (0.0, 0.0) if q_of(0.0, 0.0) == 0.0 else None
    if target == INF:
        m = float(F32(2e19))
        return (m, 0.0) if q_of(m, 0.0) == INF else None
    m0 = float(F32(np.sqrt(np.float64(target))))
    for m in _steps(m0, range(1, -25, -1)):
        need = target - min(m * m, FLT_MAX)
        if need < 0.0:
            continue
        cands = [0.0] + (s_cands(float(np.sqrt(need))) if need > 0.0 else [])
        for s in cands:
            if q_of(m, s) == target:
                return m, s
    return None


def exact(seam, psis=(0.0, 0.2, -0.2), reach=3.0):
    """The exact stratum of an axis-aligned seam: (Stratum, table). The rays run in the plane of the other axes pair,
    from `reach` away straight at the figure's centre, at the angles psis to that plane's first axis that is not z;
    their origins' offsets along the face's own two axes give q. table: [(label, target q, reached)], one row per
    target of exact_targets(); the stratum's e holds each ray's q."""
    assert axis_aligned(seam)
    i1, i2 = _axis_index(seam.own[0]), _axis_index(seam.own[1])
    j1, j2 = _axis_index(seam.other[0]), _axis_index(seam.other[1])
    if j1 == 2:  # z is up: keep the rays level, off the ground
        j1, j2 = j2, j1
    if seam.centre[i1] != 0.0 and seam.centre[i2] == 0.0:
        i1, i2 = i2, i1  # the bulk along a coordinate whose centre is 0: there the offset is the origin's coordinate
    c32 = seam.centre.astype(F32)

    def origin(m, s, psi):
        o = c32.astype(np.float64)
        o[j1] -= reach * np.cos(psi)
        o[j2] -= reach * np.sin(psi)
        o[i1], o[i2] = float(c32[i1]) - m, float(c32[i2]) - s
        d = np.zeros(4)
        d[j1], d[j2] = np.cos(psi), np.sin(psi)
        return np.concatenate([o, d]).astype(F32)

    def q_of(m, s, psi=psis[0]):
        return axes_dist_sq_f32(reach - 1.0, origin(m, s, psi), c32, seam.other[0], seam.other[1])  # the filter's cylinder

    def s_cands(s0):
        c = float(c32[i2])
        if c == 0.0:
            return _steps(s0, (0, -1, 1, -2, 2))
        return [c - p for p in _steps(c - s0, (0, -1, 1, -2, 2, -3, 3))]  # the origin's coordinate moves in its own ulps

    rays, qs, table = [], [], []
    for label, target in exact_targets(seam):
        ms = _reach(target, q_of, s_cands) if target is not None else None
        good = ms is not None and all(q_of(ms[0], ms[1], psi) == target for psi in psis)
        table.append((label, target, good))
        if good:
            rays += [origin(ms[0], ms[1], psi) for psi in psis]
            qs += [target] * len(psis)
    n = len(rays)
    rays = np.array(rays, F32).reshape(n, 8)
    return Stratum(rays, np.full(n, np.nan), np.zeros(n, np.int64), np.array(qs, np.float64), "exact"), table


def exact_kept(seam, desc, st):
    """The band decision of the definition for the exact stratum's rays (their q is st.e): both filters of a tiger's
    face, the one of a union's."""
    if seam.kind == "union":
        return kept(st.e, seam.filter_r)
    t = desc.tigers[0]
    r_out, r_in = (t.outer_cyl2.r, t.inner_cyl2.r) if seam.name.startswith("tiger_a") else (t.outer_cyl1.r, t.inner_cyl1.r)
    return kept(st.e, r_out, r_in)


# --------------------------------------------------------------------------------------------------- views
def zoom_view(rt4, seam, matrix_height, fi=0.0, te=0.0, psi=0.0, samples=2, reflections=2, seed=77, face=-1):
    """Uniforms (64 x 40) of a camera three units in front of a seam point, zoomed so far in that neighbouring pixels
    differ by about an ulp in direction: focus = x - 3 forward. The seam point is the one whose face normal looks
    most at the camera and whose filter direction lies most along the image's right (or up) direction, so that the
    seam crosses the frame. None when the camera turned by fi, te, psi (degrees) sees the face edge-on."""
    u = rt4.make_uniforms(64, 40, samples=samples, reflections=reflections, seed=seed, matrix_height=matrix_height, fi=fi,
                          te=te, psi=psi)
    fwd = np.array(list(u.vec_to_mtr), np.float64)
    fwd /= np.linalg.norm(fwd)

    def in_plane(v, pair):
        return (v @ pair[0]) * pair[0] + (v @ pair[1]) * pair[1]

    normal = -in_plane(fwd, seam.other)
    if np.linalg.norm(normal) < 0.3:
        return None
    across = in_plane(np.array(list(u.right_drct), np.float64), seam.own)
    if np.linalg.norm(across) < 0.3:
        across = in_plane(np.array(list(u.top_drct), np.float64), seam.own)
    if np.linalg.norm(across) < 0.3:
        return None
    x = (seam.centre + seam.faces[face].r * normal / np.linalg.norm(normal)
         + seam.filter_r * across / np.linalg.norm(across))
    focus = tuple(float(v) for v in (x - 3.0 * fwd).astype(F32))
    return rt4.make_uniforms(64, 40, samples=samples, reflections=reflections, seed=seed, matrix_height=matrix_height,
                             fi=fi, te=te, psi=psi, focus=focus)


VIEW_TURNS = ([(fi, te, 0.0) for te in (0.0, 30.0, 60.0) for fi in (0.0, 180.0, 90.0, 270.0, 45.0, 135.0, 225.0, 315.0)]
              + [(fi, te, psi) for psi in (90.0, -90.0) for te in (60.0, 30.0) for fi in (0.0, 180.0, 90.0, 270.0)])
MIN_CLASS = 0.2  # a zoomed view counts when the second most frequent pixel value holds this share of the frame


def pick_view(rt4, oracle, desc, seam):
    """(fi, te, psi, face) of the first camera turn of VIEW_TURNS and face (the outer radius first) for which, by the
    oracle alone, the ray through the seam point, three units away, ends on that face (nothing of the scene stands in
    between) and the frame at matrix_height 2^-14, one sample, no reflections, has two pixel values of at least
    MIN_CLASS of the pixels each: what lies behind the seam differs from the face. None: no such view."""
    import denoise_ref

    reg = rt4.region(64, 40)
    # at a seam two faces of the figure meet (the filter's radius is the other pair's face radius): either may win
    colors = np.array(sorted({f.color for sm in seams(desc) if sm.kind == seam.kind for f in sm.faces}), F32)
    for fi, te, psi in VIEW_TURNS:
        for face in range(len(seam.faces) - 1, -1, -1):
            u = zoom_view(rt4, seam, 2.0 ** -14, fi=fi, te=te, psi=psi, samples=1, reflections=0, face=face)
            if u is None:
                continue
            rays = denoise_ref.primary_rays(u, reg)[::13, ::7].reshape(-1, 8)  # the seam passes through the centre
            out, col = oracle.find_intersection(desc, rays)
            on_face = (out[:, 0] > 0) & (np.abs(out[:, 1] - 3.0) < 1e-3) & (col[:, None] == colors[None]).all(2).any(1)
            if on_face.any() and two_classes(oracle.render(desc, u, reg)[0]) >= MIN_CLASS:
                return fi, te, psi, face
    return None


def two_classes(image):
    """Share of the second most frequent pixel value of an (h, w, 4) image."""
    px = np.ascontiguousarray(image, F32).reshape(-1, image.shape[-1]).view(np.uint32)
    _, counts = np.unique(px, axis=0, return_counts=True)
    counts = np.sort(counts)[::-1]
    return (counts[1] if len(counts) > 1 else 0) / px.shape[0]


# ------------------------------------------------------------------------------------------- special radii
SPECIAL_RADII = [float("nan"), 0.0, -0.0, -0.5, 1e-23, 1e-20, 2e-4, 1e20, float("inf")]
SPECIAL_SCENE = {"cylinder2": "cylinder4d", "outer_cyl1": "tiger", "outer_cyl2": "tiger", "inner_cyl1": "tiger",
                 "inner_cyl2": "tiger"}


def special_case(rt4, base, field, radius, seed=4242):
    """(the scene with that one radius set, rays, [(seam, slice of its exact stratum, table)]) of a special-radius
    case: test_gpu_parity.random_rays(20000, seed), the exact strata of the threshold's seams for the changed scene,
    and 4000 rays per seam through points of the filtered faces whose distance to the other pair is spread over
    0 .. twice the original radius, where the original and the special radius decide differently. These last rays
    are not among the inputs the cases were specified with: the random rays and the exact stratum alone leave the
    small inner radii under MIN_DEPENDENT (inner_cyl1 = 1e-20 and 2e-4: 174 of 20 021 rays, 0.87 %)."""
    from test_gpu_parity import random_rays

    d = rt4.SceneDesc.from_buffer_copy(bytes(base))
    radius_field(d, field).r = radius
    rays, parts, at = [random_rays(20000, seed)], [], 20000
    for sm in seams(d):
        if sm.field != field:
            continue
        st, table = exact(sm)
        parts.append((sm, slice(at, at + len(st.rays)), table))
        rays.append(st.rays)
        at += len(st.rays)
    for k, sm in enumerate(s for s in seams(base) if s.field == field):
        e = np.random.default_rng(seed + k).uniform(-1.0, 1.0, 4000)
        rays.append(aimed(sm, seed + 100 + k, 4000, e).rays)
    return d, np.concatenate(rays), parts


# (field, radius) whose filter cannot show on rays of generic direction: the special radius is also the radius of a
# face, that face then answers with a hit at distance NaN, and such a hit wins every closest() it is the second
# argument of (a.dist < NaN is false): the figure's answer is that NaN hit or nothing, never a face at a finite
# distance, whatever the filter decided. Only the exact stratum shows the filter there: its rays miss the NaN face by
# its projection's early-out (their direction has no component in its plane).
MASKED = [("cylinder2", "nan"), ("cylinder2", "0.0"), ("cylinder2", "-0.0"), ("cylinder2", "-0.5"), ("outer_cyl2", "nan")]
MIN_DEPENDENT = 0.01  # a case counts when the oracle's result of this share of its rays depends on the one radius
_special = {}


def special_case_checked(rt4, oracle, field, radius):
    """special_case() of the field's scene with the oracle's results (d, rays, rows, colours, info, parts), after asserting,
    on the oracle alone, that the case counts:
      * a case of MASKED is masked: no ray of generic direction ends on the figure at a finite distance, and some end
        on it at distance NaN; at least one ray of its exact stratum gets another result than with the radius restored;
      * any other case is not masked, and at least MIN_DEPENDENT of its rays get another result than with the radius
        restored.
    info: the counts, for the log."""
    from test_gpu_parity import bits_equal

    key = (field, repr(radius))
    if key not in _special:
        base = rt4.Scene.named(SPECIAL_SCENE[field]).desc
        d, rays, parts = special_case(rt4, base, field, radius)
        c, cc = oracle.find_intersection(d, rays)
        b, bc = oracle.find_intersection(base, rays)
        dep = ~(bits_equal(c, b).all(1) & bits_equal(cc, bc).all(1))
        generic = np.ones(len(rays), bool)
        for _, sl, _ in parts:
            generic[sl] = False
        colors = np.array(sorted({f.color for sm in seams(base) for f in sm.faces}), F32)
        on_figure = (c[:, 0] > 0) & (cc[:, None] == colors[None]).all(2).any(1)
        finite = int((on_figure & np.isfinite(c[:, 1]) & generic).sum())
        nan = int((on_figure & np.isnan(c[:, 1]) & generic).sum())
        masked = finite == 0 and nan > 0
        info = {"rays": len(rays), "dependent": int(dep.sum()), "dependent_exact": int(dep[~generic].sum()),
                "exact": int((~generic).sum()), "finite_figure_hits": finite, "nan_figure_hits": nan, "masked": masked}
        assert masked == (key in MASKED), f"{key}: {info}"
        if masked:
            assert info["dependent_exact"] >= 1, f"{key}: {info}"
        else:
            assert info["dependent"] >= MIN_DEPENDENT * len(rays), f"{key}: {info}"
        _special[key] = (d, rays, c, cc, info, parts)
    return _special[key]


ZOOMS = [2.0 ** -14, 2.0 ** -18, 2.0 ** -20]
_zoom = {}


def zoom_cases(rt4, oracle, name):
    """[(label, uniforms, share)] of a named scene: for every seam kind the view pick_view() finds, at each zoom of
    ZOOMS, with 2 samples and 2 reflections; asserted, on the oracle's frame of the same view with one sample and no
    reflections: the second most frequent pixel value holds at least MIN_CLASS of the pixels (share)."""
    if name not in _zoom:
        d = rt4.Scene.named(name).desc
        reg = rt4.region(64, 40)
        out = []
        for sm in seams(d):
            view = pick_view(rt4, oracle, d, sm)
            assert view is not None, f"{name} {sm.name}: no view of the seam"
            fi, te, psi, face = view
            for mh in ZOOMS:
                flat = zoom_view(rt4, sm, mh, fi=fi, te=te, psi=psi, samples=1, reflections=0, face=face)
                share = two_classes(oracle.render(d, flat, reg)[0])
                label = f"{sm.name} fi {fi} te {te} psi {psi} face {face} height 2^{int(np.log2(mh))}"
                assert share >= MIN_CLASS, f"{name} {label}: smaller class {share:.3f}"
                out.append((label, zoom_view(rt4, sm, mh, fi=fi, te=te, psi=psi, face=face), share))
        _zoom[name] = out
    return _zoom[name]
