"""executable/shader.frag restated in numpy, vectorised over rays and pixels: the independent reference of
test_scene_shapes.py, test_shader_f64.py and test_gpu_shader_f64.py (a plain helper, not a fixture).

Written from the shader (line numbers cited), not from oracle/rt4_oracle.cpp or the kernel headers; it imports
neither the oracle nor the library and reads rt4_scene_desc / rt4_uniforms ctypes objects as data only.

Two formulations of the sphere test, chosen by the dtype:
  * float64 (the reference): the closed form, the roots of |o + t d - c| = r (_quadratic). It shares nothing with the
    shader's acos / asin chain, so a misreading of that chain shows against it.
  * any other dtype (float32: what a GL driver's fp32 would do with the shader as written): the acos / asin chain
    of shader.frag:197-221 literally, PI = 3.14159265f included. It exists only to size the tolerances: E_ref of the
    tests is the difference between this run and the float64 one.
Everything else is one set of expressions evaluated in the dtype. The integer RNG (hash, random_uint, the mantissa
trick of rand(), the comparison of rand_outcome) and scr_coord are exact uint32 / float32 whatever the dtype: they
are bit-level definitions and they decide the random path.

The float64 run also says where it cannot be trusted to decide like an fp32 evaluation: a ray is `ambiguous` when a
discrete decision of find_intersection sits within MARGIN of its boundary (see find()), a pixel when any
find_intersection of any of its paths was.
"""
import numpy as np

SMALL_FLOAT = 0.0003  # shader.frag:24
PI32 = float(np.float32(3.14159265))  # shader.frag:23, the value the fp32 constant has
# Below the small_indent of every test that uses this file (0.005, rt4.make_uniforms' default): a bounce origin
# lies small_indent off the surface it left, which must not count as "on the surface".
MARGIN = 1e-3
# A cosine of two unit vectors carries an fp32 error of a few 2^-24, some 1e-5 after three bounces: a ray whose cosine
# with a space is exactly zero (every primary ray of the default camera, w = 0, against a wall w = const) is a miss in
# any arithmetic. Below SMALL_FLOAT, so that such a ray is kept.
MISS_MARGIN = 1e-4
# The shader's sphere test goes through acos(cos_opa) with cos_opa near 1 for a far origin and through asin(sin_oap)
# with sin_oap near 1 for a grazing hit: in fp32 the hit point moves along the surface by about
# 2^-24 * max(1, (len_po / r)^2) / |cos of incidence| radii, times a constant for the roundings of the chain. find()
# returns that factor (`cond`, 0 for spaces and cells); a hit with 2^-24 * cond above COND_LIMIT is ill-conditioned
# and its normal is compared with nothing (the hit flag, winner, material and distance still are). The limit is the
# largest E_ref a normal may have, (1e-3 / 4), over a constant of 10.
COND_LIMIT = 2.5e-5
NEWTON_CAP = 64  # w_by_volume's loop has no cap in the shader; this one only turns a runaway into an error


def _vec(a, T=np.float64):
    return np.array(a[:4], T)


def _dot(a, b):
    return (a * b).sum(-1)


# ------------------------------------------------------------------------------ single objects, closed form
def _quadratic(po, dn, r, outer):
    """Ray from the origin o with unit direction dn against |x - c| = r, po = c - o (any dimension).
    Returns (hit, t, ambiguous). Near root from outside when `outer`, far root otherwise.

    An origin within SMALL_FLOAT of the centre takes the sphere test's own branch (shader.frag:202-203): cos_opa = 0
    whatever the direction, which in exact arithmetic makes sin_oap = len_po / r and dist = sqrt(r^2 - len_po^2). The
    default camera sits exactly on the axes plane of the reference's tiger and 4D cylinder, so every primary ray of
    those scenes takes it. Around the branch's threshold, from half of it to twice, the ray is ambiguous."""
    b = (po * dn).sum(1)
    l2 = (po * po).sum(1)
    len_po = np.sqrt(l2)
    disc = b * b - (l2 - r * r)
    outside = l2 > r * r
    centred = len_po < SMALL_FLOAT
    hit = np.where(centred, ~outside, (disc > 0) & ~(outside & (b < 0)))
    root = np.sqrt(np.maximum(disc, 0))
    t = np.where(centred, np.sqrt(np.maximum(r * r - l2, 0)), np.where(outside & bool(outer), b - root, b + root))
    amb = (np.abs(disc) <= MARGIN * r * r) | (np.abs(len_po - r) <= MARGIN * max(1.0, r))
    amb |= (len_po >= SMALL_FLOAT / 2) & (len_po < 2 * SMALL_FLOAT)
    return hit, t, amb


def _ball_normal(po, dn, t, r, outer):
    """(c - (p + d * dist)) / r, negated for a hit from outside with `outer` (shader.frag:218-219), and the fp32
    loss of the shader's acos / asin chain at this hit as a factor of 2^-24 (COND_LIMIT)."""
    norm = (po - dn * t[:, None]) / r
    l2 = (po * po).sum(1)
    flip = (l2 > r * r) & bool(outer)
    with np.errstate(all="ignore"):
        cond = np.maximum(1.0, l2 / (r * r)) / np.abs((dn * norm).sum(1))
    return np.where(flip[:, None], -norm, norm), cond


def _space(s, o, dn, T=np.float64):
    """space_intersection (shader.frag:231-239): (hit, t, norm, ambiguous, cond = 0). The normal is -drct_h, the
    unit normal on the ray's side."""
    p, n = _vec(s.point, T), _vec(s.norm, T)
    vn = (p - o) @ n
    sgn = np.sign(vn)
    cos = sgn * (dn @ n)
    hit = cos >= T(SMALL_FLOAT)
    t = np.abs(vn) / np.where(hit, cos, T(1))
    # a hit with a cosine just above the threshold is far away and ill-conditioned (dist = |vn| / cos), hence the
    # whole MARGIN on that side; a miss only has to be a robust one
    amb = ((cos > SMALL_FLOAT - MISS_MARGIN) & (cos <= SMALL_FLOAT + MARGIN)) | (np.abs(vn) <= MARGIN)
    return hit, t, -sgn[:, None] * n, amb, np.zeros(len(o))


def _sphere(s, o, dn, outer):
    po, r = _vec(s.center) - o, float(s.r)
    hit, t, amb = _quadratic(po, dn, r, outer)
    norm, cond = _ball_normal(po, dn, t, r, outer)
    return hit, t, norm, amb, cond


def _cylinder(c, o, dn, outer):
    """The quadratic on the ray projected off the two axes; t is rescaled by the projected direction's length.
    Returns (hit, t, norm, ambiguous, cond); the normal lies in the plane orthogonal to both axes."""
    a1, a2 = _vec(c.axis1), _vec(c.axis2)

    def off_axes(v):
        v = v - (v @ a1)[:, None] * a1
        return v - (v @ a2)[:, None] * a2

    po, dp = off_axes(_vec(c.point) - o), off_axes(dn)
    ln = np.linalg.norm(dp, axis=1)
    ok = ln >= SMALL_FLOAT
    safe = np.where(ok, ln, 1.0)
    dpn = dp / safe[:, None]
    hit, t, amb = _quadratic(po, dpn, float(c.r), outer)
    norm, cond = _ball_normal(po, dpn, t, float(c.r), outer)
    return hit & ok, t / safe, norm, amb | (np.abs(ln - SMALL_FLOAT) <= MARGIN), cond


# -------------------------------------------------------------------- single objects, the shader as written
def _point_in_space(p, sp, sn):
    """point_in_space (shader.frag:64-71)."""
    return p + sn * _dot(sp - p, sn)[:, None]


def _sphere_written(center, r, p, dn, outer, T):
    """sphere_intersection (shader.frag:197-221), statement by statement in T: (hit, dist, norm, ambiguous, 0)."""
    pi, small = T(PI32), T(SMALL_FLOAT)
    po = center - p
    len_po = np.sqrt(_dot(po, po))
    centred = len_po < small  # :202
    dot_pord = _dot(po, dn)
    miss = ~centred & (len_po >= r) & (dot_pord < 0)  # :206
    with np.errstate(all="ignore"):
        cos_opa = np.where(centred, T(0), np.clip(dot_pord / np.where(centred, T(1), len_po), T(-1), T(1)))  # :207-209
        angle_opa = np.arccos(cos_opa)
        sin_oap = len_po * np.sin(angle_opa) / r
        miss |= sin_oap >= 1  # :213
        angle_oap = np.arcsin(np.minimum(sin_oap, T(1)))
        flip = bool(outer) & (len_po > r)
        angle_oap = np.where(flip, pi - angle_oap, angle_oap)  # :215
        angle_aop = pi - angle_opa - angle_oap
        dist = np.sqrt(r * r + len_po * len_po - T(2) * r * len_po * np.cos(angle_aop))  # :217
    norm = (center - (p + dn * dist[:, None])) / r
    norm = np.where(flip[:, None], -norm, norm)
    amb = (np.abs(1 - sin_oap) <= MARGIN) | (np.abs(len_po - r) <= MARGIN * max(1.0, float(r)))
    amb |= (len_po >= small / 2) & (len_po < 2 * small)
    return ~miss, dist.astype(T), norm.astype(T), amb, np.zeros(len(p))


def _cylinder_written(c, p, dn, outer, T):
    """cylinder_intersection (shader.frag:251-267) in T."""
    cp, a1, a2, small = _vec(c.point, T), _vec(c.axis1, T), _vec(c.axis2, T), T(SMALL_FLOAT)
    p1, d1 = _point_in_space(p, cp, a1), dn - a1 * _dot(dn, a1)[:, None]
    ok = ~(np.sqrt(_dot(d1, d1)) < small)  # :253
    p12, d12 = _point_in_space(p1, cp, a2), d1 - a2 * _dot(d1, a2)[:, None]
    ln = np.sqrt(_dot(d12, d12))
    ok &= ~(ln < small)  # :257
    safe = np.where(ok, ln, T(1))
    hit, dist, norm, amb, cond = _sphere_written(cp, T(c.r), p12, d12 / safe[:, None], outer, T)
    return hit & ok, dist / safe, norm, amb | (np.abs(ln - small) <= MARGIN), cond


def _dist_to_axes_plane(dist, o, dn, c, T):
    """dist_to_axes_plane (shader.frag:270-275)."""
    cp = _vec(c.point, T)
    point = o + dn * dist[:, None]
    p1 = _point_in_space(point, cp, _vec(c.axis1, T))
    p12 = _point_in_space(p1, cp, _vec(c.axis2, T))
    return np.sqrt(_dot(cp - p12, cp - p12))


# --------------------------------------------------------------------------------------------- candidates
class Cand:
    """An `intersection` (shader.frag:171-176) per ray; surface is the flat number of rt4.h rt4_scene_surface, part the
    piece of a composite (union cylinder 0..1, cell 0..7, the tiger's face test 0..7 in the order of :328-335)."""

    def __init__(self, hit, t, norm, surface, part=0, cond=0.0):
        n = len(hit)
        self.hit = hit
        self.cond = np.where(hit, cond, 0.0)
        self.t = np.where(hit, t, 0)  # NOT_INTERSECT.dist (:178): the band checks read it
        self.norm = np.where(hit[:, None], norm, 0)
        self.surface = np.where(hit, surface, -1) if np.ndim(surface) else np.where(hit, np.full(n, surface), -1)
        self.part = np.where(hit, part, -1) if np.ndim(part) else np.where(hit, np.full(n, part), -1)


def _closest(a, b):
    """closest(inter1, inter2) (shader.frag:181-185): on a tie the second argument."""
    take_a = a.hit & (~b.hit | (a.t < b.t))
    out = Cand.__new__(Cand)
    out.hit = a.hit | b.hit
    out.t = np.where(take_a, a.t, b.t)
    out.norm = np.where(take_a[:, None], a.norm, b.norm)
    out.surface = np.where(take_a, a.surface, b.surface)
    out.part = np.where(take_a, a.part, b.part)
    out.cond = np.where(take_a, a.cond, b.cond)
    return out


def surface_bases(d):
    """First flat surface number of each kind (rt4.h rt4_scene_surface: the arrays in order, tested or not)."""
    counts = [d.n_spaces, d.n_spheres, d.n_cylinders, 2 * d.n_unions, 8 * d.n_hypercubes, 4 * d.n_tigers]
    return dict(zip(range(1, 7), np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()))


def surface_materials(d):
    """(glow, refl_prob, colour (n, 3)) float32 tables indexed by surface number."""
    mats = [d.spaces[i].material for i in range(d.n_spaces)] + [d.spheres[i].material for i in range(d.n_spheres)]
    mats += [d.cylinders[i].material for i in range(d.n_cylinders)]
    for i in range(d.n_unions):
        mats += [d.unions[i].cylinder1.material, d.unions[i].cylinder2.material]
    for i in range(d.n_hypercubes):
        mats += [c.material for c in d.hypercubes[i].cubes]
    for i in range(d.n_tigers):
        t = d.tigers[i]
        mats += [t.inner_cyl1.material, t.outer_cyl1.material, t.inner_cyl2.material, t.outer_cyl2.material]
    glow = np.array([m.glow for m in mats] + [0.0], np.float32)  # the last entry serves surface -1 (a miss)
    refl = np.array([m.refl_prob for m in mats] + [0.0], np.float32)
    col = np.array([list(m.color) for m in mats] + [[0.0] * 3], np.float32).reshape(-1, 3)
    return glow, refl, col


class _Finder:
    """One find_intersection (shader.frag:434-451) over n rays."""

    def __init__(self, d, o, dn, T, union_check2_r1=False, as_written=False):
        self.d, self.o, self.dn, self.T = d, o, dn, T
        self.closed = T == np.float64 and not as_written
        self.n = len(o)
        self.amb = np.zeros(self.n, bool)
        self.leaves = []  # every candidate that entered a closest(): (hit, t, surface)
        self.union_check2_r1 = union_check2_r1
        self.not_nearest = np.zeros(self.n, bool)  # a hypercube returned a cell that is not its nearest hitting one
        self.inside_cube = np.zeros(self.n, bool)  # h < 0 for all eight cells of some tested hypercube

    def leaf(self, c):
        self.leaves.append((c.hit, c.t, c.surface))
        return c

    def cylinder(self, c, outer):
        if self.closed:
            return _cylinder(c, self.o, self.dn, outer)
        return _cylinder_written(c, self.o, self.dn, outer, self.T)

    def band(self, cand_hit, t, cyl, r):
        """dist_to_axes_plane(inter.dist, ray, cyl) and its distance from r; near r is ambiguous if the candidate's
        own cylinder test accepted it."""
        dap = _dist_to_axes_plane(np.where(cand_hit, t, 0).astype(self.T), self.o, self.dn, cyl, self.T)
        self.amb |= cand_hit & (np.abs(dap - r) <= MARGIN * max(1.0, float(r)))
        return dap

    def union(self, u, base):
        """cylinders_union_intersection (shader.frag:284-294); both band checks compare with cylinder2.r (:286, :290)."""
        T = self.T
        h1, t1, n1, a1, c1 = self.cylinder(u.cylinder1, True)
        self.amb |= a1
        h1 = h1 & ~(self.band(h1, t1, u.cylinder2, T(u.cylinder2.r)) > T(u.cylinder2.r))
        h2, t2, n2, a2, c2 = self.cylinder(u.cylinder2, True)
        self.amb |= a2
        r_second = T(u.cylinder1.r) if self.union_check2_r1 else T(u.cylinder2.r)
        h2 = h2 & ~(self.band(h2, t2, u.cylinder1, r_second) > r_second)
        return _closest(self.leaf(Cand(h1, t1, n1, base, 0, c1)), self.leaf(Cand(h2, t2, n2, base + 1, 1, c2)))

    def tiger(self, t, base):
        """tiger_intersection (shader.frag:327-341): eight tigers_face_intersection (:317-324) and closest's tree."""
        T = self.T
        faces = []
        for k, (cyl, s, outer_cyl, inner_cyl) in enumerate((
                (t.inner_cyl1, 0, t.outer_cyl2, t.inner_cyl2), (t.outer_cyl1, 1, t.outer_cyl2, t.inner_cyl2),
                (t.inner_cyl2, 2, t.outer_cyl1, t.inner_cyl1), (t.outer_cyl2, 3, t.outer_cyl1, t.inner_cyl1))):
            for j, outer in enumerate((True, False)):
                h, dist, norm, a, cond = self.cylinder(cyl, outer)
                self.amb |= a
                keep = h & ~(self.band(h, dist, outer_cyl, T(outer_cyl.r)) > T(outer_cyl.r))  # :321
                keep &= ~(self.band(h, dist, inner_cyl, T(inner_cyl.r)) < T(inner_cyl.r))  # :322
                faces.append(self.leaf(Cand(keep, dist, norm, base + s, 2 * k + j, cond)))
        c = _closest
        return c(c(c(faces[0], faces[1]), c(faces[2], faces[3])), c(c(faces[4], faces[5]), c(faces[6], faces[7])))

    def hypercube(self, hc, base):
        """hypercube_intersection (shader.frag:394-400): the first cell in array order that hits; cube_intersection
        (:352-366) per cell. A cell after the first hit is never evaluated, so it cannot make the ray ambiguous."""
        T, o, dn, n = self.T, self.o, self.dn, self.n
        found = Cand(np.zeros(n, bool), np.zeros(n, T), np.zeros((n, 4), T), -1, -1)
        nearest, all_behind = np.full(n, np.inf), np.ones(n, bool)
        for k, cube in enumerate(hc.cubes):
            r, pt, vec_n = T(cube.r), _vec(cube.point, T), -_vec(cube.norm, T)
            h = (pt - o) @ vec_n
            cos_dn = dn @ vec_n
            front = ~(h < 0) & ~(cos_dn < 0)  # :356, :358
            with np.errstate(all="ignore"):
                dist = h / cos_dn
                vec_cp = (o + dn * dist[:, None]) - pt
                side = [np.abs(vec_cp @ _vec(ax, T)) for ax in (cube.x, cube.y, cube.z)]
                hit = front & ~(side[0] > r) & ~(side[1] > r) & ~(side[2] > r)  # :362-364
                amb = (np.abs(h) <= MARGIN) | (~(h < 0) & (np.abs(cos_dn) <= MARGIN))  # :358 runs only after :356
                for s in side:
                    amb |= front & ~(np.abs(s - r) > MARGIN * max(1.0, float(r)))
            pending = ~found.hit
            self.amb |= pending & amb
            all_behind &= h < 0
            nearest = np.where(hit, np.minimum(nearest, dist), nearest)
            # a cell is taken only where no earlier one hit, so closest() never has two hits to compare here
            found = _closest(found, Cand(hit & pending, dist, np.broadcast_to(_vec(cube.norm, T), (n, 4)), base + k, k))
        self.not_nearest |= found.hit & (found.t > nearest)
        self.inside_cube |= all_behind
        return self.leaf(found)

    def run(self):
        d, o, dn, T, n = self.d, self.o, self.dn, self.T, self.n
        base = surface_bases(d)
        inter = Cand(np.zeros(n, bool), np.zeros(n, T), np.zeros((n, 4), T), -1, -1)
        for g in d.groups[: d.n_groups]:
            for i in range(g.first, g.first + g.count):
                if g.kind == 1:
                    hit, t, norm, a, cond = _space(d.spaces[i], o, dn, T)
                    new = self.leaf(Cand(hit, t, norm, base[1] + i))
                elif g.kind == 2:
                    s = d.spheres[i]
                    hit, t, norm, a, cond = (_sphere(s, o, dn, g.outer) if self.closed else
                                             _sphere_written(_vec(s.center, T), T(s.r), o, dn, g.outer, T))
                    new = self.leaf(Cand(hit, t, norm, base[2] + i, 0, cond))
                elif g.kind == 3:
                    hit, t, norm, a, cond = self.cylinder(d.cylinders[i], g.outer)
                    new = self.leaf(Cand(hit, t, norm, base[3] + i, 0, cond))
                elif g.kind == 4:
                    new, a = self.union(d.unions[i], base[4] + 2 * i), False
                elif g.kind == 5:
                    new, a = self.hypercube(d.hypercubes[i], base[5] + 8 * i), False
                elif g.kind == 6:
                    new, a = self.tiger(d.tigers[i], base[6] + 4 * i), False
                else:
                    raise ValueError(f"group kind {g.kind} is not one of shader.frag's")
                self.amb |= a
                # closest(new, inter): the new hit wins when strictly nearer; closest(inter, new): also on a tie
                inter = _closest(new, inter) if g.new_first else _closest(inter, new)
        # the second nearest candidate; the winner itself met again (an object listed twice, a tiger's cylinder under
        # both values of `outer` seen from inside) is the same hit, not a rival
        second = np.full(n, np.inf)
        for hit, t, surface in self.leaves:
            rival = hit & ~((surface == inter.surface) & (t == inter.t))
            second = np.where(rival, np.minimum(second, t), second)
        with np.errstate(invalid="ignore"):
            self.amb |= inter.hit & (second - inter.t <= MARGIN * np.maximum(1.0, inter.t))
        return inter


def find(d, o, dn, dtype=np.float64, union_check2_r1=False, as_written=False):
    """find_intersection (shader.frag:434-451) of the rays (o, dn) as given (dn is not normalised here, as in the
    shader). Returns a dict: hit, dist, norm, surface, part, glow / refl_prob / color (float32, the winner's material),
    ambiguous, cond (see COND_LIMIT), and two scene-design aids: not_nearest (a hypercube returned a cell that is not its nearest hitting
    one), inside_cube (the origin is behind all eight cells of a tested hypercube).

    Ambiguous, from this run's own values: some evaluated test sits on a boundary (a sphere's normalised discriminant
    near zero, the origin within MARGIN of a sphere's, cylinder's, space's or cell's surface, a plane or cell cosine
    near its threshold, a projected direction near SMALL_FLOAT, a band check of an accepted union / tiger candidate
    or a cell's side check within MARGIN of its radius), or the two nearest candidates are within a relative MARGIN
    of each other. union_check2_r1: the union's second band check with cylinder1.r, the obvious misreading of :290.
    as_written: the shader's acos / asin chain for spheres and cylinders in float64 too (any other dtype always)."""
    T = np.dtype(dtype).type
    f = _Finder(d, np.asarray(o, T), np.asarray(dn, T), T, union_check2_r1, as_written)
    c = f.run()
    glow, refl, col = surface_materials(d)
    return dict(hit=c.hit, dist=c.t, norm=c.norm, surface=c.surface, part=c.part, glow=glow[c.surface],
                refl_prob=refl[c.surface], color=col[c.surface], ambiguous=f.amb, cond=c.cond,
                not_nearest=f.not_nearest, inside_cube=f.inside_cube)


def ill_conditioned(cond):
    return 2.0 ** -24 * np.asarray(cond) > COND_LIMIT


def ref_find_rays(d, rays, dtype=np.float64, **kw):
    """find() of (n, 8) rays (point, direction); the direction is normalised first, in the dtype."""
    T = np.dtype(dtype).type
    rays = np.asarray(rays, T)
    return find(d, rays[:, :4], rays[:, 4:] / np.sqrt(_dot(rays[:, 4:], rays[:, 4:]))[:, None], T, **kw)


def ref_find_intersection(d, rays):
    """find_intersection in float64: (hit, winner colour (n, 3), distance, ambiguous); ref_find_rays has the rest."""
    r = ref_find_rays(d, rays)
    return r["hit"], r["color"], np.where(r["hit"], r["dist"], 0.0), r["ambiguous"]


# ---------------------------------------------------------------------------------------------------- RNG
def hash_u32(x):
    """hash (shader.frag:94-102) on uint32 arrays (wrapping)."""
    x = x.astype(np.uint32).copy()
    x += x << np.uint32(10)
    x ^= x >> np.uint32(6)
    x += x << np.uint32(3)
    x ^= x >> np.uint32(11)
    x += x << np.uint32(15)
    x ^= x >> np.uint32(9)
    return x


class Rng:
    """The per-pixel stream (shader.frag:90-118): rand_iter_seed starts at uint(seed) for every pixel and runs on
    over the bounces and samples of that pixel; only the lanes of `mask` draw."""

    def __init__(self, seed, scr_bits_x, scr_bits_y):
        self.uint_seed = np.uint32(seed & 0xFFFFFFFF)
        self.iter = np.full(scr_bits_x.shape, self.uint_seed, np.uint32)
        self.scr = scr_bits_x ^ (scr_bits_y << np.uint32(9))  # :106-107

    def rand(self, mask):
        """rand() (:111-118) as float32, exact; lanes outside the mask keep their state (their value is unused)."""
        self.iter = np.where(mask, self.iter + np.uint32(0x79A010A9), self.iter)  # :105
        bits = hash_u32(self.scr ^ self.iter ^ self.uint_seed)
        bits = (bits & np.uint32(0x007FFFFF)) | np.uint32(0x3F800000)
        return bits.view(np.float32) - np.float32(1.0)


# ------------------------------------------------------------------------------------------------ sampler
def _volume_by_w(w, T):
    with np.errstate(invalid="ignore"):
        return (w * np.sqrt(1 - w * w) - np.arccos(w)) / T(PI32) + 1  # :136-138


def w_by_volume(v, T):
    """The Newton loop as written (shader.frag:141-150), each lane until its own step is below SMALL_FLOAT."""
    small = T(SMALL_FLOAT)
    new_w, done = np.zeros_like(v), np.zeros(v.shape, bool)
    for _ in range(NEWTON_CAP):
        old_w = new_w
        old_v = _volume_by_w(old_w, T)
        df = np.where(old_w > 0, old_v - _volume_by_w(old_w - small, T), _volume_by_w(old_w + small, T) - old_v)
        with np.errstate(all="ignore"):
            new_w = np.where(done, old_w, old_w - small / df * (old_v - v))
        done |= ~(np.abs(new_w - old_w) >= small)
        if done.all():
            return new_w
    raise RuntimeError("w_by_volume did not converge")


def rand_drct(rng, mask, T):
    """rand_drct (shader.frag:153-158): three rands in the order w, z, fi."""
    pi = T(PI32)
    w = w_by_volume(rng.rand(mask).astype(T), T)
    with np.errstate(invalid="ignore"):
        r = np.sqrt(1 - w * w)
        z = (rng.rand(mask).astype(T) * 2 - 1) * r
        rr = np.sqrt(r * r - z * z)
    fi = rng.rand(mask).astype(T) * 2 * pi
    return np.stack([rr * np.cos(fi), rr * np.sin(fi), z, w], axis=1)  # cyl_vec_to_vec :128-130


# ------------------------------------------------------------------------------------------------- pixels
def final_light(d, drct, T):
    """final_light (shader.frag:454-468), or the constant of an override (rt4.h RT4_FINAL_LIGHT_CONSTANT):
    (light (n, 3), the ray ends inside the sun's disc)."""
    n = len(drct)
    if d.final_light_mode == 1:
        return np.broadcast_to(np.array(list(d.final_light_const), T), (n, 3)), np.zeros(n, bool)
    sky, sun, light = np.array(list(d.sky_light), T), _vec(d.sun.drct, T), np.array(list(d.sun.light), T)
    size, s = T(d.sun.angular_size), T(d.sun.sharpness)
    with np.errstate(all="ignore"):
        deviation = np.arccos(_dot(drct, sun) / np.sqrt(_dot(drct, drct)) / np.sqrt(_dot(sun, sun)))  # :45-50, :459
        k = deviation / size
        k = (s * s * k / (1 - s * k) + 1) * (1 - k)  # :463
    in_sun = deviation < size  # false for a NaN deviation
    return np.where(in_sun[:, None], light * k[:, None] + sky * (1 - k)[:, None], sky), in_sun


def region_rows(region):
    i = np.arange(region.h)
    if region.band_rows > 0:
        return region.y0 + (i // region.band_rows) * region.band_step + i % region.band_rows
    return region.y0 + i


def ref_pixels(desc, uniforms, region, old=None, dtype=np.float64):
    """main() (shader.frag:513-528) for every pixel of a region. Row i of the image is gl_FragCoord.y = i + 0.5
    (rt4.h conventions: row 0 is the top of the displayed image). old: the (h, w, 4) old_frame, zeros if None.

    Returns a dict: rgba (h, w, 4) in the dtype, counts (find_intersection calls per pixel), the primary hit
    (hit, depth: +inf on a miss, normal, surface: -1 on a miss, glow, refl_prob, primary_ambiguous, primary_cond),
    in_sun (the primary ray ends in deviation < angular_size) and ambiguous (any find_intersection of any path of
    the pixel was)."""
    T = np.dtype(dtype).type
    u, h, w = uniforms, region.h, region.w
    n = h * w
    ys, xs = np.meshgrid(region_rows(region), region.x0 + np.arange(w), indexing="ij")
    # scr_coord = gl_FragCoord.xy / resolution in fp32 (:515-516); its bits seed the hash
    scr_x = ((xs.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(u.resolution[0])).astype(np.float32)
    scr_y = ((ys.ravel().astype(np.float32) + np.float32(0.5)) / np.float32(u.resolution[1])).astype(np.float32)
    rng = Rng(u.seed, scr_x.view(np.uint32), scr_y.view(np.uint32))
    # ray_drct (:501-505)
    mx = (scr_x.astype(T) - T(0.5)) * T(u.mtr_sizes[0])
    my = (T(0.5) - scr_y.astype(T)) * T(u.mtr_sizes[1])
    drct0 = _vec(u.vec_to_mtr, T) + _vec(u.top_drct, T) * my[:, None] + _vec(u.right_drct, T) * mx[:, None]
    drct0 = drct0 / np.sqrt(_dot(drct0, drct0))[:, None]
    indent = T(u.small_indent)

    light = np.zeros((n, 3), T)
    counts, amb = np.zeros(n, np.uint32), np.zeros(n, bool)
    primary = None
    for _ in range(u.samples):  # :520-521
        point, drct = np.broadcast_to(_vec(u.focus, T), (n, 4)).copy(), drct0.copy()
        result, unabsorbed = np.zeros((n, 3), T), np.ones((n, 3), T)
        alive = np.ones(n, bool)
        for _ in range(u.reflections_amount + 1):  # trace :471-495
            idx = np.flatnonzero(alive)
            if not len(idx):
                break
            f = find(desc, point[idx], drct[idx], T)
            counts[idx] += 1
            amb[idx] |= f["ambiguous"]
            hit = f["hit"]
            missed = idx[~hit]
            fl, in_sun = final_light(desc, drct[missed], T)
            if primary is None:
                primary = dict(f)
                primary["in_sun"] = np.zeros(n, bool)
                primary["in_sun"][missed] = in_sun
            light[missed] += result[missed] + unabsorbed[missed] * fl  # :478
            alive[missed] = False
            k, fh = idx[hit], {key: v[hit] for key, v in f.items()}
            color = fh["color"].astype(T)
            result[k] += color * fh["glow"].astype(T)[:, None] * unabsorbed[k]  # :481
            unabsorbed[k] *= color  # :482
            point[k] += drct[k] * fh["dist"][:, None] + fh["norm"] * indent  # :485
            lane = np.zeros(n, bool)
            lane[k] = True
            reflects = ~(rng.rand(lane)[k] > fh["refl_prob"])  # rand_outcome :121, float32 against float32
            diffuse = np.zeros(n, bool)
            diffuse[k[~reflects]] = True
            rd = rand_drct(rng, diffuse, T)[k]
            dot = _dot(rd, fh["norm"])
            redirected = np.where((dot >= 0)[:, None], rd, rd - 2 * dot[:, None] * fh["norm"])  # redirect :82-85
            nd = _dot(fh["norm"], drct[k])
            reflected = drct[k] - 2 * nd[:, None] * fh["norm"]  # GLSL reflect(I, N) = I - 2 dot(N, I) N
            drct[k] = np.where(reflects[:, None], reflected, redirected)
        light[alive] += result[alive]  # :494
    light = light / T(u.samples)  # :522
    new = 1 - 1 / (T(u.light_to_color_conversion_coefficient) * light + 1)  # :509-511
    old_rgb = np.zeros((n, 3), T) if old is None else np.asarray(old, T).reshape(n, 4)[:, :3]
    part = T(u.part)
    rgba = np.concatenate([old_rgb * (1 - part) + new * part, np.ones((n, 1), T)], axis=1)  # mix :526-527
    hit = primary["hit"]
    return dict(rgba=rgba.reshape(h, w, 4), counts=counts.reshape(h, w), ambiguous=amb.reshape(h, w),
                hit=hit.reshape(h, w), depth=np.where(hit, primary["dist"], np.inf).reshape(h, w),
                normal=primary["norm"].reshape(h, w, 4), surface=primary["surface"].reshape(h, w),
                glow=primary["glow"].reshape(h, w), refl_prob=primary["refl_prob"].reshape(h, w),
                in_sun=primary["in_sun"].reshape(h, w), primary_ambiguous=primary["ambiguous"].reshape(h, w),
                primary_cond=primary["cond"].reshape(h, w))
