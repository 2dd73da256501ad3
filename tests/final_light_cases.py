"""Shared inputs of test_final_light.py and test_gpu_final_light.py (a plain helper, not a fixture): suns, escaping
directions aimed at the boundaries of final_light's shortcuts, and the kernel's fp32 predicates restated in numpy.

final_light of the trace kernels (rt4_trace.hip) is the shader's formula behind three host-derived shortcuts: the sky
pre-test `a <= pre_a || a*a < l2 * sky_pre_k` under a guard on l2, the sky threshold `!(vcos > sky_c_star)` and the
verified divisors (rt4_aux.h). A shortcut can only be wrong in a band of relative width about 1e-5 in cos^2 around its
boundary, so the directions here are generated around those boundaries, not at random.

A sun is a scene: the `sphere` scene's description with only sun and sky_light replaced (a constant-mode case replaces
final_light_mode and final_light_const too). Every generator is seeded by the sun's name and the set's name.
"""
import zlib

import numpy as np

f32 = np.float32
PIO2_UP = f32(np.pi / 2)  # 1.57079637..., above pi/2: c* = 2^-24, still positive (acos(c) = float(pi/2) below that)
PIO2_DN = np.nextafter(PIO2_UP, f32(0))  # below pi/2: c* = 3 * 2^-24; both too small for a sky_pre_k in range
N_MAIN = 1 << 18  # directions of a rim, pre-test or great-circle set (the most a set may have)
N_SIDE = 1 << 16  # directions of a guard or half-space set
L2_LO, L2_HI = f32(2.0 ** -40), f32(2.0 ** 40)  # the pre-test's guard on l2, and the range sky_pre_k must lie in


def _len_for_k(ang, k):
    """A sun length whose sky_pre_k = c*^2 len^2 (1 - 1e-5) is about k (c* is cos(ang) within 1e-6)."""
    return float(np.sqrt(k / (np.cos(ang) ** 2 * (1.0 - 1e-5))))


def _along(length, v=(0.6, 0.0, 0.8, 0.0)):
    return tuple(float(f32(length * x)) for x in v)


# name -> (sun.drct, angular_size, sharpness); "ref_*" take sun and sky_light from the builtin scene of that name
SUNS = {
    "ref_sphere": None, "ref_tiger": None, "ref_hypercube": None, "ref_room": None,
    "ang_1e-3": ((0, 0, 1, 0), 1e-3, 0.5),
    "ang_0.02": ((0, 1, 1, 0), 0.02, 0.5),
    "ang_0.3": ((0, 0, 1, 0), 0.3, 0.5),
    "ang_1.0": ((1, 2, 3, 4), 1.0, 0.5),
    "ang_1.5": ((0, 0, 1, 0), 1.5, 0.5),
    "ang_pio2_dn": ((0, 1, 1, 0), float(PIO2_DN), 0.5),
    "ang_pio2_up": ((0, 1, 1, 0), float(PIO2_UP), 0.5),
    "ang_3.2": ((0, 0, 1, 0), 3.2, 0.5),
    "drct_0110": ((0, 1, 1, 0), 0.3, 0.5),
    "drct_1234": ((1, 2, 3, 4), 0.3, 0.5),
    "drct_3040": ((3, 0, 4, 0), 0.3, 0.5),
    "len_2^-22": (_along(2.0 ** -22), 0.3, 0.5),  # sky_pre_k about 2^-44: outside [2^-40, 2^40], disabled
    "len_2^22": (_along(2.0 ** 22), 0.3, 0.5),    # about 2^44: disabled
    "k_low_in": (_along(_len_for_k(0.3, 2.0 ** -40 * 1.001)), 0.3, 0.5),  # sky_pre_k just inside each end
    "k_high_in": (_along(_len_for_k(0.3, 2.0 ** 40 * 0.999)), 0.3, 0.5),
    "sharp_0": ((0, 1, 1, 0), 0.3, 0.0),
    "sharp_0.7": ((0, 1, 1, 0), 0.3, 0.7),
    "sharp_1.0": ((0, 1, 1, 0), 0.3, 1.0),
    "sharp_1.5": ((0, 1, 1, 0), 0.3, 1.5),  # the pole 1 - s k = 0 lies inside the disc: inf and NaN lights
    "constant": ((0, 1, 1, 0), 0.3, 0.5),   # a valid sun behind a constant override
}
SUN_NAMES = tuple(SUNS)
CONSTANT_RGB = (0.5, 0.25, 0.125)
# Suns whose scene makes a branch of the kernel's final_light empty (test_gpu_final_light.py asserts the others):
#   pre-test: off when c* is not positive: at 3.2 every cosine is in the sun (c* is below -1). A sky_pre_k outside
#   [2^-40, 2^40] only drops the product test, `a <= 0` still fires: the two long and short suns, and both roundings of
#   pi/2, whose c* are 3 * 2^-24 and 2^-24 (the float below the smallest c with acos(c) < ang), both positive;
#   threshold only: empty at 3.2, where no finite cosine is at or below c*; the constant modes return before all three.
CONSTANT_MODE = ("ref_room", "constant")
NO_PRETEST = ("ang_3.2",) + CONSTANT_MODE
NO_THRESHOLD_ONLY = ("ang_3.2",) + CONSTANT_MODE
NO_IN_SUN = CONSTANT_MODE
PRE_K_DISABLED = ("len_2^-22", "len_2^22", "ang_pio2_dn", "ang_pio2_up") + NO_PRETEST  # sky_pre_k = 0

# Candidates of the slow-divisor search (rt4_debug_verify_div(b, full=0) != 0 refuses the 3-op quotient): angular
# sizes and sun lengths, a fixed list. The sun of a length candidate is (b, 0, 0, 0), whose length is b exactly.
# A grid of ordinary values (refused on the MI355X, every one: the 3-op form misses subnormal quotients) and the
# multiples of 1/64 up to 2, whose short mantissas are the ones that get accepted.
DIV_CANDIDATES = tuple(dict.fromkeys([k / 64.0 for k in range(2, 129)]
                                     + [float(f32(0.05) + f32(k) * f32(0.0041)) for k in range(240)]))


def scene(rt4, name, ang=None, drct=None):
    """The sun `name` as an rt4.Scene; ang / drct override the table (the slow-divisor suns)."""
    d = rt4.SceneDesc.from_buffer_copy(rt4.Scene.builtin("sphere").to_bytes())
    if name.startswith("ref_"):
        src = rt4.Scene.builtin(name[4:]).desc
        d.sun = type(d.sun).from_buffer_copy(bytes(src.sun))
        for q in range(3):
            d.sky_light[q] = src.sky_light[q]
            d.final_light_const[q] = src.final_light_const[q]
        d.final_light_mode = src.final_light_mode
        return rt4.Scene(d)
    spec = SUNS.get(name) or ((0, 0, 1, 0), 0.3, 0.5)
    i = SUN_NAMES.index(name) if name in SUNS else len(SUN_NAMES)
    sd = drct if drct is not None else spec[0]
    for q in range(4):
        d.sun.drct[q] = sd[q]
    d.sun.angular_size = ang if ang is not None else spec[1]
    d.sun.sharpness = spec[2]
    sky, light = (0.11 + 0.01 * i, 0.23, 0.47 - 0.01 * i), (9.0 + 0.5 * i, 5.0, 2.5 - 0.05 * i)  # distinct, not grey
    for q in range(3):
        d.sky_light[q], d.sun.light[q] = sky[q], light[q]
    if name == "constant":
        d.final_light_mode = rt4.FINAL_LIGHT_CONSTANT
        for q in range(3):
            d.final_light_const[q] = CONSTANT_RGB[q]
    return rt4.Scene(d)


def _rng(name, what):
    return np.random.default_rng(zlib.crc32(f"{name}/{what}".encode()))


def _sun_unit(desc):
    s = np.array(list(desc.sun.drct), np.float64)
    n = np.linalg.norm(s)
    return s / n if np.isfinite(n) and n > 0 else np.array([0.0, 0.0, 1.0, 0.0])


def _perp(rng, s, n):
    p = rng.normal(size=(n, 4))
    p -= (p @ s)[:, None] * s
    return p / np.linalg.norm(p, axis=1, keepdims=True)


def _around(desc, rng, n, c0, scale_exp):
    """d = c s + sqrt(1 - c^2) p in float64 (p a random unit vector perpendicular to s), c = c0 +- eps with eps = 0
    (one in sixteen) or log-uniform in [1e-8, 1e-2], times 2^scale_exp, rounded to fp32. A c beyond +-1 is mirrored
    there (the direction passes the pole and comes out on the other side), which only the suns below 0.15 rad and
    the one of 3.2 rad reach."""
    s = _sun_unit(desc)
    eps = np.where(rng.integers(0, 16, n) == 0, 0.0, 10.0 ** rng.uniform(-8, -2, n)) * rng.choice([-1.0, 1.0], n)
    c = c0 + eps
    c = np.where(c > 1.0, 2.0 - c, np.where(c < -1.0, -2.0 - c, c))
    d = c[:, None] * s + np.sqrt(1.0 - c * c)[:, None] * _perp(rng, s, n)
    return (d * (2.0 ** scale_exp)[:, None]).astype(f32)


def _c0(desc, what):
    c = np.cos(float(desc.sun.angular_size))
    return c if what == "rim" else c * np.sqrt(1.0 - 1e-5)


def rim(desc, name, n=N_MAIN):
    """Around cos = cos(ang), where the threshold decides; scales 2^-3 .. 2^3."""
    rng = _rng(name, "rim")
    return _around(desc, rng, n, _c0(desc, "rim"), rng.integers(-3, 4, n).astype(np.float64))


def pretest(desc, name, n=N_MAIN):
    """Around cos = cos(ang) sqrt(1 - 1e-5), the pre-test's boundary; scales 2^-3 .. 2^3."""
    rng = _rng(name, "pretest")
    return _around(desc, rng, n, _c0(desc, "pretest"), rng.integers(-3, 4, n).astype(np.float64))


GUARD_EXPS = np.array(list(range(-75, -17)) + list(range(18, 64)), np.float64)


def guard(desc, name, n=N_SIDE):
    """The rim and pre-test directions at scales 2^-75 .. 2^-18 and 2^18 .. 2^63: l2 crosses 2^-40 and 2^40, the
    products reach the subnormal range and overflow."""
    rng = _rng(name, "guard")
    e = rng.choice(GUARD_EXPS, n)
    half = n // 2
    return np.concatenate([_around(desc, rng, half, _c0(desc, "rim"), e[:half]),
                           _around(desc, rng, n - half, _c0(desc, "pretest"), e[half:])])


def halfspace(desc, name, n=N_SIDE):
    """dot(d, s) within +-1e-7 of 0 (the `a <= pre_a` shortcut), and directions opposite the sun."""
    rng = _rng(name, "halfspace")
    s = _sun_unit(desc)
    half = n // 2
    c = np.concatenate([rng.uniform(-1e-7, 1e-7, half), -rng.uniform(0.0, 1.0, n - half)])
    c[:8] = 0.0
    c[half:half + 8] = -1.0
    d = c[:, None] * s + np.sqrt(1.0 - c * c)[:, None] * _perp(rng, s, n)
    return (d * (2.0 ** rng.integers(-3, 4, n).astype(np.float64))[:, None]).astype(f32)


def great_circle(desc, name, n=N_MAIN):
    """n equally spaced angles on a great circle through the sun."""
    s = _sun_unit(desc)
    p = _perp(_rng(name, "circle"), s, 1)[0]
    t = 2.0 * np.pi * np.arange(n) / n
    return (np.cos(t)[:, None] * s + np.sin(t)[:, None] * p).astype(f32)


def specials(desc, name):
    """The zero vector, NaN, +-inf and subnormal components, alone and next to the sun's own direction."""
    s = _sun_unit(desc).astype(f32)
    nan, inf, sub = f32(np.nan), f32(np.inf), f32(1e-42)
    rows = [(0, 0, 0, 0), (-0.0, 0, -0.0, 0), (nan, 0, 0, 0), (0, nan, 1, 0), (nan, nan, nan, nan), (inf, 0, 0, 0),
            (-inf, 0, 0, 0), (0, inf, inf, 0), (inf, -inf, 0, 0), (sub, 0, 0, 0), (0, sub, sub, 0), (-sub, sub, 0, sub),
            (1, sub, 0, 0), (0, 0, f32(1e-38), 0), (f32(3e38), 0, 0, 0), (0, f32(3e38), f32(3e38), 0)]
    out = [np.array(r, f32) for r in rows]
    for v in (nan, inf, -inf, sub, f32(0)):
        for q in range(4):
            d = s.copy()
            d[q] = v
            out.append(d)
    out += [s, -s, s * sub, s * f32(3e38), s * f32(2.0 ** -64), s * f32(2.0 ** 63)]
    return np.array(out, f32)


SETS = {"rim": rim, "pretest": pretest, "guard": guard, "halfspace": halfspace, "circle": great_circle,
        "specials": specials}


def directions(desc, name, sets=tuple(SETS)):
    """{set: (n, 4) float32} for a sun."""
    return {k: SETS[k](desc, name) for k in sets}


# ------------------------------------------------------------------ the kernel's fp32 predicates, in numpy
def fma(a, b, c):
    """One fp32 fma, emulated in float64 (the product of two fp32 values is exact there)."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def dot(a, b):
    """rt4_device_math.h dot: fma(w, w', fma(z, z', fma(y, y', x x')))."""
    with np.errstate(all="ignore"):
        x = (a[..., 0] * b[..., 0]).astype(f32)
    return fma(a[..., 3], b[..., 3], fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], x)))


_c_min = {}


def c_min_sweep(oracle, ang):
    """The smallest float c with acos(c) < ang in the oracle's acos (NaN: none), by a sweep of acos over float
    patterns: every pattern of (0.5, 1] for ang <= 1 (rt4_sky_threshold_kernel gives the reason why no smaller c can
    qualify). Above 1 the sweep covers every pattern with |c - cos(ang)| <= 2^-20 and |c| >= 2^-26, plus +-0: the
    oracle's acos is within 2^-21 of the true one (asserted on the swept patterns) and |d acos / dc| >= 1, so a c below
    the window cannot qualify and every c above it does; for |c| < 2^-26 the result is float(pi/2) - c rounded, which
    is float(pi/2) itself, the value at +-0. An ang above pi + 2^-20 admits every c in [-1, 1]."""
    ang = f32(ang)
    key = ang.tobytes()
    if key in _c_min:
        return _c_min[key]
    EVAL_ACOS = 0
    if not ang > 0:  # NaN, zero or negative: acos is never below it
        res = f32(np.nan)
    elif ang > f32(np.pi + 2.0 ** -20):
        assert oracle.eval_array(EVAL_ACOS, np.array([-1.0], f32))[0][0] < ang
        res = f32(-1.0)
    else:
        if ang <= 1:
            pats = [np.arange(0x3F000001, 0x3F800001, dtype=np.uint32)]
        else:
            c0, w = np.cos(np.float64(ang)), 2.0 ** -20
            lo, hi = f32(c0 - w), f32(c0 + w)
            tiny = f32(2.0 ** -26)
            pats = [np.array([0, 0x80000000], np.uint32)]
            if hi >= tiny:  # positive floats in [max(lo, tiny), hi]
                pats.append(np.arange(max(lo, tiny).view(np.uint32), hi.view(np.uint32) + 1, dtype=np.uint32))
            if lo <= -tiny:  # negative floats in [lo, min(hi, -tiny)]
                pats.append(np.arange(min(hi, -tiny).view(np.uint32), lo.view(np.uint32) + 1, dtype=np.uint32))
        best = f32(np.inf)
        for p in pats:
            for at in range(0, len(p), 1 << 23):
                c = p[at:at + (1 << 23)].view(f32)
                a = oracle.eval_array(EVAL_ACOS, c)[0]
                if ang > 1:
                    assert np.abs(a.astype(np.float64) - np.arccos(c.astype(np.float64))).max() <= 2.0 ** -21
                ok = a < ang
                if ok.any():
                    best = min(best, c[ok].min())
        res = f32(np.nan) if np.isinf(best) else best
    _c_min[key] = res
    return res


def aux(oracle, desc):
    """What build_aux (rt4_trace.hip) derives for final_light: c_star, sun_len, sky_pre_k, pre_a."""
    if desc.final_light_mode != 0:
        return {"c_star": f32(-np.inf), "sun_len": f32(0), "pre_k": f32(0), "pre_a": f32(-np.inf)}
    m = c_min_sweep(oracle, desc.sun.angular_size)
    c_star = f32(np.inf) if np.isnan(m) else np.nextafter(m, f32(-np.inf))
    sd = np.array(list(desc.sun.drct), f32)
    with np.errstate(all="ignore"):
        sun_len = np.sqrt(dot(sd, sd))
    pre_k = f32(0)
    c, ln = float(c_star), float(sun_len)
    if np.isfinite(c) and c > 0 and np.isfinite(ln) and ln > 0:
        k = c * c * ln * ln * (1.0 - 1e-5)
        if 2.0 ** -40 <= k <= 2.0 ** 40:
            pre_k = f32(k)
    pre_ok = c_star > 0
    return {"c_star": c_star, "sun_len": sun_len, "pre_k": pre_k if pre_ok else f32(0),
            "pre_a": f32(0) if pre_ok else f32(-np.inf)}


def pretest_terms(desc, d):
    """a = dot(d, sun.drct), l2 = dot(d, d) and the two products of the pre-test, as the kernel rounds them."""
    sd = np.array(list(desc.sun.drct), f32)
    a, l2 = dot(d, sd[None]), dot(d, d)
    with np.errstate(all="ignore"):
        return a, l2, (a * a).astype(f32)


def pretest_fires(desc, ax, d, margin_k=None, use_guard=True):
    """The kernel's sky pre-test (rt4_trace.hip final_light) on directions d (n, 4) float32. margin_k / use_guard
    exist for the hand mutations of the test's own copy (another sky_pre_k, no range guard on l2)."""
    a, l2, aa = pretest_terms(desc, d)
    k = ax["pre_k"] if margin_k is None else f32(margin_k)
    with np.errstate(all="ignore"):
        fires = (a <= ax["pre_a"]) | (aa < (l2 * k).astype(f32))
        return fires & ((l2 >= L2_LO) & (l2 <= L2_HI) if use_guard else True)


def vcos(desc, ax, d):
    """(dot / length(d)) / length(sun.drct) in IEEE fp32 (shader.frag:45-47; the verified quotient equals x / b)."""
    a, l2, _ = pretest_terms(desc, d)
    with np.errstate(all="ignore"):
        return ((a / np.sqrt(l2)).astype(f32) / ax["sun_len"]).astype(f32)


def is_sky(desc, light):
    """The result equals sky_light bit for bit (n,)."""
    sky = np.array(list(desc.sky_light), f32)
    return (np.ascontiguousarray(light, f32).view(np.uint32) == sky.view(np.uint32)[None]).all(axis=1)


def branches(desc, ax, d, light):
    """(pre-test, threshold only, in sun) of directions d whose oracle final_light is `light`: the first two from the
    fp32 predicates, the third from the result (not the sky's bits)."""
    pre = pretest_fires(desc, ax, d)
    with np.errstate(invalid="ignore"):
        thr = ~pre & ~(vcos(desc, ax, d) > ax["c_star"])
    return pre, thr, ~pre & ~thr & ~is_sky(desc, light)


def same_bits(a, b):
    """Equal bit for bit, NaN == NaN (any payload)."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
