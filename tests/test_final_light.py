"""final_light at the sun's rim and at the boundaries of the kernel's shortcuts, on the CPU (no GPU needed): the oracle
against the float64 reference, and the sky pre-test's derivation (rt4_trace.hip build_aux) checked on the kernel's
fp32 op sequence in numpy, in the style of test_cyl_precull.py. Inputs: final_light_cases.py. test_gpu_final_light.py
runs the kernels on the same inputs.

a. Oracle against shader_f64.final_light in float64, per sun of angular size <= 1 on its rim, pre-test and great-circle
sets together (3 x 2^18 directions). Rules of the reference alone:
  * a direction is ambiguous (nothing compared) iff |cos(dev64) - cos(ang)| <= 8 * 2^-24, the rim, or
    cos(dev64) >= 1 - 8 * 2^-24, the centre. The second band is a finding of this test: in fp32 the two divisions of
    v_cos (shader.frag:45-47) can round a cosine of a direction within 3.5e-4 rad of the sun's centre to 1.0000001, acos
    of which is NaN, so the shader as written in fp32 (numpy, the oracle and the kernels alike) returns the sky in the
    middle of the sun where float64 returns the full light. On 2^18 points of a great circle about 10 are such.
  * a direction inside the disc is ill-conditioned (branch compared, light not) iff |d light / d cos| exceeds 1000
    times the light's scale: |dg/dk| / (ang sin(dev)) > COND_LIMIT for the profile g(k) = (s^2 k / (1 - s k) + 1) (1 - k),
    k = dev / ang. An fp32 cosine carries about 4 * 2^-24, so beyond that limit no fp32 evaluation can stay within a
    quarter of the cap below. This takes out the few great-circle points within 2.5e-3 rad of the centre (acos is
    singular at 1) and the surroundings of the pole 1 - s k = 0 of sharp_1.5, where the light is unbounded.
  * suns below MIN_ANG = 0.15 rad (1e-3 and 0.02) are left out for the reason the issue leaves out those above 1.3: the
    two bands merge (a disc of 1e-3 rad spans 8 ulp of cosine below 1), and offsets of up to 1e-2 in cosine pass the
    centre, so that at most 13 % of a case can be kept inside. Their shortcuts are covered by b and on the GPU.
On every kept direction the branch (sun or sky, read off the oracle by whether the result is sky_light's bits) agrees;
on every kept, well-conditioned one the light is within min(4 * E_ref, 1e-3 * max(sun.light)), E_ref being the largest
difference there between the reference run in numpy fp32 and in float64. At most 20 % of a case is ambiguous; kept-in
and kept-out are at least 20 % each.

Measured here (reference alone):
  sun            ambiguous   kept in  kept out  ill-cond.   E_ref     bound
  ref_sphere       11.03 %   22.76 %   66.20 %    0.01 %   1.10e-03  4.41e-03
  ref_tiger        11.06 %   22.77 %   66.17 %    0.04 %   7.04e-02  2.82e-01
  ref_hypercube    11.08 %   22.72 %   66.20 %    0.04 %   2.96e-01  1.18e+00
  ang_0.3          11.08 %   23.00 %   65.92 %    0.03 %   5.40e-04  2.16e-03
  ang_1.0          11.23 %   30.91 %   57.86 %    0.01 %   6.91e-04  2.76e-03
  drct_0110        11.05 %   22.97 %   65.98 %    0.03 %   1.89e-03  7.55e-03
  drct_1234        11.06 %   22.96 %   65.98 %    0.03 %   1.46e-03  5.82e-03
  drct_3040        11.09 %   22.94 %   65.97 %    0.03 %   1.77e-03  7.07e-03
  len_2^-22        11.08 %   22.93 %   65.99 %    0.03 %   1.88e-03  7.51e-03
  len_2^22         11.10 %   22.96 %   65.94 %    0.03 %   1.87e-03  7.49e-03
  k_low_in         11.05 %   22.98 %   65.97 %    0.03 %   2.24e-03  8.98e-03
  k_high_in        11.02 %   23.06 %   65.93 %    0.03 %   3.37e-03  1.35e-02
  sharp_0          11.05 %   22.91 %   66.04 %    0.04 %   2.71e-03  1.08e-02
  sharp_0.7        11.06 %   22.95 %   65.99 %    0.02 %   3.04e-03  1.22e-02
  sharp_1.0        11.03 %   22.92 %   66.05 %    0.00 %   1.91e-06  7.63e-06
  sharp_1.5        11.06 %   23.01 %   65.93 %    0.53 %   2.96e-03  1.19e-02
(sun.light is about 10 to 20 here, 500 for ref_tiger and 2100 for ref_hypercube.)

b. Wherever the pre-test's predicate holds in fp32, the oracle returns sky_light's bits: rim, pre-test, guard and
half-space sets of every sun. c* comes from a sweep of the oracle's acos, sky_pre_k as build_aux computes it.
Mutating this file's copy of the predicate by hand: a sky_pre_k with (1 + 1e-5) fails on every sun whose sky_pre_k is
enabled (13 000 to 87 000 directions of the rim set, about 6 000 of the pre-test set, 100 to 650 of the guard set).
Dropping the guard on l2 fails nothing, down to directions of length 2^-75 and up to 2^63: each side of the comparison
is one rounding of an exact product and rounding is monotone, so the fp32 comparison still implies the exact one, and
v_cos is computed from the same a and l2. The guard is conservative, not load-bearing.

c. Specials (zero vector, NaN, inf, subnormals) and the constant mode.
"""
import numpy as np
import pytest

import final_light_cases as fc
import shader_f64 as sf

f32 = np.float32
BAND = 8 * 2.0 ** -24
MAX_AMBIGUOUS = 0.20
MIN_SIDE = 0.20
COND_LIMIT = 1000.0
MIN_ANG = 0.15  # 1 - cos(ang) above the largest eps of the generator (1e-2): no offset passes the sun's centre
F64_SUNS = [n for n in fc.SUN_NAMES if n not in fc.CONSTANT_MODE
            and (fc.SUNS[n] is None or MIN_ANG <= fc.SUNS[n][1] <= 1.0)]
SUN_SKY = [n for n in fc.SUN_NAMES if n not in fc.CONSTANT_MODE]


def _profile_slope(s, k):
    """dg/dk of g(k) = (s^2 k / (1 - s k) + 1) (1 - k)."""
    with np.errstate(all="ignore"):
        return (1 - k) * s * s / (1 - s * k) ** 2 - (s * s * k / (1 - s * k) + 1)


@pytest.mark.parametrize("name", F64_SUNS)
def test_oracle_matches_float64_reference(rt4, oracle, name):
    d = fc.scene(rt4, name).desc
    v = np.concatenate(list(fc.directions(d, name, ("rim", "pretest", "circle")).values()))
    assert np.isfinite(v).all() and (np.abs(v).max(axis=1) >= 2.0 ** -100).all()
    v64 = v.astype(np.float64)
    ref, in_sun = sf.final_light(d, v64, np.float64)
    ref32, _ = sf.final_light(d, v, np.float32)
    sun, ang, s = np.array(list(d.sun.drct), np.float64), np.float64(d.sun.angular_size), np.float64(d.sun.sharpness)
    cos = (v64 @ sun) / np.linalg.norm(v64, axis=1) / np.linalg.norm(sun)
    ambiguous = (np.abs(cos - np.cos(ang)) <= BAND) | (cos >= 1.0 - BAND)
    keep = ~ambiguous
    dev = np.arccos(np.minimum(cos, 1.0))
    with np.errstate(all="ignore"):
        ill = in_sun & ~(np.abs(_profile_slope(s, dev / ang)) / (ang * np.sin(dev)) <= COND_LIMIT)
    well = keep & ~ill
    with np.errstate(all="ignore"):
        e_ref = float(np.abs(ref32.astype(np.float64) - ref)[well].max())
    bound = min(4.0 * e_ref, 1e-3 * max(d.sun.light))
    print(f"  {name:14s} {100 * ambiguous.mean():7.2f} % {100 * (keep & in_sun).mean():7.2f} % "
          f"{100 * (keep & ~in_sun).mean():7.2f} % {100 * ill.mean():7.2f} %   {e_ref:.2e}  {bound:.2e}")
    assert ambiguous.mean() <= MAX_AMBIGUOUS
    assert (keep & in_sun).mean() >= MIN_SIDE and (keep & ~in_sun).mean() >= MIN_SIDE
    got = oracle.final_light(d, v)
    got_in = ~fc.is_sky(d, got)
    wrong = keep & (got_in != in_sun)
    assert not wrong.any(), (int(wrong.sum()), v[wrong][0], float(cos[wrong][0] - np.cos(ang)))
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(np.float64) - ref).max(axis=1)
    worst = np.where(well, err, 0.0)
    assert np.isfinite(err[well]).all() and worst.max() <= bound, (float(worst.max()), bound, v[np.argmax(worst)])


@pytest.mark.parametrize("name", SUN_SKY)
def test_pretest_implies_sky(rt4, oracle, name):
    d = fc.scene(rt4, name).desc
    ax = fc.aux(oracle, d)
    enabled = ax["pre_k"] > 0
    assert bool(enabled) == (name not in fc.PRE_K_DISABLED)
    assert bool(ax["pre_a"] == 0) == (name not in fc.NO_PRETEST)
    if name.startswith("k_"):  # sky_pre_k just inside an end of [2^-40, 2^40]
        end = 2.0 ** -40 if name == "k_low_in" else 2.0 ** 40
        assert abs(float(ax["pre_k"]) / end - 1.0) <= 2e-3
    sets = fc.directions(d, name, ("rim", "pretest", "guard", "halfspace"))
    for what, v in sets.items():
        fires = fc.pretest_fires(d, ax, v)
        sky = fc.is_sky(d, oracle.final_light(d, v))
        bad = fires & ~sky
        assert not bad.any(), (what, int(bad.sum()), v[bad][0])
        a, l2, aa = fc.pretest_terms(d, v)
        if what == "pretest" and enabled:
            with np.errstate(all="ignore"):
                rhs = (l2 * ax["pre_k"]).astype(f32).astype(np.float64)
                close = fires & (np.abs(aa.astype(np.float64) - rhs) <= 1e-4 * rhs)
            print(f"  {name}: pre-test fires on {fires.mean():.3f} of its set, within 1e-4 of the boundary {close.mean():.3f}")
            assert fires.mean() >= 0.20 and close.mean() >= 0.05
        if what == "guard":
            for lim in (fc.L2_LO, fc.L2_HI):  # both sides of both limits, within a factor 2^6 of them
                with np.errstate(all="ignore"):
                    below = (l2 < lim) & (l2 >= lim * f32(2.0 ** -6))
                    above = (l2 >= lim) & (l2 <= lim * f32(2.0 ** 6))
                assert below.sum() >= 1000 and above.sum() >= 1000, (float(lim), int(below.sum()), int(above.sum()))


@pytest.mark.parametrize("name", ["ref_sphere", "ang_1.0", "ang_pio2_up", "ang_3.2", "len_2^22", "sharp_1.5"])
def test_specials(rt4, oracle, name):
    """The zero vector and NaN directions: 0 / 0 and NaN reach acos, `deviation < ang` is false, the sky. The same for
    every direction whose cosine is NaN by inf - inf or inf / inf."""
    d = fc.scene(rt4, name).desc
    v = fc.specials(d, name)
    got = oracle.final_light(d, v)
    sky = fc.is_sky(d, got)
    assert sky[:5].all()  # zero, -zero, and the three NaN rows of specials()
    assert sky[np.isnan(v).any(axis=1)].all()
    with np.errstate(all="ignore"):
        ref, in_sun = sf.final_light(d, v.astype(np.float64), np.float64)
        nan_cos = np.isnan((v.astype(np.float64) @ np.array(list(d.sun.drct), np.float64)) / np.linalg.norm(v.astype(np.float64), axis=1))
    assert sky[nan_cos].all() and not in_sun[nan_cos].any()


@pytest.mark.parametrize("name", fc.CONSTANT_MODE)
def test_constant_mode(rt4, oracle, name):
    d = fc.scene(rt4, name).desc
    assert d.final_light_mode == rt4.FINAL_LIGHT_CONSTANT
    want = np.array(list(d.final_light_const), f32)
    if name == "constant":
        assert list(want) == [f32(x) for x in fc.CONSTANT_RGB]
    for what, v in fc.directions(d, name).items():
        got = oracle.final_light(d, v)
        assert (got.view(np.uint32) == want.view(np.uint32)[None]).all(), what


def test_reference_suns_cover_the_builtin_scenes(rt4):
    """Every distinct sun of the five builtin scenes is one of the ref_* cases."""
    have = {bytes(fc.scene(rt4, n).desc.sun) for n in fc.SUN_NAMES if n.startswith("ref_")}
    for n in rt4.BUILTIN_SCENES:
        assert bytes(rt4.Scene.builtin(n).desc.sun) in have, n
    assert len(set(fc.DIV_CANDIDATES)) == len(fc.DIV_CANDIDATES) >= 200
