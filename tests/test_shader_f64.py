"""The CPU oracle against shader_f64.py, the independent float64 restatement of executable/shader.frag (no GPU
needed): composites, normals, materials and whole pixels.

The GPU tests prove kernel == oracle bit for bit, and the oracle was written from the same reading of the shader as
the kernel. This file is the second reading. Rays: the hit flag, the winner, glow and refl_prob must be equal and the
distance and the normal within a bound, on every ray the reference does not itself call ambiguous. Pixels: the
per-pixel find_intersection counts must be equal (so the random path is the same: the order and number of rand()
calls, the seed carried over bounces and samples, the row orientation) and the colour within a bound, after one frame
and after a second one blended on top with another seed and part = 0.5.

Every bound is 4 * E_ref, where E_ref is the largest difference on the kept items between the reference run in
float32 and in float64 (shader_f64.py: the shader as written in plain numpy fp32, which is what a GL driver would do);
the factor 4 is the project's margin for other seeds and for rt4's own acos / asin / fma definitions.
Nothing of the oracle's or the kernel's output enters a bound. A bound coarser than 1e-3 (distances, normals) or one
8-bit step (colours) fails the test by itself. The caps on the ambiguous share (MAX_EXCLUDED of the rays, MAX_AMBIGUOUS
of the pixels: up to 8 find_intersection calls go into a pixel) and every "at least MIN_WINS" condition of the new
scenes are asserted from the reference's output alone.

Measured here (reference alone; E_ref as dist / normal for rays and as colour for pixels):

  rays                 excluded  ill-cond.  E_ref dist  E_ref normal
  union_2                 0.55 %    0.00 %   2.05e-05    2.21e-05
  hypercube_2             0.86 %    0.00 %   1.29e-06    0.00e+00
  tiger_2                 1.51 %    0.02 %   3.19e-05    3.76e-05
  tiger_5                 1.62 %    0.02 %   3.34e-05    3.71e-05
  all_1_3_1               1.84 %    1.64 %   7.03e-05    5.92e-05
  all_2_2_1               1.74 %    0.26 %   2.85e-05    7.66e-05
  all_2_3_2               1.82 %    0.32 %   3.35e-05    5.28e-05
  all_3_1_16              2.22 %    1.06 %   5.57e-05    6.21e-05
  unions_2                0.68 %    0.03 %   1.52e-05    4.51e-05
  hypercubes_2            1.69 %    0.00 %   1.25e-06    0.00e+00
  tigers_2                2.46 %    0.23 %   2.23e-05    6.88e-05
  tigers_4                2.80 %    0.45 %   3.81e-05    7.78e-05
  tiger_first             1.17 %    0.02 %   7.63e-05    6.27e-05
  union_radii             0.51 %    0.01 %   2.03e-05    4.70e-05
  hypercube_rotated       0.80 %    0.00 %   9.33e-06    0.00e+00
  hypercube_order         0.95 %    0.00 %   1.68e-06    0.00e+00
  tiger_faces             1.47 %    0.03 %   5.50e-05    5.38e-05
  sun_views               0.25 %    0.27 %   1.96e-05    5.21e-05
  spaces_1                0.35 %    0.00 %   1.62e-06    0.00e+00
  spaces_3                0.71 %    0.00 %   2.40e-05    0.00e+00
  spaces_32               3.30 %    0.00 %   1.00e-05    0.00e+00
  spheres_1_1             0.27 %    0.02 %   1.97e-05    4.84e-05
  spheres_1_3             0.40 %    1.74 %   3.80e-05    6.40e-05
  spheres_2_2             0.48 %    1.82 %   4.16e-05    4.93e-05
  spheres_9_2             1.63 %    0.75 %   3.31e-05    7.28e-05
  spheres_1_32            0.41 %    5.04 %   2.63e-05    6.56e-05
  spheres_2_0             0.51 %    0.00 %   4.44e-06    0.00e+00
  spaces_cylinders        0.43 %    0.39 %   2.41e-05    5.28e-05
  spheres_only            0.56 %    0.10 %   6.17e-05    4.92e-05
  outer_0                 0.51 %    0.42 %   2.18e-05    5.83e-05
  new_first_0             0.63 %    4.74 %   3.56e-05    4.86e-05
  sub_range               0.51 %    0.84 %   3.84e-05    6.76e-05
  kind_twice              0.46 %    1.62 %   4.27e-05    7.48e-05
  sphere_untested_tiger   0.26 %    0.06 %   3.16e-05    3.19e-05
  snippet                 0.47 %    0.70 %   2.35e-05    4.68e-05

  pixels (36x20, 2 spp, 3 bounces, two frames)   ambiguous  E_ref colour
  sphere                  0.97 %   3.15e-05
  room                    8.61 %   2.75e-08
  tiger                   0.83 %   2.88e-05
  cylinder4d              0.42 %   2.88e-05
  hypercube               9.58 %   1.71e-05
  union_2                 0.28 %   9.49e-06
  hypercube_2             2.92 %   5.06e-06
  tiger_2                 0.97 %   4.08e-06
  all_2_2_1               5.56 %   7.85e-07
  outer_0                 1.11 %   1.08e-05
  union_radii             2.78 %   8.34e-06
  hypercube_rotated       4.17 %   4.65e-06
  hypercube_order         3.89 %   1.68e-06
  tiger_faces             0.69 %   1.44e-05
  sun_views               0.14 %   2.80e-05
  sun_views_sharp         0.14 %   4.10e-05
  sun_views_constant      0.14 %   6.13e-08

test_gpu_shader_f64.py runs the kernels against the same references.
"""
import ctypes

import numpy as np
import pytest

import scene_builder as sb
import shader_f64 as sf
from test_scene_shapes import MAX_EXCLUDED, MIN_WINS

MAX_AMBIGUOUS = 0.25  # of a case's pixels
DIST_CAP = NORMAL_CAP = 1e-3  # the coarsest bound a ray case may have
COLOR_CAP = 1.0 / 255.0  # the coarsest bound a pixel case may have: one 8-bit display step
WIDTH, HEIGHT, SPP, BOUNCES = 36, 20, 2, 3  # partial 8x8 tiles in both directions
FRAMES = ((31, 1.0), (77, 0.5))  # (seed, part): the second frame is blended onto the first


# ---------------------------------------------------------------------------------------- new scenes
def _material(m, glow, refl_prob):
    m.glow, m.refl_prob = float(np.float32(glow)), float(np.float32(refl_prob))


def _extra_rays(rng, origins, n):
    v = rng.normal(size=(n, 4))
    return np.concatenate([origins, v / np.linalg.norm(v, axis=1, keepdims=True)], axis=1).astype(np.float32)


def union_radii(rt4):
    """One union whose cylinders differ in radius: both band checks compare with cylinder2.r (shader.frag:286,290),
    so a hit of cylinder2 between 0.5 and 0.9 from cylinder1's axes plane counts. refl_prob 0.5 and 1, a glowing part."""
    d = sb.compose(rt4, spaces=2, unions=1, seed=301)
    u = d.unions[0]
    u.cylinder1.r, u.cylinder2.r = 0.5, float(np.float32(0.9))
    _material(u.cylinder1.material, 1.5, 0.5)
    _material(u.cylinder2.material, 0.0, 1.0)
    return dict(desc=d, rays=sb.case_rays(d, 9301))


def _init_hypercube(hc, point, q, r):
    """init_hypercube (shader.frag:374-392) on the frame q (columns x, y, z, w), point +- axis * r formed in fp32."""
    point, q, r = np.asarray(point, np.float32), np.asarray(q, np.float32), np.float32(r)
    for sgn in range(2):
        for a in range(4):
            cube = hc.cubes[sgn * 4 + a]
            axis = q[:, a] if sgn == 0 else -q[:, a]
            sb._set(cube.point, point + q[:, a] * r if sgn == 0 else point - q[:, a] * r)
            sb._set(cube.norm, axis)
            others = [k for k in range(4) if k != a]
            sb._set(cube.x, q[:, others[0]])
            sb._set(cube.y, q[:, others[1]])
            sb._set(cube.z, q[:, others[2]])
            cube.r = float(r)


def hypercube_rotated(rt4):
    """A hypercube on a frame rotated by about 0.4 rad (the composed ones are axis-aligned), and rays that start
    inside it: a cell is invisible from behind (h < 0, shader.frag:356), so they pass through every wall."""
    d = sb.compose(rt4, spaces=2, hypercubes=1, seed=302)
    rng = np.random.default_rng(302)
    q = sb._frame(rng, 0.4)
    cubes = d.hypercubes[0].cubes
    centre, r = np.mean([list(c.point) for c in cubes], axis=0), cubes[0].r
    _init_hypercube(d.hypercubes[0], centre, q, r)
    _material(cubes[2].material, 2.0, 1.0)
    inside = centre + rng.uniform(-0.9, 0.9, (800, 4)) @ q.T * r
    return dict(desc=d, rays=np.concatenate([sb.case_rays(d, 9302), _extra_rays(rng, inside, 800)]))


def hypercube_order(rt4):
    """Eight cells that are no init_hypercube: cubes[1] is the cell facing the camera and cubes[0] a parallel copy
    0.5 behind it. hypercube_intersection returns the first cell in array order that hits (shader.frag:394-400),
    so a ray through both ends on the far one."""
    d = sb.compose(rt4, spaces=2, hypercubes=1, seed=303)
    cubes = d.hypercubes[0].cubes
    front = cubes[5]  # init_hypercube's -y cell
    for k, back in ((1, 0.0), (0, 0.5)):
        point = np.array(list(front.point), np.float32) + np.array([0, back, 0, 0], np.float32)
        sb._set(cubes[k].point, point)
        for name in ("norm", "x", "y", "z"):
            sb._set(getattr(cubes[k], name), list(getattr(front, name)))
        cubes[k].r = front.r
    return dict(desc=d, rays=sb.case_rays(d, 9303))


def tiger_faces(rt4):
    """One tiger, with origins in the hole, inside the wall and outside: each of the eight face tests of
    shader.frag:328-335 (a cylinder from outside or from inside, banded by the other pair) has to win rays."""
    d = sb.compose(rt4, spaces=2, tigers=1, seed=304)
    t = d.tigers[0]
    _material(t.inner_cyl1.material, 0.0, 1.0)
    _material(t.outer_cyl2.material, 3.0, 0.5)
    rng = np.random.default_rng(304)
    centre = np.array(list(t.inner_cyl1.point), np.float64)
    hole = centre + rng.uniform(-0.5, 0.5, (1500, 4)) * t.inner_cyl1.r
    wall = sb._targets(d, 6, 0, 1500, rng) + rng.normal(0, 0.03, (1500, 4))
    return dict(desc=d, rays=np.concatenate([sb.case_rays(d, 9304), _extra_rays(rng, hole, 1500),
                                             _extra_rays(rng, wall, 1500)]))


def _sun_views(rt4, sharpness, constant=False):
    """A camera pitched up 45 degrees, straight at the sun (0, 1, 1, 0): the disc (0.09 pi across) fills the middle
    of the image, between two spheres in its lower corners."""
    d = sb.compose(rt4, spaces=1, spheres=2, seed=305)
    sb._set(d.sun.drct, (0.0, 1.0, 1.0, 0.0))  # not a unit vector: v_cos normalises (shader.frag:45-47)
    d.sun.sharpness = float(np.float32(sharpness))
    for s, centre, r in ((d.spheres[0], (-0.8, 0.4, 1.1, 0.0), 0.6), (d.spheres[1], (0.9, 0.6, 1.0, 0.0), 0.5)):
        sb._set(s.center, centre)
        s.r = float(np.float32(r))
    _material(d.spheres[0].material, 0.0, 0.5)
    if constant:
        d.final_light_mode = rt4.FINAL_LIGHT_CONSTANT
        sb._set(d.final_light_const, (0.3, 0.2, 0.1))
    return dict(desc=d, rays=sb.case_rays(d, 9305), camera=dict(te=45.0))


NEW_SCENES = {
    "union_radii": union_radii,
    "hypercube_rotated": hypercube_rotated,
    "hypercube_order": hypercube_order,
    "tiger_faces": tiger_faces,
    "sun_views": lambda rt4: _sun_views(rt4, 0.0),
    "sun_views_sharp": lambda rt4: _sun_views(rt4, 0.7),
    "sun_views_constant": lambda rt4: _sun_views(rt4, 0.7, constant=True),
}
COMPOSITE_CASES = [n for n in sb.CASES if n not in sb.SIMPLE_CASES and not n.startswith("tie_")]
RAY_CASES = COMPOSITE_CASES + ["union_radii", "hypercube_rotated", "hypercube_order", "tiger_faces", "sun_views"]
PIXEL_CASES = (["sphere", "room", "tiger", "cylinder4d", "hypercube", "union_2", "hypercube_2", "tiger_2", "all_2_2_1",
                "outer_0"] + list(NEW_SCENES))

_cases = {}


def case_of(rt4, name):
    """dict(desc, rays (None for a builtin scene), camera: make_uniforms keywords) of a case, built once."""
    if name not in _cases:
        if name in NEW_SCENES:
            c = NEW_SCENES[name](rt4)
        elif name in rt4.BUILTIN_SCENES:
            c = dict(desc=rt4.Scene.builtin(name).desc, rays=None)
        else:
            d, rays = sb.case_scene_and_rays(rt4, name)
            c = dict(desc=d, rays=rays, camera=dict(focus=sb.case_focus(name)))
        c.setdefault("camera", {})
        _cases[name] = c
    return _cases[name]


def frame_uniforms(rt4, name):
    """The uniforms of the case's two frames."""
    return [rt4.make_uniforms(WIDTH, HEIGHT, samples=SPP, reflections=BOUNCES, seed=seed, part=part,
                              **case_of(rt4, name)["camera"]) for seed, part in FRAMES]


# --------------------------------------------------------------------------- references, once per case
_ray_refs, _pixel_refs = {}, {}


def _agree(a, b):
    """Two reference runs name the same hit."""
    return (a["hit"] == b["hit"]) & (a["surface"] == b["surface"])


def ray_reference(rt4, name):
    """The float64 reference of the case's rays, its keep masks and the case's bounds, from the reference alone."""
    if name not in _ray_refs:
        c = case_of(rt4, name)
        r64, r32 = sf.ref_find_rays(c["desc"], c["rays"]), sf.ref_find_rays(c["desc"], c["rays"], np.float32)
        keep = ~r64["ambiguous"]
        ill = sf.ill_conditioned(r64["cond"])
        hits = keep & r64["hit"]
        split = int((keep & ~_agree(r64, r32)).sum())  # the reference's own fp32 run takes another branch
        e_dist = np.abs(r32["dist"] - r64["dist"]) / np.maximum(1.0, r64["dist"])
        e_norm = np.abs(r32["norm"] - r64["norm"]).max(axis=1)
        _ray_refs[name] = dict(
            r64=r64, keep=keep, ill=ill, hits=hits, split=split, excluded=float((~keep).mean()),
            ill_share=float((keep & ill & r64["hit"]).mean()),
            e_dist=float(e_dist[hits & _agree(r64, r32)].max(initial=0.0)),
            e_norm=float(e_norm[hits & ~ill & _agree(r64, r32)].max(initial=0.0)))
    return _ray_refs[name]


def pixel_reference(rt4, name):
    """Both frames of the case in float64, the kept pixels after each, and the bounds, from the reference alone."""
    if name not in _pixel_refs:
        d, reg = case_of(rt4, name)["desc"], rt4.region(WIDTH, HEIGHT)
        frames, old64, old32, amb, e_color = [], None, None, np.zeros((HEIGHT, WIDTH), bool), 0.0
        split = 0
        for u in frame_uniforms(rt4, name):
            f64, f32 = sf.ref_pixels(d, u, reg, old64), sf.ref_pixels(d, u, reg, old32, np.float32)
            amb = amb | f64["ambiguous"]
            split += int((~amb & (f64["counts"] != f32["counts"])).sum())
            e_color = max(e_color, float(np.abs(f32["rgba"] - f64["rgba"])[~amb].max(initial=0.0)))
            frames.append(dict(f64, keep=~amb))
            old64, old32 = f64["rgba"], f32["rgba"]
        p64, p32 = frames[0], f32  # the primary hit does not depend on the seed
        keep = ~p64["primary_ambiguous"] & p64["hit"] & _agree(p64, p32)
        with np.errstate(invalid="ignore"):  # inf - inf where both runs miss
            depth_diff = np.abs(p32["depth"] - p64["depth"]) / np.maximum(1.0, p64["depth"])
        _pixel_refs[name] = dict(
            frames=frames, ambiguous=float(amb.mean()), e_color=e_color, split=split,
            e_depth=float(depth_diff[keep].max(initial=0.0)),
            e_normal=float(np.abs(p32["normal"] - p64["normal"]).max(axis=2)[
                keep & ~sf.ill_conditioned(p64["primary_cond"])].max(initial=0.0)))
    return _pixel_refs[name]


# ------------------------------------------------------------------------------------------- checks
def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def check_ray_reference(name, ref):
    """The conditions on the reference itself: caps and bounds that are fine enough to catch a misreading."""
    print(f"{name}: excluded {ref['excluded']:.4f} ill-conditioned {ref['ill_share']:.4f} kept hits "
          f"{int(ref['hits'].sum())} E_ref dist {ref['e_dist']:.2e} normal {ref['e_norm']:.2e}")
    assert ref["split"] == 0, f"{name}: the reference's fp32 run differs from its float64 run on {ref['split']} kept rays"
    assert ref["excluded"] + ref["ill_share"] <= MAX_EXCLUDED
    assert ref["hits"].sum() > 2000
    assert 4 * ref["e_dist"] <= DIST_CAP and 4 * ref["e_norm"] <= NORMAL_CAP


def check_rays(name, ref, out, col, who):
    """find_intersection rows (rt4.h rt4_debug_find_intersection's layout) of `who` against the reference."""
    r64, keep = ref["r64"], ref["keep"]
    hit = out[:, 0] > 0
    bad = np.flatnonzero(keep & (hit != r64["hit"]))
    assert len(bad) == 0, f"{name} {who}: hit flag differs on {len(bad)} kept rays, first {bad[:3]}"
    both = keep & hit
    bad = np.flatnonzero(both & (bits(col) != bits(r64["color"])).any(axis=1))
    assert len(bad) == 0, f"{name} {who}: winner differs on {len(bad)} kept rays, first {bad[:3]}"
    assert np.array_equal(bits(out[both, 6]), bits(r64["glow"][both])), f"{name} {who}: glow"
    assert np.array_equal(bits(out[both, 7]), bits(r64["refl_prob"][both])), f"{name} {who}: refl_prob"
    e_dist = (np.abs(out[:, 1].astype(np.float64) - r64["dist"]) / np.maximum(1.0, r64["dist"]))[both].max(initial=0.0)
    e_norm = np.abs(out[:, 2:6].astype(np.float64) - r64["norm"]).max(axis=1)[both & ~ref["ill"]].max(initial=0.0)
    print(f"{name} {who}: dist error {e_dist:.2e} (bound {4 * ref['e_dist']:.2e}) normal error {e_norm:.2e} "
          f"(bound {4 * ref['e_norm']:.2e})")
    assert e_dist <= 4 * ref["e_dist"], f"{name} {who}: distance"
    assert e_norm <= 4 * ref["e_norm"], f"{name} {who}: normal"


def check_pixel_reference(name, ref):
    print(f"{name}: ambiguous {ref['ambiguous']:.4f} E_ref colour {ref['e_color']:.2e} primary depth "
          f"{ref['e_depth']:.2e} normal {ref['e_normal']:.2e}")
    assert ref["split"] == 0, f"{name}: the reference's fp32 run takes another path on {ref['split']} kept pixels"
    assert ref["ambiguous"] <= MAX_AMBIGUOUS
    assert 4 * ref["e_color"] <= COLOR_CAP
    assert 4 * ref["e_depth"] <= DIST_CAP and 4 * ref["e_normal"] <= NORMAL_CAP


def check_frame(name, ref, k, rgba, who, counts=None, total=None):
    """Frame k (0 or 1) of `who` against the reference: alpha, colour on the kept pixels, and the find_intersection
    counts: per pixel where `who` reports them, else the total (every path of a pixel that is not kept makes
    between one call and BOUNCES + 1)."""
    f = ref["frames"][k]
    keep = f["keep"]
    assert (rgba[..., 3] == 1.0).all(), f"{name} {who} frame {k}: alpha"
    if counts is not None:
        bad = np.argwhere(keep & (counts != f["counts"]))
        assert len(bad) == 0, f"{name} {who} frame {k}: find_intersection count differs on {len(bad)} kept pixels, first {bad[:3].tolist()}"
    if total is not None:
        rest = total - int(f["counts"][keep].sum())
        assert SPP * int((~keep).sum()) <= rest <= SPP * (BOUNCES + 1) * int((~keep).sum()), f"{name} {who} frame {k}: count"
    err = np.abs(rgba[..., :3].astype(np.float64) - f["rgba"][..., :3]).max(axis=2)[keep].max(initial=0.0)
    print(f"{name} {who} frame {k}: colour error {err:.2e} (bound {4 * ref['e_color']:.2e})")
    assert err <= 4 * ref["e_color"], f"{name} {who} frame {k}: colour"


# -------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(NEW_SCENES))
def test_new_scene_is_valid(rt4, name):
    d = case_of(rt4, name)["desc"]
    err = ctypes.create_string_buffer(256)
    assert rt4.lib.rt4_scene_validate(ctypes.byref(d), err, len(err)) == 0, err.value
    cols = [c for _, _, cs in sb.objects(d) for c in cs]
    assert len(set(cols)) == len(cols)


def test_materials_cover_the_outcomes(rt4):
    """refl_prob 0, 0.5 and 1 (rand_outcome never, sometimes, always: rand() is below 1) and a glowing part of a
    composite, among the surfaces that win kept rays of the new scenes."""
    refl, glowing_part = set(), False
    for name in ("union_radii", "hypercube_rotated", "tiger_faces"):
        ref, d = ray_reference(rt4, name), case_of(rt4, name)["desc"]
        r64, first_part = ref["r64"], sf.surface_bases(d)[4]
        for s in np.unique(r64["surface"][ref["hits"]]):
            won = ref["hits"] & (r64["surface"] == s)
            if won.sum() >= MIN_WINS:
                refl.add(float(r64["refl_prob"][won][0]))
                glowing_part |= bool(s >= first_part and r64["glow"][won][0] > 0)
    assert {0.0, 0.5, 1.0} <= refl and glowing_part


def test_union_radii_rays_tell_the_radii_apart(rt4):
    """At least MIN_WINS kept rays whose result differs if the second band check compares with cylinder1.r."""
    c, ref = case_of(rt4, "union_radii"), ray_reference(rt4, "union_radii")
    other = sf.ref_find_rays(c["desc"], c["rays"], union_check2_r1=True)
    differs = ref["keep"] & ~other["ambiguous"] & ~_agree(ref["r64"], other)
    assert differs.sum() >= MIN_WINS, int(differs.sum())


def test_hypercube_order_rays_end_on_the_far_cell(rt4):
    """At least MIN_WINS kept rays whose winner is a cell that is not the nearest hitting one."""
    ref = ray_reference(rt4, "hypercube_order")
    far = ref["hits"] & ref["r64"]["not_nearest"] & (ref["r64"]["part"] == 0)
    assert far.sum() >= MIN_WINS, int(far.sum())


def test_rays_from_inside_the_hypercube_miss_it(rt4):
    ref, d = ray_reference(rt4, "hypercube_rotated"), case_of(rt4, "hypercube_rotated")["desc"]
    inside = ref["keep"] & ref["r64"]["inside_cube"]
    assert inside.sum() >= MIN_WINS, int(inside.sum())
    first = sf.surface_bases(d)[5]
    assert not ((ref["r64"]["surface"][inside] >= first) & (ref["r64"]["surface"][inside] < first + 8)).any()


def test_every_tiger_face_test_wins_rays(rt4):
    ref, d = ray_reference(rt4, "tiger_faces"), case_of(rt4, "tiger_faces")["desc"]
    on_tiger = ref["hits"] & (ref["r64"]["surface"] >= sf.surface_bases(d)[6])
    wins = np.bincount(ref["r64"]["part"][on_tiger], minlength=8)
    assert (wins >= MIN_WINS).all(), wins.tolist()


def test_sun_views_look_at_the_sun(rt4):
    for name in ("sun_views", "sun_views_sharp"):
        f = pixel_reference(rt4, name)["frames"][0]
        assert (f["in_sun"] & f["keep"]).sum() >= MIN_WINS, name
    assert case_of(rt4, "sun_views_constant")["desc"].final_light_mode == rt4.FINAL_LIGHT_CONSTANT


def test_both_sphere_formulations_agree_in_float64(rt4):
    """The closed form the float64 reference uses and the shader's acos / asin chain (what its float32 run uses) are
    the same function: in float64 they differ by rounding only (the chain's PI is the fp32 constant: 8.7e-8)."""
    for name in ("all_2_2_1", "outer_0", "tiger_faces"):
        c = case_of(rt4, name)
        rays = np.asarray(c["rays"], np.float64)
        dn = rays[:, 4:] / np.linalg.norm(rays[:, 4:], axis=1, keepdims=True)
        closed = sf.find(c["desc"], rays[:, :4], dn)
        written = sf.find(c["desc"], rays[:, :4], dn, as_written=True)
        keep = ~closed["ambiguous"] & closed["hit"]
        assert np.array_equal(closed["hit"][~closed["ambiguous"]], written["hit"][~closed["ambiguous"]])
        assert np.array_equal(closed["surface"][keep], written["surface"][keep])
        assert (np.abs(closed["dist"] - written["dist"])[keep] <= 2e-6 * np.maximum(1, closed["dist"][keep])).all()


@pytest.mark.parametrize("name", RAY_CASES)
def test_oracle_rays_against_reference(rt4, oracle, name):
    ref = ray_reference(rt4, name)
    check_ray_reference(name, ref)
    c = case_of(rt4, name)
    out, col = oracle.find_intersection(c["desc"], c["rays"])
    check_rays(name, ref, out, col, "oracle")


@pytest.mark.parametrize("name", sb.SIMPLE_CASES)
def test_oracle_normals_and_materials_of_simple_cases(rt4, oracle, name):
    """What test_scene_shapes.test_oracle_against_float64_reference leaves out for the scenes of spaces, spheres and
    cylinders: the normal (the sign flip of shader.frag:219 and -drct_h of :238 included), glow and refl_prob."""
    ref = ray_reference(rt4, name)
    check_ray_reference(name, ref)
    c = case_of(rt4, name)
    out, col = oracle.find_intersection(c["desc"], c["rays"])
    check_rays(name, ref, out, col, "oracle")


@pytest.mark.parametrize("name", PIXEL_CASES)
def test_oracle_pixels_against_reference(rt4, oracle, name):
    ref = pixel_reference(rt4, name)
    check_pixel_reference(name, ref)
    d, reg = case_of(rt4, name)["desc"], rt4.region(WIDTH, HEIGHT)
    frame = np.zeros((HEIGHT, WIDTH, 4), np.float32)
    for k, u in enumerate(frame_uniforms(rt4, name)):
        _, total, _, counts = oracle.render(d, u, reg, frame=frame, threads=4, pixel_counts=True)
        check_frame(name, ref, k, frame, "oracle", counts=counts, total=total)
