"""The CPU oracle's find_intersection against the float64 reference of shader_f64.py (written from the geometry;
it lived here before it grew composites, normals and whole pixels: test_shader_f64.py), on the composed scenes of
scene_builder.py (no GPU needed).

The GPU tests prove kernel == oracle bit for bit; test_oracle.py checks single objects on hand-picked rays. This
file checks what lies between: that the oracle's group list (first, count, outer, the order of closest's
arguments) and its acos / asin formulation of the sphere test give the hit, the winner and the distance that the
plain quadratic gives. It also asserts, from the oracle alone, the conditions that give the GPU tests of
test_gpu_scene_shapes.py their teeth: every tested object wins rays, the images have hits and sky tiles.

A ray is compared unless the reference itself calls it ambiguous (shader_f64.find); at most MAX_EXCLUDED of
a scene's rays may be.
"""
import ctypes

import numpy as np
import pytest

import scene_builder as sb
# the float64 reference (moved to shader_f64.py, where it also covers composites, normals and whole pixels)
from shader_f64 import MARGIN, SMALL_FLOAT, _cylinder, _quadratic, _space, _sphere, ref_find_intersection  # noqa: F401

# Share of a scene's rays the reference may call ambiguous. Measured with MARGIN = 1e-3 (about 20000 rays each):
#   spaces_1 0.35 %   spaces_3 0.71 %   spaces_32 3.30 %   spheres_1_1 0.27 %   spheres_1_3 0.40 %
#   spheres_2_2 0.48 %   spheres_9_2 1.63 %   spheres_1_32 0.41 %   spheres_2_0 0.51 %
#   sphere_untested_tiger 0.26 %   spaces_cylinders 0.43 %   spheres_only 0.56 %   outer_0 0.51 %
#   new_first_0 0.63 %   sub_range 0.51 %   kind_twice 0.46 %   snippet 0.47 %
# (many spaces: their near-parallel floors cross, so two candidates are often within the margin). Two rules of the
# reference are finer than when it lived here, hence shares below the 0.37 % .. 5.57 % first measured: a robust miss
# of a space (a cosine more than shader_f64.MISS_MARGIN below SMALL_FLOAT) is not ambiguous, and an origin well
# within SMALL_FLOAT of a sphere's centre or a cylinder's axes plane takes the closed form of the shader's own branch
# (snippet: 1000 of its background rays start at the default camera, which lies on its tube's axes plane; it had
# 5.57 %).
# On the kept rays the hit flag and the winner agreed on every ray of every case.
MAX_EXCLUDED = 0.10
MIN_WINS = 20
SPP, BOUNCES, WIDTH, HEIGHT = 3, 4, 64, 40  # the renders of test_gpu_scene_shapes.py

# Largest |d_oracle - d_f64| / max(1, d_f64) over the kept rays of all SIMPLE_CASES: measured 6.27e-5
# (new_first_0; per case between 1.0e-6 for one space and 6.3e-5; the fp32 acos / asin chain of the sphere test
# loses precision towards grazing). The bound is four times the measured value, for other seeds.
MEASURED_DIST_ERROR = 6.27e-5
DIST_BOUND = 4 * MEASURED_DIST_ERROR


# ------------------------------------------------------------------------------------------ fixtures
_scenes = {}


def scene_of(rt4, name):
    if name not in _scenes:
        _scenes[name] = sb.case_scene_and_rays(rt4, name)
    return _scenes[name]


def is_simple(d):
    return all(g.kind <= 3 for g in d.groups[: d.n_groups])


# --------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name", list(sb.CASES))
def test_case_is_valid_and_colours_are_unique(rt4, name):
    d, _ = scene_of(rt4, name)
    err = ctypes.create_string_buffer(256)
    assert rt4.lib.rt4_scene_validate(ctypes.byref(d), err, len(err)) == 0, err.value
    cols = [c for _, _, cs in sb.objects(d) for c in cs]
    assert len(set(cols)) == len(cols)
    mats = ([d.spaces[i].material for i in range(d.n_spaces)] + [d.spheres[i].material for i in range(d.n_spheres)])
    assert any(m.glow > 0 for m in mats)


@pytest.mark.parametrize("name", list(sb.CASES))
def test_every_tested_object_wins_rays(rt4, oracle, name):
    """Every object of every tested group, and every cell or face of a composite, wins at least MIN_WINS of the
    case's rays (by colour)."""
    d, rays = scene_of(rt4, name)
    out, col = oracle.find_intersection(d, rays)
    won = sb.wins_per_material(d, out[:, 0], col)
    tested = sb.tested_objects(d)
    if name.startswith("tie_"):  # the coincident spheres: exactly one of the two wins (test_tie_rule)
        tested = {(2, 0 if name == "tie_new_first_1" else 1)}
    few = {(sb.KIND_NAMES[k], i, j): n for (k, i, j), n in won.items() if (k, i) in tested and n < MIN_WINS}
    assert not few, f"{name}: materials that win fewer than {MIN_WINS} of {len(rays)} rays: {few}"


@pytest.mark.parametrize("name", list(sb.CASES))
def test_render_has_hits_and_sky_tiles(rt4, oracle, name):
    """The oracle's 64x40 image of the case: primary hits (more than one find_intersection per sample) on at
    least a quarter of the pixels, and at least one 8x8 tile whose centre ray reaches the sky: the tile-order
    pre-pass (rt4_tile_order_kernel) only reorders when such tiles exist."""
    d, _ = scene_of(rt4, name)
    u = sb.case_uniforms(rt4, name, WIDTH, HEIGHT, SPP, BOUNCES, seed=31)
    _, _, _, counts = oracle.render(d, u, rt4.region(WIDTH, HEIGHT), pixel_counts=True)
    assert (counts > SPP).mean() >= 0.25, f"{name}: primary hits on {(counts > SPP).mean():.2%} of the pixels"
    centres = counts[4::8, 4::8]
    assert (centres == SPP).any() and (centres > SPP).any(), f"{name}: sky tiles {(centres == SPP).sum()} of {centres.size}"


def compare(rt4, oracle, name):
    d, rays = scene_of(rt4, name)
    out, col = oracle.find_intersection(d, rays)
    hit, rcol, dist, amb = ref_find_intersection(d, rays)
    keep = ~amb
    o_hit = out[:, 0] > 0
    bad_hit = keep & (o_hit != hit)
    bad_win = keep & o_hit & hit & (col != rcol).any(axis=1)
    both = keep & o_hit & hit & ~bad_win
    err = np.abs(out[:, 1].astype(np.float64) - dist) / np.maximum(1.0, dist)
    return dict(excluded=float(amb.mean()), bad_hit=np.flatnonzero(bad_hit), bad_win=np.flatnonzero(bad_win),
                max_err=float(err[both].max()) if both.any() else 0.0, kept_hits=int(both.sum()), rays=rays)


@pytest.mark.parametrize("name", sb.SIMPLE_CASES)
def test_oracle_against_float64_reference(rt4, oracle, name):
    d, _ = scene_of(rt4, name)
    assert is_simple(d)
    r = compare(rt4, oracle, name)
    print(f"{name}: excluded {r['excluded']:.4f} kept hits {r['kept_hits']} max rel dist err {r['max_err']:.3e} "
          f"hit flag differs on {len(r['bad_hit'])} winner differs on {len(r['bad_win'])}")
    assert r["excluded"] <= MAX_EXCLUDED
    assert r["kept_hits"] > 2000
    assert len(r["bad_hit"]) == 0, (name, r["rays"][r["bad_hit"][:3]])
    assert len(r["bad_win"]) == 0, (name, r["rays"][r["bad_win"][:3]])
    assert r["max_err"] <= DIST_BOUND


def test_tie_rule(rt4, oracle):
    """Two coincident spheres: closest(new, inter) keeps the accumulated hit (sphere 0), closest(inter, new) takes
    the new one (sphere 1): rt4.h rt4_group.new_first. Everything else of the hit is the same."""
    res = {}
    for nf in (1, 0):
        d, rays = scene_of(rt4, f"tie_new_first_{nf}")
        out, col = oracle.find_intersection(d, rays)
        hits = out[:, 0] > 0
        assert hits.sum() > 2000
        keeper = d.spheres[0 if nf else 1].material
        assert (col[hits] == np.array(keeper.color[:3], np.float32)).all()
        assert (out[hits, 6] == np.float32(keeper.glow)).all() and (out[hits, 7] == np.float32(keeper.refl_prob)).all()
        res[nf] = (rays, out, col)
    assert np.array_equal(res[0][0], res[1][0])
    assert np.array_equal(res[0][1][:, :6].view(np.uint32), res[1][1][:, :6].view(np.uint32))
    assert (res[0][2] != res[1][2]).any()
