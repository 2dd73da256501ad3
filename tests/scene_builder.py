"""Composed scenes for the scene-shape tests (test_scene_shapes.py, test_gpu_scene_shapes.py): a plain helper,
not a fixture.

The seven named scenes each run on a kernel compiled for their exact object counts. A user's scene has other
counts and other group lists, so it runs on one of the six runtime-count kernels (rt4_trace.hip kVariants) or on
the generic find_intersection. compose() builds such scenes from counts, an explicit group list and a seed:

  * every object, and every cell / face of a composite, has its own material colour, so the colour output of
    find_intersection names the winning object; refl_prob and glow vary, material 0 always glows;
  * everything lies in view of the default make_uniforms camera (focus (0, -2, 0, 0), looking along +y, x to the
    right, z up, w = 0): spheres and composites in the frustum at depths 1..5, cylinders as tubes that run away
    from the camera below eye level, spaces as a ground, one side wall and further tilted floors under the ground,
    so that the rays of the image's upper part reach the sky (the tile-order pre-pass needs sky tiles to reorder);
  * tigers have one point and one axes pair per cylinder pair (init_tiger) and hypercubes the cells of
    init_hypercube, so scene_shape() takes them for the specialised kernels; unions have orthonormal axes.

aimed_rays() sends rays at every object: uniform random rays let a small sphere among 32 win a handful of 20000
rays or none, and an object that never wins is not tested.
"""
import numpy as np

FOCUS = np.array([0.0, -2.0, 0.0, 0.0])  # rt4.make_uniforms default camera
KIND_NAMES = {1: "space", 2: "sphere", 3: "cylinder", 4: "union", 5: "hypercube", 6: "tiger"}


def _set(arr, v):
    for i, x in enumerate(v):
        arr[i] = float(np.float32(x))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _frame(rng, angle):
    """An orthonormal basis (columns) within about `angle` radians of the standard one."""
    a = rng.normal(size=(4, 4))
    a = (a - a.T) / 2.0
    a *= angle / np.linalg.norm(a, 2)
    q, r = np.linalg.qr(np.eye(4) + a)
    return q * np.sign(np.diag(r))


def set_material(m, k):
    """Material number k of a scene: a colour no other number has (k < 512), varied refl_prob and glow."""
    m.color[0] = float(np.float32((k % 8 + 2) / 10.0))
    m.color[1] = float(np.float32((k // 8 % 8 + 2) / 10.0))
    m.color[2] = float(np.float32((k // 64 + 2) / 10.0))
    m.refl_prob = float(np.float32((0.0, 0.3, 0.7, 0.15)[k % 4]))
    m.glow = float(np.float32((1.5, 0.5, 4.0)[k // 3 % 3])) if k % 3 == 0 else 0.0


def _cylinder(c, point, a1, a2, r):
    _set(c.point, point)
    _set(c.axis1, a1)
    _set(c.axis2, a2)
    c.r = float(np.float32(r))


def canonical_groups(rt4, spaces, spheres, cylinders, unions, hypercubes, tigers):
    """shader.frag's form: one statement per kind, in kind order, outer = true, closest(new, inter)."""
    g = []
    for kind, n, outer in ((rt4.GROUP_SPACES, spaces, 0), (rt4.GROUP_SPHERES, spheres, 1),
                           (rt4.GROUP_CYLINDERS, cylinders, 1), (rt4.GROUP_CYLINDERS_UNION, unions, 1),
                           (rt4.GROUP_HYPERCUBE, hypercubes, 0), (rt4.GROUP_TIGER, tigers, 0)):
        if n:
            g.append((kind, 0, n, outer, 1))
    return g


def set_groups(d, groups):
    d.n_groups = len(groups)
    for i, (kind, first, count, outer, new_first) in enumerate(groups):
        g = d.groups[i]
        g.kind, g.first, g.count, g.outer, g.new_first = kind, first, count, outer, new_first


def add_spaces(d, n, rng, next_material):
    """Spaces d.n_spaces .. d.n_spaces + n - 1: the ground, a wall on the left, then tilted floors below the
    ground. The camera is above all the floors, so rays that point up enough miss every one of them."""
    for _ in range(n):
        i = d.n_spaces
        s = d.spaces[i]
        if i == 0:
            point, norm = (0.0, 0.0, -1.5, 0.0), _unit(np.array([0, 0, 1.0, 0]) + rng.normal(0, 0.02, 4))
        elif i == 1:
            point, norm = (-4.0, 0.0, 0.0, 0.0), _unit(np.array([1.0, 0, 0, 0]) + rng.normal(0, 0.05, 4))
        else:
            point = (rng.normal(0, 0.5), 2.0 + rng.normal(0, 0.5), -1.5 - 0.12 * (i - 1), rng.normal(0, 0.2))
            norm = _unit(np.array([0, 0, 1.0, 0]) + rng.normal(0, 0.1, 4))
        _set(s.point, point)
        _set(s.norm, norm)
        set_material(s.material, next_material())
        d.n_spaces += 1


def compose(rt4, spaces=0, spheres=0, cylinders=0, unions=0, hypercubes=0, tigers=0, groups=None, seed=1,
            sphere_r=(0.25, 0.6)):
    """An rt4.SceneDesc with the given object counts. groups: (kind, first, count, outer, new_first) tuples,
    default canonical_groups(). Every sphere and cylinder has its own radius (set_scene verifies each as a divisor;
    measured on the MI355X: 14 ms for the 32 radii of spheres_1_32)."""
    rng = np.random.default_rng(seed)
    d = rt4.SceneDesc()
    counter = [0]

    def next_material():
        counter[0] += 1
        return counter[0] - 1

    _set(d.sky_light, (0.2, 0.6, 1.2))
    _set(d.sun.drct, _unit(np.array([0, 1.0, 1.0, 0]) + rng.normal(0, 0.1, 4)))
    d.sun.angular_size = float(np.float32(0.09 * np.pi))
    _set(d.sun.light, (10.0, 10.0, 0.95))
    d.sun.sharpness = float(np.float32(0.8))
    d.final_light_mode = rt4.FINAL_LIGHT_SUN_SKY

    add_spaces(d, spaces, rng, next_material)

    d.n_spheres = spheres
    for i in range(spheres):
        s = d.spheres[i]
        r = rng.uniform(*sphere_r)
        y = rng.uniform(1.0, 5.0)
        _set(s.center, (rng.uniform(-0.75, 0.75) * (y + 2), y, rng.uniform(-0.33, 0.27) * (y + 2), rng.uniform(-0.5, 0.5) * r))
        s.r = float(np.float32(r))
        set_material(s.material, next_material())

    d.n_cylinders = cylinders
    for i in range(cylinders):  # tubes along (about) y and w, beside and below the camera
        r = rng.uniform(0.12, 0.35)
        while True:
            q = _frame(rng, 0.25)
            point = np.array([rng.uniform(-3, 3), rng.uniform(1, 4), rng.uniform(-1.3, -0.1), rng.uniform(-0.1, 0.1)])
            po = point - FOCUS
            po = po - (po @ q[:, 3]) * q[:, 3] - (po @ q[:, 1]) * q[:, 1]
            if np.linalg.norm(po) > r + 0.2:  # the camera is outside
                break
        _cylinder(d.cylinders[i], point, q[:, 3], q[:, 1], r)
        set_material(d.cylinders[i].material, next_material())

    # composites: side by side across the view
    n_comp = unions + hypercubes + tigers
    size = 0.8 if n_comp == 1 else 0.55
    slots = [np.array([(i - (n_comp - 1) / 2.0) * 1.7, 3.0 + 0.3 * i, -0.3, 0.0]) + rng.normal(0, 0.1, 4)
             for i in range(n_comp)]
    d.n_unions = unions
    for i in range(unions):  # the reference's union (cylinder4d): axes pairs (x, w) and (z, y) through one point
        q, c = _frame(rng, 0.2), slots.pop(0)
        u = d.unions[i]
        _cylinder(u.cylinder1, c, q[:, 0], q[:, 3], size * rng.uniform(0.9, 1.1))
        _cylinder(u.cylinder2, c, q[:, 2], q[:, 1], size * rng.uniform(0.9, 1.1))
        set_material(u.cylinder1.material, next_material())
        set_material(u.cylinder2.material, next_material())
    d.n_hypercubes = hypercubes
    for i in range(hypercubes):  # init_hypercube (shader.frag:374-392) on the standard axes
        c, r = slots.pop(0).astype(np.float32), np.float32(size * rng.uniform(0.8, 1.0))
        eye = np.eye(4, dtype=np.float32)
        for sgn in range(2):
            for a in range(4):
                cube = d.hypercubes[i].cubes[sgn * 4 + a]
                sr = r if sgn == 0 else -r
                # point + axis * r, one fma per component: exact here, the axis has a single 1
                _set(cube.point, c + eye[a] * sr)
                _set(cube.norm, eye[a] if sgn == 0 else -eye[a])
                others = [k for k in range(4) if k != a]
                _set(cube.x, eye[others[0]])
                _set(cube.y, eye[others[1]])
                _set(cube.z, eye[others[2]])
                cube.r = float(r)
                set_material(cube.material, next_material())
    d.n_tigers = tigers
    for i in range(tigers):  # init_tiger (shader.frag:303-314): point and axes shared inside each pair
        q, c = _frame(rng, 0.2), slots.pop(0)
        inner, outer = 0.64 * size * rng.uniform(0.9, 1.1), size * rng.uniform(0.95, 1.1)
        t = d.tigers[i]
        _cylinder(t.inner_cyl1, c, q[:, 0], q[:, 3], inner)
        _cylinder(t.outer_cyl1, c, q[:, 0], q[:, 3], outer)
        _cylinder(t.inner_cyl2, c, q[:, 2], q[:, 1], inner)
        _cylinder(t.outer_cyl2, c, q[:, 2], q[:, 1], outer)
        for cyl in (t.inner_cyl1, t.outer_cyl1, t.inner_cyl2, t.outer_cyl2):
            set_material(cyl.material, next_material())

    set_groups(d, canonical_groups(rt4, spaces, spheres, cylinders, unions, hypercubes, tigers) if groups is None
               else groups)
    return d


# ------------------------------------------------------------------------------------------- objects
def _color(m):
    return tuple(np.float32(x).item() for x in m.color)


def objects(d):
    """Every object of the scene, tested or not: (kind, index, colours of its materials)."""
    out = []
    for i in range(d.n_spaces):
        out.append((1, i, [_color(d.spaces[i].material)]))
    for i in range(d.n_spheres):
        out.append((2, i, [_color(d.spheres[i].material)]))
    for i in range(d.n_cylinders):
        out.append((3, i, [_color(d.cylinders[i].material)]))
    for i in range(d.n_unions):
        u = d.unions[i]
        out.append((4, i, [_color(u.cylinder1.material), _color(u.cylinder2.material)]))
    for i in range(d.n_hypercubes):
        out.append((5, i, [_color(c.material) for c in d.hypercubes[i].cubes]))
    for i in range(d.n_tigers):
        t = d.tigers[i]
        out.append((6, i, [_color(c.material) for c in (t.inner_cyl1, t.outer_cyl1, t.inner_cyl2, t.outer_cyl2)]))
    return out


def tested_objects(d):
    """The (kind, index) pairs some group of the scene tests."""
    seen = set()
    for g in d.groups[: d.n_groups]:
        seen |= {(g.kind, g.first + k) for k in range(g.count)}
    return seen


def wins_per_material(d, hit, color):
    """{(kind, index, material number within the object): rays it won}, read from the colour output of
    find_intersection."""
    color = np.ascontiguousarray(color, np.float32)
    return {(kind, idx, j): int(((hit > 0) & (color == np.array(c, np.float32)).all(axis=1)).sum())
            for kind, idx, cols in objects(d) for j, c in enumerate(cols)}


# ---------------------------------------------------------------------------------------------- rays
def _complement(a1, a2, rng):
    """Two unit vectors spanning the plane orthogonal to the (orthonormal) axes a1, a2."""
    q = np.linalg.qr(np.stack([a1, a2] + list(rng.normal(size=(2, 4)))).T)[0].T
    return q[2], q[3]


def _f64(v):
    return np.array(v[:4], np.float64)


def _targets(d, kind, i, n, rng):
    """n points inside (on, for a space) object i of a kind."""
    if kind == 1:
        s = d.spaces[i]
        p, nn = _f64(s.point), _unit(_f64(s.norm))
        v = rng.normal(0, 2.0, (n, 4))
        return p + v - (v @ nn)[:, None] * nn
    if kind == 2:
        s = d.spheres[i]
        v = rng.normal(size=(n, 4))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        return _f64(s.center) + v * (s.r * rng.uniform(0, 1, (n, 1)) ** 0.25)
    if kind == 3:
        c = d.cylinders[i]
        a1, a2 = _f64(c.axis1), _f64(c.axis2)
        b1, b2 = _complement(a1, a2, rng)
        rho, phi = c.r * np.sqrt(rng.uniform(0, 1, (n, 1))), rng.uniform(0, 2 * np.pi, (n, 1))
        return (_f64(c.point) + rng.uniform(-2, 2, (n, 1)) * a1 + rng.uniform(-2, 2, (n, 1)) * a2
                + rho * (np.cos(phi) * b1 + np.sin(phi) * b2))
    if kind == 4:
        u = d.unions[i]
        return _f64(u.cylinder1.point) + rng.uniform(-0.5, 0.5, (n, 4)) * min(u.cylinder1.r, u.cylinder2.r)
    if kind == 5:
        cubes = d.hypercubes[i].cubes
        centre = np.mean([_f64(c.point) for c in cubes], axis=0)
        return centre + rng.uniform(-0.9, 0.9, (n, 4)) * cubes[0].r
    t = d.tigers[i]  # between the inner and the outer radius around both axes planes
    mid = 0.5 * (t.inner_cyl1.r + t.outer_cyl1.r)
    al, be = rng.uniform(0, 2 * np.pi, (n, 1)), rng.uniform(0, 2 * np.pi, (n, 1))
    return (_f64(t.inner_cyl1.point) + mid * (np.cos(al) * _f64(t.inner_cyl2.axis1) + np.sin(al) * _f64(t.inner_cyl2.axis2))
            + mid * (np.cos(be) * _f64(t.inner_cyl1.axis1) + np.sin(be) * _f64(t.inner_cyl1.axis2)))


def aimed_rays(d, n_per_object, seed, n_background=4000, focus=FOCUS):
    """For every object of the scene n_per_object rays (a composite: as many for each of its cells or faces)
    towards a random point inside it, with a direction jitter of about 0.02 rad: a quarter start at the camera focus, the others 0.05 to 8 away from their target
    (log-uniform) in a uniform direction. Then n_background rays of test_gpu_parity.random_rays. Returns (n, 8)
    float32."""
    from test_gpu_parity import random_rays

    rng = np.random.default_rng(seed)
    out = []
    for kind, i, cols in objects(d):
        n = n_per_object * len(cols)
        tgt = _targets(d, kind, i, n, rng)
        u = rng.normal(size=(n, 4))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        org = tgt + u * np.exp(rng.uniform(np.log(0.05), np.log(8.0), (n, 1)))
        org[: n // 4] = focus
        v = tgt - org
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        v += rng.normal(0, 0.02, v.shape)
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        out.append(np.concatenate([org, v], axis=1))
    out.append(random_rays(n_background, seed + 1))
    return np.concatenate(out).astype(np.float32)


def case_rays(d, seed, focus=FOCUS):
    """About 20000 rays for a scene: 16000 aimed ones shared among its materials, 4000 background rays."""
    n_mat = sum(len(cols) for _, _, cols in objects(d))
    return aimed_rays(d, 16000 // n_mat, seed, focus=focus)


# --------------------------------------------------------------------------------------------- cases
GENERIC = 0xFFFFFFFF
S, SPH, CYL, UNI, HYP, TIG = 1, 2, 3, 4, 5, 6  # rt4_group_kind

# name -> (expected kernel_shape, compose() arguments). Counts are (spaces, spheres, cylinders, unions,
# hypercubes, tigers); a runtime-count shape is the plain kind bits with zero count fields (rt4.h).
RUNTIME_CASES = {
    "spaces_1": (0x01, dict(spaces=1)),
    "spaces_3": (0x01, dict(spaces=3)),
    "spaces_32": (0x01, dict(spaces=32)),  # RT4_MAX_SPACES
    "spheres_1_1": (0x03, dict(spaces=1, spheres=1, sphere_r=(0.9, 1.0))),
    "spheres_1_3": (0x03, dict(spaces=1, spheres=3)),
    "spheres_2_2": (0x03, dict(spaces=2, spheres=2)),
    "spheres_9_2": (0x03, dict(spaces=9, spheres=2)),
    "spheres_1_32": (0x03, dict(spaces=1, spheres=32)),  # RT4_MAX_SPHERES: pending-mask bit 31
    "spheres_2_0": (0x03, dict(spaces=2, groups=[(S, 0, 2, 0, 1), (SPH, 0, 0, 1, 1)])),  # an empty spheres group
    "sphere_untested_tiger": (0x03, None),  # the `sphere` scene + a tiger no group tests: not the exact-count kernel
    "union_2": (0x09, dict(spaces=2, unions=1)),
    "hypercube_2": (0x11, dict(spaces=2, hypercubes=1)),
    "tiger_2": (0x21, dict(spaces=2, tigers=1)),
    "tiger_5": (0x21, dict(spaces=5, tigers=1)),
    "all_1_3_1": (0x3F, dict(spaces=1, spheres=3, cylinders=1, unions=1, hypercubes=1, tigers=1)),
    "all_2_2_1": (0x3F, dict(spaces=2, spheres=2, cylinders=1, unions=1, hypercubes=1, tigers=1)),
    "all_2_3_2": (0x3F, dict(spaces=2, spheres=3, cylinders=2, unions=1, hypercubes=1, tigers=1)),
    "all_3_1_16": (0x3F, dict(spaces=3, spheres=1, cylinders=16, unions=1, hypercubes=1, tigers=1)),  # RT4_MAX_CYLINDERS
}
GENERIC_CASES = {
    "spaces_cylinders": (GENERIC, dict(spaces=2, cylinders=3)),  # a kind set without a variant
    "spheres_only": (GENERIC, dict(spheres=14, sphere_r=(0.7, 1.1))),
    "unions_2": (GENERIC, dict(spaces=2, unions=2)),
    "hypercubes_2": (GENERIC, dict(spaces=2, hypercubes=2)),
    "tigers_2": (GENERIC, dict(spaces=2, tigers=2)),
    "tigers_4": (GENERIC, dict(spaces=2, tigers=4)),  # RT4_MAX_TIGERS
    # outer = false: a ray from outside passes the front wall and hits the far one from inside, as in a room
    "outer_0": (GENERIC, dict(spaces=2, spheres=3, cylinders=2, sphere_r=(0.5, 0.9),
                              groups=[(S, 0, 2, 0, 1), (SPH, 0, 3, 0, 1), (CYL, 0, 2, 0, 1)])),
    "new_first_0": (GENERIC, dict(spaces=2, spheres=3, groups=[(S, 0, 2, 0, 0), (SPH, 0, 3, 1, 0)])),
    "sub_range": (GENERIC, dict(spaces=3, spheres=3, groups=[(S, 0, 3, 0, 1), (SPH, 1, 1, 1, 1)])),
    "kind_twice": (GENERIC, dict(spaces=2, spheres=4, groups=[(SPH, 0, 4, 1, 1), (S, 0, 2, 0, 1), (SPH, 0, 4, 1, 1)])),
    "tiger_first": (GENERIC, dict(spaces=2, tigers=1, groups=[(TIG, 0, 1, 0, 1), (S, 0, 2, 0, 1)])),
    "snippet": (GENERIC, None),  # test_boundary.SNIPPET + two spaces
    "tie_new_first_1": (GENERIC, None),  # two coincident spheres, closest(new, inter)
    "tie_new_first_0": (GENERIC, None),  # two coincident spheres, closest(inter, new)
}
CASES = {**RUNTIME_CASES, **GENERIC_CASES}
# The default camera sits on the axes plane of SNIPPET's tube (inside it, so every ray hits the tube): that case
# is seen from one unit higher.
CASE_FOCUS = {"snippet": (0.0, -2.0, 1.0, 0.0)}


def case_focus(name):
    return CASE_FOCUS.get(name, tuple(float(x) for x in FOCUS))


def case_uniforms(rt4, name, width, height, samples, reflections, seed):
    """make_uniforms of the case's camera."""
    return rt4.make_uniforms(width, height, samples=samples, reflections=reflections, seed=seed, focus=case_focus(name))


def case_seed(name):
    return 9999 if name.startswith("tie_") else 9000 + list(CASES).index(name)  # the tie scenes share their rays


def case_scene_and_rays(rt4, name):
    d = build_case(rt4, name)
    return d, case_rays(d, case_seed(name), focus=np.array(case_focus(name)))
# one case per runtime-count shape and two generic ones also run three pipelined progressive frames
FRAMES_CASES = ["spaces_3", "spheres_2_2", "union_2", "hypercube_2", "tiger_2", "all_2_2_1", "outer_0", "tiger_first"]
# scenes of spaces, spheres and cylinders only: the float64 reference of test_scene_shapes.py covers them
SIMPLE_CASES = [n for n, (_, kw) in CASES.items() if kw is not None and not any(
    kw.get(k) for k in ("unions", "hypercubes", "tigers"))] + ["sphere_untested_tiger", "snippet"]


def tie_scene(rt4, new_first):
    """Two coincident spheres with different colours in one spheres group (no spaces: a kind set without a
    variant, so the generic kernel). closest(new, inter) keeps sphere 0 on the tie, closest(inter, new) takes
    sphere 1 (rt4.h rt4_group.new_first)."""
    d = compose(rt4, spheres=2, seed=5, groups=[(SPH, 0, 2, 1, new_first)])
    _set(d.spheres[0].center, (0.0, 1.5, 0.0, 0.0))
    d.spheres[0].r = 1.75
    _set(d.spheres[1].center, (0.0, 1.5, 0.0, 0.0))
    d.spheres[1].r = 1.75
    return d


def build_case(rt4, name):
    """The rt4.SceneDesc of a case of CASES; the seed is the case's position in the table."""
    _, kw = CASES[name]
    seed = 100 + list(CASES).index(name)
    if kw is not None:
        return compose(rt4, seed=seed, **kw)
    if name == "sphere_untested_tiger":
        d = rt4.SceneDesc.from_buffer_copy(rt4.Scene.builtin("sphere").to_bytes())
        d.n_tigers = 1
        d.tigers[0] = compose(rt4, tigers=1, seed=seed).tigers[0]
        return d
    if name == "snippet":
        from test_boundary import SNIPPET

        d = rt4.Scene.parse(SNIPPET).desc
        counter = iter(range(100, 200))
        add_spaces(d, 2, np.random.default_rng(seed), lambda: next(counter))
        set_groups(d, [(g.kind, g.first, g.count, g.outer, g.new_first) for g in d.groups[: d.n_groups]]
                   + [(S, 0, 2, 0, 1)])
        return d
    return tie_scene(rt4, 1 if name == "tie_new_first_1" else 0)
