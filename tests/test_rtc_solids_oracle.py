"""CPU tier: the oracle's RTC solids, CSG and scopes pinned against references that share nothing with it or with the kernel, plus
the small world builder that tests/test_gpu_rtc_solids.py imports to hold the kernel to the oracle.

  a. CSG membership: random trees of closed solids carry a numpy predicate inside(p) composed from the solids' implicit inequalities
     and the inverse matrices; the oracle's sorted t list of a ray must be exactly the parameters at which membership toggles.
  b. Root residuals: the quadric roots the oracle returns, put back into a t^2 + b t + c at 60 digits, stay within a derived
     first-order rounding bound.
  c. Directed known answers that the reference's own unit tables (tests/test_known_answers_rtc_shapes.py) do not have.
"""
import math

import numpy as np

EPS = 1e-8  # cylinder.rs:9 / cone.rs:9


# ----------------------------------------------------------------------------- matrices
def T(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def S(x, y, z):
    return np.diag([float(x), float(y), float(z), 1.0])


def R(axis, angle):
    c, s = math.cos(angle), math.sin(angle)
    m = np.eye(4)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    m[i, i], m[i, j], m[j, i], m[j, j] = c, -s, s, c
    return m


def apply_point(m, p):
    return np.asarray(p, dtype=np.float64) @ m[:3, :3].T + m[:3, 3]


def apply_vec(m, v):
    return np.asarray(v, dtype=np.float64) @ m[:3, :3].T


# ----------------------------------------------------------------------------- world builder
class WorldBuilder:
    """Records for RtcWorld.from_arrays.  Every method returns the (kind, index) reference of what it made; material 0 is a plain white
    one.  Leaf identities in intersection records are n_triangles + shape index (triangles: their own index)."""

    def __init__(self, api):
        self.api = api
        self.shapes, self.tr, self.csgs, self.groups, self.items, self.boundeds, self.tris, self.mats, self.pats = [], [], [], [], [], [], [], [], []
        self.material()

    def material(self, color=(1, 1, 1), pattern=0, **kw):
        m = np.zeros(1, dtype=self.api.RTC_MATERIAL)
        m["color"], m["ambient"], m["diffuse"], m["specular"], m["shininess"], m["refractive_index"], m["pattern"] = color, 0.1, 0.9, 0.9, 200.0, 1.0, pattern
        for k, v in kw.items():
            m[k] = v
        self.mats.append(m[0])
        return len(self.mats) - 1

    def pattern(self, kind, a, b, matrix):
        """-> the 1-based index a material's `pattern` field takes"""
        p = np.zeros(1, dtype=self.api.RTC_PATTERN)
        p["kind"], p["a"], p["b"], p["inverse"] = kind, a, b, np.linalg.inv(matrix).reshape(16)
        self.pats.append(p[0])
        return len(self.pats)

    def shape(self, kind, minimum=None, maximum=None, closed=0, material=0):
        r = np.zeros(1, dtype=self.api.RTC_SHAPE)[0]
        r["kind"], r["material"], r["closed"] = kind, material, closed
        if minimum is not None:
            r["has_minimum"], r["minimum"] = 1, minimum
        if maximum is not None:
            r["has_maximum"], r["maximum"] = 1, maximum
        self.shapes.append(r)
        return (kind, len(self.shapes) - 1)

    def leaf(self, ref):
        """the `object` value of a shape's intersection records; valid once every triangle of the world is added"""
        return len(self.tris) + ref[1]

    def xf(self, matrix, child):
        self.tr.append(self.api.rtc_transformed(matrix, child[0], child[1]))
        return (self.api.O_TRANSFORMED, len(self.tr) - 1)

    def csg(self, operation, left, right):
        c = np.zeros(1, dtype=self.api.RTC_CSG)[0]
        c["operation"] = operation
        c["left"]["kind"], c["left"]["index"] = left
        c["right"]["kind"], c["right"]["index"] = right
        self.csgs.append(c)
        return (self.api.O_CSG, len(self.csgs) - 1)

    def group(self, children):
        g = np.zeros(1, dtype=self.api.RTC_GROUP)[0]
        g["first"], g["count"] = len(self.items), len(children)
        self.items.extend(children)
        self.groups.append(g)
        return (self.api.O_GROUP, len(self.groups) - 1)

    def bounded(self, minimum, maximum, child):
        b = np.zeros(1, dtype=self.api.RTC_BOUNDED)[0]
        b["minimum"], b["maximum"] = minimum, maximum
        b["child"]["kind"], b["child"]["index"] = child
        self.boundeds.append(b)
        return (self.api.O_BOUNDED, len(self.boundeds) - 1)

    def triangle(self, p1, p2, p3, normals=None, material=0):
        """Triangle::new / SmoothTriangle (triangle.rs): e1 = p2 - p1, e2 = p3 - p1, flat normal = unit(e2 x e1)"""
        p1, p2, p3 = (np.asarray(p, dtype=np.float64) for p in (p1, p2, p3))
        t = np.zeros(1, dtype=self.api.RTC_TRIANGLE)[0]
        t["p1"], t["e1"], t["e2"], t["material"] = p1, p2 - p1, p3 - p1, material
        if normals is None:
            n = np.cross(p3 - p1, p2 - p1)
            t["n1"] = n / math.sqrt(float(n @ n))
        else:
            t["smooth"], t["n1"], t["n2"], t["n3"] = 1, normals[0], normals[1], normals[2]
        self.tris.append(t)
        return (self.api.O_TRIANGLE, len(self.tris) - 1)

    def world(self, rl, roots, lights=(), **kw):
        api = self.api

        def arr(records, dt):
            return np.array(records, dtype=dt) if records else ()
        objs = np.zeros(len(roots), dtype=api.HREF)
        objs["kind"], objs["index"] = [r[0] for r in roots], [r[1] for r in roots]
        items = np.zeros(len(self.items), dtype=api.HREF)
        if self.items:
            items["kind"], items["index"] = [r[0] for r in self.items], [r[1] for r in self.items]
        lt = np.zeros(len(lights), dtype=api.RTC_LIGHT)
        if len(lights):
            lt["position"], lt["intensity"] = [p for p, _ in lights], [i for _, i in lights]
        return rl.RtcWorld.from_arrays(arr(self.tris, api.RTC_TRIANGLE), arr(self.mats, api.RTC_MATERIAL), objs, lt, groups=arr(self.groups, api.RTC_GROUP),
                                       group_items=items, boundeds=arr(self.boundeds, api.RTC_BOUNDED), transformeds=arr(self.tr, api.RTC_TRANSFORMED),
                                       shapes=arr(self.shapes, api.RTC_SHAPE), csgs=arr(self.csgs, api.RTC_CSG), patterns=arr(self.pats, api.RTC_PATTERN), **kw)


# ----------------------------------------------------------------------------- closed solids with their membership predicates
def _r2(p):
    return p[..., 0] ** 2 + p[..., 2] ** 2


def closed_solid(b, which):
    """One of five closed solids and its open interior as a predicate of local-space points.  The cone bounds are those at which the
    reference's cap radius |y| (cone.rs check_cap) is the true one, y^2."""
    api = b.api
    if which == 0:
        return b.shape(api.O_SPHERE), lambda p: (p * p).sum(-1) < 1
    if which == 1:
        return b.shape(api.O_CUBE), lambda p: np.abs(p).max(-1) < 1
    if which == 2:
        return b.shape(api.O_CYLINDER, -1.0, 1.0, 1), lambda p: (_r2(p) < 1) & (np.abs(p[..., 1]) < 1)
    if which == 3:
        return b.shape(api.O_CONE, -1.0, 0.0, 1), lambda p: (_r2(p) < p[..., 1] ** 2) & (p[..., 1] > -1) & (p[..., 1] < 0)
    return b.shape(api.O_CONE, -1.0, 1.0, 1), lambda p: (_r2(p) < p[..., 1] ** 2) & (np.abs(p[..., 1]) < 1)


def random_matrix(rng, spread):
    return T(*rng.uniform(-spread, spread, 3)) @ R(int(rng.integers(0, 3)), rng.uniform(-3, 3)) @ S(*rng.uniform(0.5, 1.5, 3))


def transformed_solid(b, matrix, node, inside):
    inv = np.linalg.inv(matrix)
    return b.xf(matrix, node), (lambda p, inv=inv, f=inside: f(apply_point(inv, p)))


def csg_predicate(operation, fl, fr):
    if operation == 0:  # csg.rs:16-28 by what it is meant to compute
        return lambda p: fl(p) | fr(p)
    if operation == 1:
        return lambda p: fl(p) & fr(p)
    return lambda p: fl(p) & ~fr(p)


def random_csg_tree(b, rng, depth):
    """-> (reference, inside).  Leaves under translate . rotate . non-uniform scale, inner nodes union / intersection / difference nested
    up to `depth` deep, half of them under a further Transformed."""
    if depth == 0 or rng.random() < 0.25:
        node, f = closed_solid(b, int(rng.integers(0, 5)))
        return transformed_solid(b, random_matrix(rng, 0.45), node, f)
    left, fl = random_csg_tree(b, rng, depth - 1)
    right, fr = random_csg_tree(b, rng, depth - 1)
    operation = int(rng.integers(0, 3))
    node, f = b.csg(operation, left, right), csg_predicate(operation, fl, fr)
    if rng.random() < 0.5:
        node, f = transformed_solid(b, random_matrix(rng, 0.3), node, f)
    return node, f


def rays_at_origin_region(rng, n, distance=9.0, extent=1.5):
    """unit-direction rays from a sphere of radius `distance` aimed into the cube [-extent, extent]^3"""
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = u * distance
    d = rng.uniform(-extent, extent, (n, 3)) - o
    return o, d / np.linalg.norm(d, axis=1, keepdims=True)


CLOSE = 1e-6  # two toggles closer than this cannot be told apart by midpoint samples


def membership_disagreement(ts, o, d, inside, chord=18.0):
    """None when the sorted parameters `ts` are exactly where inside(o + t d) toggles, 'skip' when two of them are closer than CLOSE,
    otherwise a description of the disagreement."""
    ts = np.asarray(ts, dtype=np.float64)
    if len(ts) == 0:
        grid = np.linspace(0.0, chord, int(round(chord / 0.1)) + 1)
        hit = inside(o + grid[:, None] * d)
        return None if not hit.any() else f"no intersections, but inside at t = {grid[np.nonzero(hit)[0][:4]]}"
    if len(ts) > 1 and np.diff(ts).min() < CLOSE:
        return "skip"
    mids = np.concatenate([[ts[0] - 1.0], 0.5 * (ts[1:] + ts[:-1]), [ts[-1] + 1.0]])
    got = inside(o + mids[:, None] * d)
    want = (np.arange(len(mids)) % 2) == 1
    return None if np.array_equal(got, want) else f"{len(ts)} intersections at {ts}, membership between them {got.astype(int)}"


def random_csg_world(rl, seed, depth=4, lights=()):
    """-> (world, inside, the generator to draw the rays from) of one random tree; the root is always a CSG"""
    rng = np.random.default_rng(seed)
    while True:
        b = WorldBuilder(rl.api)
        root, inside = random_csg_tree(b, rng, depth)
        if b.csgs:
            return b.world(rl, [root], lights=lights), inside, rng


# ----------------------------------------------------------------------------- a. membership
def test_csg_lists_are_where_membership_toggles(rl, oracle):
    n_worlds, n_rays = 60, 300
    hit = skipped = deep = 0
    deepest = 0
    for w in range(n_worlds):
        world, inside, rng = random_csg_world(rl, 1000 + w)
        o, d = rays_at_origin_region(rng, n_rays)
        for i in range(n_rays):
            ts = oracle.rtc_intersect(world.desc, o[i], d[i], cap=256)[0]
            hit += len(ts) > 0
            deep += len(ts) >= 4
            deepest = max(deepest, len(ts))
            bad = membership_disagreement(ts, o[i], d[i], inside)
            if bad == "skip":
                skipped += 1
                continue
            assert bad is None, (w, i, bad)
    total = n_worlds * n_rays
    print(f"rays {total} hit {hit} skipped {skipped} with >= 4 intersections {deep} longest list {deepest}")
    assert skipped < 0.01 * total, skipped
    assert hit >= 0.25 * total, hit
    assert deep >= 500, deep


# ----------------------------------------------------------------------------- b. root residuals
def _quadric_world(rl, kind):
    b = WorldBuilder(rl.api)
    return b.world(rl, [b.shape(kind)])


def test_quadric_roots_leave_first_order_residuals(rl, oracle):
    """|f(t)| <= eps (3A t^2 + 3B|t| + 3C) + eps sqrt(disc) (4|t| + (3(B^2 + 4AC) / (2 sqrt(disc)) + B + sqrt(disc)) / |2a|), eps = 2^-53.
    The first term is what the roundings of a, b and c (three operations deep, on term magnitudes A, B, C) move f by at t; the second is
    f'(t) = +-sqrt(disc) times the error of t itself: the discriminant's roundings (relative to B^2 + 4AC, through the square root), -b +-
    sqrt(disc) and the division by 2a.  A, B, C are sums of the absolute values of the terms: the cone's coefficients cancel."""
    import mpmath as mp
    api = rl.api
    eps = mp.mpf(2) ** -53
    rng = np.random.default_rng(9)
    with mp.workdps(60):
        for kind in (api.O_SPHERE, api.O_CYLINDER, api.O_CONE):
            world = _quadric_world(rl, kind)
            n = 2500
            o = rng.uniform(-3, 3, (n, 3))
            d = rng.uniform(-1, 1, (n, 3)) - o  # unnormalised
            worst, used = 0.0, 0
            for i in range(n):
                ts = oracle.rtc_intersect(world.desc, o[i], d[i], cap=16)[0]
                if len(ts) != 2:
                    continue
                ox, oy, oz = (mp.mpf(float(v)) for v in o[i])
                dx, dy, dz = (mp.mpf(float(v)) for v in d[i])
                if kind == api.O_SPHERE:
                    a, bb, c = dx * dx + dy * dy + dz * dz, 2 * (ox * dx + oy * dy + oz * dz), ox * ox + oy * oy + oz * oz - 1
                    A, B, Cm = a, 2 * (abs(ox * dx) + abs(oy * dy) + abs(oz * dz)), ox * ox + oy * oy + oz * oz + 1
                elif kind == api.O_CYLINDER:
                    a, bb, c = dx * dx + dz * dz, 2 * (ox * dx + oz * dz), ox * ox + oz * oz - 1
                    A, B, Cm = a, 2 * (abs(ox * dx) + abs(oz * dz)), ox * ox + oz * oz + 1
                else:
                    a, bb, c = dx * dx - dy * dy + dz * dz, 2 * (ox * dx - oy * dy + oz * dz), ox * ox - oy * oy + oz * oz
                    A, B, Cm = dx * dx + dy * dy + dz * dz, 2 * (abs(ox * dx) + abs(oy * dy) + abs(oz * dz)), ox * ox + oy * oy + oz * oz
                disc = bb * bb - 4 * a * c
                if disc <= 0 or abs(a) < 1e-3 * A or disc < 1e-3 * (B * B + 4 * A * Cm):
                    continue
                sq = mp.sqrt(disc)
                for t in ts:
                    t = mp.mpf(float(t))
                    f = a * t * t + bb * t + c
                    bound = eps * (3 * A * t * t + 3 * B * abs(t) + 3 * Cm) + eps * sq * (4 * abs(t) + (3 * (B * B + 4 * A * Cm) / (2 * sq) + B + sq) / abs(2 * a))
                    worst = max(worst, float(abs(f) / bound))
                    used += 1
                    assert abs(f) <= bound, (kind, i, float(t), float(f), float(bound))
            print(f"kind {kind}: {used} roots, worst |f| / bound {worst:.3f}")
            assert used >= 1000, (kind, used)


# ----------------------------------------------------------------------------- c. directed known answers
def _one(rl, kind, **kw):
    b = WorldBuilder(rl.api)
    return b.world(rl, [b.shape(kind, **kw)])


def _isect(oracle, world, o, d):
    ts, _, normals = oracle.rtc_intersect(world.desc, o, d)
    return [float(t) for t in ts], normals


def _ulp_close(got, want):
    want = np.asarray(want, dtype=np.float64)
    return bool(np.all(np.abs(np.asarray(got) - want) <= np.spacing(np.maximum(np.abs(want), 1e-300))))


SQH = math.sqrt(0.5)


def test_cone_ray_parallel_to_the_side_has_one_root_and_none_through_the_apex(rl, oracle):
    """cone.rs:100-107.  d = (0, 1, 1) from (0, 0, -1): a = 0 - 1 + 1 = 0, b = 2 (-1)(1) = -2, c = 0 - 0 + 1 = 1, so the single root is
    -c / (2 b) = 1/4, the reference's own formula (the ray meets the cone's surface at t = 1/2; the book's b carries no factor 2).  It is
    pushed without an in_bounds test, so bounds that exclude y = 1/4 keep it.  Its point (0, 1/4, -3/4) has y > 0: the wall normal is
    unit(0, -3/4, -3/4).  From the apex a = b = c = 0: nothing."""
    api = rl.api
    ts, normals = _isect(oracle, _one(rl, api.O_CONE), (0, 0, -1), (0, 1, 1))
    assert ts == [0.25]
    assert _ulp_close(normals[0], (0.0, -SQH, -SQH))
    assert _isect(oracle, _one(rl, api.O_CONE, minimum=-2.0, maximum=-1.0), (0, 0, -1), (0, 1, 1))[0] == [0.25]
    assert _isect(oracle, _one(rl, api.O_CONE), (0, 0, 0), (0, 1, 1))[0] == []
    assert _isect(oracle, _one(rl, api.O_CONE), (0, 0, 0), (0, -1, 1))[0] == []
    # a closed cone still offers its caps to such a ray: y = 1 at t = 1 with x^2 + z^2 = 0 <= 1 and the cap's normal; y = -1 at t = -1
    # with z = -2 misses
    ts, normals = _isect(oracle, _one(rl, api.O_CONE, minimum=-1.0, maximum=1.0, closed=1), (0, 0, -1), (0, 1, 1))
    assert ts == [0.25, 1.0] and np.array_equal(normals[1], (0.0, 1.0, 0.0))


def test_cylinders_with_one_bound(rl, oracle):
    """cylinder.rs:21-28.  (0, -1, -2) + t (0, 1, 1): a = 1, b = -4, c = 3, disc = 4, roots 1 and 3 at y = 0 and y = 2.
    minimum 0 alone rejects the first (y > 0 is strict), maximum 1 alone the second.  Closed with minimum 0 alone: the cap at t = 1 lies
    at x^2 + z^2 = 1 <= 1, on the rim, and is kept; its point is not inside the radius, so it carries the wall's normal (0, 0, -1)."""
    api = rl.api
    o, d = (0, -1, -2), (0, 1, 1)
    assert _isect(oracle, _one(rl, api.O_CYLINDER), o, d)[0] == [1.0, 3.0]
    assert _isect(oracle, _one(rl, api.O_CYLINDER, minimum=0.0), o, d)[0] == [3.0]
    assert _isect(oracle, _one(rl, api.O_CYLINDER, maximum=1.0), o, d)[0] == [1.0]
    assert _isect(oracle, _one(rl, api.O_CYLINDER, minimum=-0.5), o, d)[0] == [1.0, 3.0]
    assert _isect(oracle, _one(rl, api.O_CYLINDER, maximum=2.5), o, d)[0] == [1.0, 3.0]
    ts, normals = _isect(oracle, _one(rl, api.O_CYLINDER, minimum=0.0, closed=1), o, d)
    assert ts == [1.0, 3.0] and np.array_equal(normals[0], (0.0, 0.0, -1.0)) and np.array_equal(normals[1], (0.0, 0.0, 1.0))
    # a closed cylinder with a maximum alone has one cap: straight down the axis from above, t = 3 - 1 = 2 and nothing else
    ts, normals = _isect(oracle, _one(rl, api.O_CYLINDER, maximum=1.0, closed=1), (0, 3, 0), (0, -1, 0))
    assert ts == [2.0] and np.array_equal(normals[0], (0.0, 1.0, 0.0))


def test_cones_with_one_bound(rl, oracle):
    """cone.rs:21-28.  (0, -2, -1) + t (0, 1, 0): a = -1, b = 4, c = -3, disc = 4, t0 = (-4 - 2) / -2 = 3 at y = 1 and t1 = 1 at y = -1
    (a < 0 puts the larger root first).  minimum -1 alone keeps y = 1 only, maximum 1 alone keeps y = -1 only; both are strict."""
    api = rl.api
    o, d = (0, -2, -1), (0, 1, 0)
    assert _isect(oracle, _one(rl, api.O_CONE), o, d)[0] == [1.0, 3.0]
    assert _isect(oracle, _one(rl, api.O_CONE, minimum=-1.0), o, d)[0] == [3.0]
    assert _isect(oracle, _one(rl, api.O_CONE, maximum=1.0), o, d)[0] == [1.0]
    assert _isect(oracle, _one(rl, api.O_CONE, minimum=-1.5), o, d)[0] == [1.0, 3.0]
    assert _isect(oracle, _one(rl, api.O_CONE, maximum=1.5), o, d)[0] == [1.0, 3.0]
    assert _isect(oracle, _one(rl, api.O_CONE, minimum=-1.0, maximum=1.0), o, d)[0] == []


def test_cone_caps_have_radius_sqrt_of_abs_y(rl, oracle):
    """cone.rs:30-35 check_cap: x^2 + z^2 <= |y|, not y^2.  Cone closed between -2 and 0.5, rays straight up from y = -5.
    x = 0.625: a = -1, b = 10, c = 0.390625 - 25, disc = 1.5625, t0 = (-10 - 1.25) / -2 = 5.625 at y = 0.625 (rejected), t1 = 4.375 at
    y = -0.625 (kept).  Lower cap t = 3: 0.390625 <= 2.  Upper cap t = 5.5: 0.390625 <= 0.5, where the true radius 0.5 would miss.
    The upper cap hit is outside normal_at's dist2 < max^2 = 0.25 (cone.rs:67-69), so it carries the wall's normal unit(x, -x, 0).
    x = 1.5: roots 6.5 at y = 1.5 (rejected) and 3.5 at y = -1.5; lower cap 2.25 <= 2 fails, where the true radius 2 would hit."""
    api = rl.api
    w = _one(rl, api.O_CONE, minimum=-2.0, maximum=0.5, closed=1)
    ts, normals = _isect(oracle, w, (0.625, -5, 0), (0, 1, 0))
    assert ts == [3.0, 4.375, 5.5]
    assert np.array_equal(normals[0], (0.0, -1.0, 0.0)) and _ulp_close(normals[1], (SQH, SQH, 0.0)) and _ulp_close(normals[2], (SQH, -SQH, 0.0))
    assert _isect(oracle, w, (1.5, -5, 0), (0, 1, 0))[0] == [3.5]
    # x = 0.25, inside both true radii: disc = 0.25, roots 5.25 at y = 0.25 and 4.75 at y = -0.25, both kept, and both caps with their
    # own normals; x = 1.25: 1.5625 <= 2 on the lower cap only, roots 6.25 at y = 1.25 (rejected) and 3.75
    ts, normals = _isect(oracle, w, (0.25, -5, 0), (0, 1, 0))
    assert ts == [3.0, 4.75, 5.25, 5.5] and np.array_equal(normals[0], (0.0, -1.0, 0.0)) and np.array_equal(normals[3], (0.0, 1.0, 0.0))
    assert _isect(oracle, w, (1.25, -5, 0), (0, 1, 0))[0] == [3.0, 3.75]


def test_cube_with_zero_direction_components_from_a_face_plane(rl, oracle):
    """cube.rs:67-79.  Origin (1, 0.5, -3), direction (0, 0, 1): x gives (-1 - 1) / 0 = -inf and (1 - 1) / 0 = NaN, kept in that order
    (-inf > NaN is false); y gives -inf, +inf; z gives 2, 4.  f64::max / min skip the NaN: tmin = 2, tmax = 4, and the ray, which runs
    in the face plane x = 1, counts as a hit.  Both points have |x| = |z| = 1: the x test comes first (cube.rs:22).  From x = -1 the NaN
    is the other element of the pair, with the same result."""
    api = rl.api
    w = _one(rl, api.O_CUBE)
    ts, normals = _isect(oracle, w, (1, 0.5, -3), (0, 0, 1))
    assert ts == [2.0, 4.0] and np.array_equal(normals, [(1.0, 0.0, 0.0)] * 2)
    ts, normals = _isect(oracle, w, (-1, 0.5, -3), (0, 0, 1))
    assert ts == [2.0, 4.0] and np.array_equal(normals, [(-1.0, 0.0, 0.0)] * 2)
    assert _isect(oracle, w, (1.0000000000000002, 0.5, -3), (0, 0, 1))[0] == []
    ts, normals = _isect(oracle, w, (0.5, -3, -1), (0, 1, 0))  # in the plane z = -1: |y| = |z| ties go to y
    assert ts == [2.0, 4.0] and np.array_equal(normals, [(0.0, -1.0, 0.0), (0.0, 1.0, 0.0)])


def test_cube_normals_on_edges_and_corners(rl, oracle):
    """cube.rs:15-30: the first of x, y, z whose magnitude equals the largest wins."""
    api = rl.api
    w = _one(rl, api.O_CUBE)
    cases = [((1, 1, -5), (0, 0, 1), (1, 0, 0)), ((-1, -1, -5), (0, 0, 1), (-1, 0, 0)),  # corners: x
             ((0.5, 1, -5), (0, 0, 1), (0, 1, 0)), ((0.5, -1, -5), (0, 0, 1), (0, -1, 0)),  # y-z edges: y
             ((1, 0.5, -5), (0, 0, 1), (1, 0, 0)), ((-5, 1, 0.25), (1, 0, 0), (-1, 0, 0))]  # x-z and x-y edges: x
    for o, d, n in cases:
        ts, normals = _isect(oracle, w, o, d)
        assert ts == [4.0, 6.0], (o, ts)
        assert np.array_equal(normals[0], n), (o, normals[0])
    # reached diagonally: (-2, -2, -2) + t (1, 1, 1) enters at the corner (-1, -1, -1), leaves at (1, 1, 1)
    ts, normals = _isect(oracle, w, (-2, -2, -2), (1, 1, 1))
    assert ts == [1.0, 3.0] and np.array_equal(normals, [(-1.0, 0.0, 0.0), (1.0, 0.0, 0.0)])


# every ray of the directed tests above: the GPU tier sends them through each primitive world, bare and under its Transformed
DIRECTED_RAYS = [((0, 0, -1), (0, 1, 1)), ((0, 0, 0), (0, 1, 1)), ((0, 0, 0), (0, -1, 1)), ((0, -1, -2), (0, 1, 1)), ((0, 3, 0), (0, -1, 0)),
                 ((0, -2, -1), (0, 1, 0)), ((0.625, -5, 0), (0, 1, 0)), ((1.5, -5, 0), (0, 1, 0)), ((0.25, -5, 0), (0, 1, 0)), ((1.25, -5, 0), (0, 1, 0)),
                 ((1, 0.5, -3), (0, 0, 1)), ((-1, 0.5, -3), (0, 0, 1)), ((1.0000000000000002, 0.5, -3), (0, 0, 1)), ((0.5, -3, -1), (0, 1, 0)),
                 ((1, 1, -5), (0, 0, 1)), ((-1, -1, -5), (0, 0, 1)), ((0.5, 1, -5), (0, 0, 1)), ((0.5, -1, -5), (0, 0, 1)), ((1, 0.5, -5), (0, 0, 1)),
                 ((-5, 1, 0.25), (1, 0, 0)), ((-2, -2, -2), (1, 1, 1))]
