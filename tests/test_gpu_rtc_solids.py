"""GPU tier: rtc_intersect_all and the color_at body (csrc/rl_rtc_full_kernel.h, rl_rtc_color_at_body.inc) held to the oracle ray by ray
and intersection record by record, on a directed matrix of solids, scopes and CSG trees plus the random trees whose membership the CPU
tier (tests/test_rtc_solids_oracle.py) checks.  counts, t, object, normal and hit_index must be equal bit for bit; colours within the
bar tests/test_gpu_ray_query.py sets for libm quantities.  Every branch a test is there for is counted from the oracle's lists and
its reach asserted."""
import math

import numpy as np
import pytest

from test_rtc_solids_oracle import (DIRECTED_RAYS, EPS, R, S, T, WorldBuilder, apply_point, apply_vec, closed_solid, csg_predicate,
                                    membership_disagreement, random_csg_world, rays_at_origin_region, transformed_solid)

pytestmark = pytest.mark.gpu
REL = 1e-9  # tests/test_gpu_ray_query.py: colour-only (libm) quantities
K = 12
LIST_CAP = 48  # RL_RTC_K: overflow has its own test in tests/test_gpu_status_accounting.py
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "flagged")
LIGHT = [((-6.0, 9.0, -7.0), (0.9, 0.9, 0.9))]


def _hit_of(ts):  # intersect.rs:159-168
    want = -1
    for j in range(len(ts)):
        if ts[j] >= 0.0 and (want < 0 or not (ts[want] < ts[j])):
            want = j
    return want


def _equal_the_oracle(rl, oracle, world, o, d, tag, inside=None, color=True):
    """-> the oracle's (ts, objs, normals) per ray, after asserting that the device returned the same"""
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    n = o.shape[0]
    st = {}
    counts, isects, hit_index = world.intersect_rays(o, d, k=K, stats=st, allow_degenerate=True)
    assert st["rays"] == n, (tag, st)
    rgb = world.color_at_rays(o, d, allow_degenerate=True) if color else None
    lists = []
    for i in range(n):
        ts, objs, normals = oracle.rtc_intersect(world.desc, o[i], d[i], cap=64)
        lists.append((ts, objs, normals))
        assert len(ts) <= LIST_CAP, (tag, i, len(ts))
        m = min(len(ts), K)
        same = counts[i] == len(ts) and np.array_equal(isects["t"][i, :m], ts[:m])
        if not same and inside is not None:  # which side is wrong: the membership reference of the CPU tier as a diagnostic
            got = isects["t"][i, :min(int(counts[i]), K)]
            assert same, (tag, i, o[i], d[i], "device:", got, membership_disagreement(got, o[i], d[i], inside) if counts[i] <= K else "list longer than K",
                          "oracle:", ts, membership_disagreement(ts, o[i], d[i], inside))
        assert same, (tag, i, o[i], d[i], counts[i], isects["t"][i, :m], ts)
        assert np.array_equal(isects["object"][i, :m], objs[:m]), (tag, i, isects["object"][i, :m], objs[:m])
        assert np.array_equal(isects["normal"][i, :m], normals[:m]), (tag, i, isects["normal"][i, :m], normals[:m])
        want = _hit_of(ts)
        assert hit_index[i] == (rl.api.NO_HIT if want < 0 else want), (tag, i, hit_index[i], want)
        if color:
            ref = oracle.rtc_color_at(world.desc, o[i], d[i])
            assert np.abs(rgb[i] - ref).max() <= REL * max(1.0, np.abs(ref).max()), (tag, i, rgb[i], ref)
    # nothing may be flagged (a list beyond LIST_CAP is) except by the rays whose list holds a normal the reference could not normalise
    # (NormalizedVec3d::new(..).unwrap() at the cone's apex): the oracle returns those as zero vectors
    clean = np.array([i for i in range(n) if not any((nr == 0.0).all() for nr in lists[i][2])], dtype=np.int64)
    if len(clean) < n:
        st = {}
        world.intersect_rays(o[clean], d[clean], k=0, stats=st)
    assert st["flagged"] == 0, (tag, st)
    return lists


def _inside_rays(rng, n, extent=1.5):
    return rng.uniform(-extent, extent, (n, 3)), rng.normal(size=(n, 3))


def _standard_rays(rng, n_out=300, n_in=100):
    o1, d1 = rays_at_origin_region(rng, n_out)
    o2, d2 = _inside_rays(rng, n_in)
    return np.concatenate([o1, o2]), np.concatenate([d1, d2])


# ----------------------------------------------------------------------------- primitive matrix
M_PRIM = T(4.0, 0.5, -1.0) @ S(2.0, 0.5, 4.0)  # powers of two: a local ray of binary fractions stays exact, zeros stay zeros
BOUNDS = [(-2.0, None), (None, 0.5), (-2.0, 0.5)]


def _variants(api, kind):
    if kind not in (api.O_CYLINDER, api.O_CONE):
        return [dict()]
    v = [dict()] + [dict(minimum=mn, maximum=mx, closed=c) for mn, mx in BOUNDS for c in (0, 1)]
    if kind == api.O_CONE:
        v += [dict(minimum=-1.0, maximum=1.0, closed=1), dict(minimum=-1.0, maximum=0.0, closed=1)]
    return v


def _axis_rays(rng, n):
    """axis-parallel rays with exact zeros from a grid of quarters that holds the face planes, rims and edges: +-1, +-0.5, ..."""
    grid = np.arange(-6, 7) * 0.25
    o = rng.choice(grid, (n, 3))
    axis, sign = rng.integers(0, 3, n), rng.choice([-1.0, 1.0], n)
    o[: n // 2] = np.where(rng.random((n // 2, 3)) < 0.6, rng.choice([-1.0, 1.0], (n // 2, 3)), o[: n // 2])  # many on face planes and edges
    d = np.zeros((n, 3))
    d[np.arange(n), axis] = sign
    o[np.arange(n), axis] = -5.0 * sign
    return o, d


def _aimed_rays(rng, api, kind):
    """rays at cap rims (the reference's radius sqrt|y| and the true |y|), cube edges and corners, and along the cone's side"""
    o, d = [], []
    th = rng.uniform(0, 2 * math.pi, 48)
    for i, t in enumerate(th):
        yb = (-2.0, 0.5, -1.0, 1.0)[i % 4]
        r = (1.0, math.sqrt(abs(yb)), abs(yb))[i % 3] if kind == api.O_CONE else 1.0
        target = np.array([r * math.cos(t), yb, r * math.sin(t)])
        org = target + rng.normal(size=3) * 3.0
        o.append(org), d.append(target - org)
    for i in range(32):  # edges and corners of the cube, from anywhere
        target = rng.choice([-1.0, 1.0], 3)
        if i % 2:
            target[rng.integers(0, 3)] = rng.uniform(-1, 1)
        org = target * 3.0 + rng.normal(size=3)
        o.append(org), d.append(target - org)
    for i in range(32):  # parallel to the cone's side: a = dx^2 - dy^2 + dz^2 vanishes to rounding
        t = i * math.pi / 8 + (0.0 if i < 16 else 0.1)
        o.append(rng.uniform(-2, 2, 3)), d.append(np.array([math.cos(t), rng.choice([-1.0, 1.0]), math.sin(t)]))
    for x in (0.25, 0.5, 0.625, 0.75, 1.0, 1.25, 1.5, 1.75):  # straight through the caps at the radii that tell |y| from y^2
        for z in (0.0, 0.25):
            o.append(np.array([x, -5.0, z])), d.append(np.array([0.0, 1.0, 0.0]))
            o.append(np.array([-z, 5.0, x])), d.append(np.array([0.0, -1.0, 0.0]))
    return np.array(o), np.array(d)


def _reach(api, rec, o, d, ts, normals):
    """Which of the named branches the local ray (o, d) took on the bare shape `rec`, from the oracle's entries (ts, normals) of that
    shape.  The coefficient arithmetic is the reference's (cylinder.rs:98-116, cone.rs:92-116), in its order."""
    got = {}
    kind = rec["kind"]
    ox, oy, oz = (float(v) for v in o)
    dx, dy, dz = (float(v) for v in d)
    if kind == api.O_CUBE:
        for t in ts:
            p = np.sort(np.abs(o + d * t))
            if p[2] == p[1]:
                got["cube edge tie"] = got.get("cube edge tie", 0) + 1
        return got
    if kind not in (api.O_CYLINDER, api.O_CONE):
        return got
    cone = kind == api.O_CONE
    a = dx * dx - dy * dy + dz * dz if cone else dx * dx + dz * dz
    b = 2.0 * ox * dx - 2.0 * oy * dy + 2.0 * oz * dz if cone else 2.0 * ox * dx + 2.0 * oz * dz
    c = ox * ox - oy * oy + oz * oz if cone else ox * ox + oz * oz - 1.0
    if cone and abs(a) < EPS:
        if not abs(b) < EPS and -c / (2.0 * b) in ts:
            got["single-root cone"] = 1
    elif not abs(a) < EPS:
        disc = b * b - 4.0 * a * c
        if not disc < 0.0:
            for t in ((-b - math.sqrt(disc)) / (2.0 * a), (-b + math.sqrt(disc)) / (2.0 * a)):
                y = oy + t * dy
                if rec["has_minimum"] and not rec["has_maximum"] and not y > rec["minimum"]:
                    got["min-only reject"] = got.get("min-only reject", 0) + 1
                if rec["has_maximum"] and not rec["has_minimum"] and not y < rec["maximum"]:
                    got["max-only reject"] = got.get("max-only reject", 0) + 1
    if rec["closed"] and not abs(dy) < EPS:
        for has, yb in ((rec["has_minimum"], rec["minimum"]), (rec["has_maximum"], rec["maximum"])):
            t = (yb - oy) / dy
            for j in np.nonzero(ts == t)[0] if has else ():
                x, z = ox + t * dx, oz + t * dz
                if x * x + z * z <= (abs(yb) if cone else 1.0):
                    got["cap hit"] = got.get("cap hit", 0) + 1
                    if abs(normals[j][1]) != 1.0:  # cap point outside normal_at's radius (cone.rs:67-73, cylinder.rs:71-82): the wall's normal
                        got["cap hit with the wall's normal"] = got.get("cap hit with the wall's normal", 0) + 1
                    break
    return got


PRIM_REACH = {"O_SPHERE": (), "O_PLANE": (), "O_CUBE": ("cube edge tie",),
              "O_CYLINDER": ("cap hit", "cap hit with the wall's normal", "min-only reject", "max-only reject"),
              "O_CONE": ("single-root cone", "cap hit", "cap hit with the wall's normal", "min-only reject", "max-only reject")}


@pytest.mark.parametrize("kind_name", list(PRIM_REACH))
def test_primitive_matrix_equals_the_oracle(rl, oracle, kind_name):
    rl.init(0)
    api = rl.api
    kind = getattr(api, kind_name)
    b = WorldBuilder(api)
    bare = [b.shape(kind, **v) for v in _variants(api, kind)]
    under = [b.xf(M_PRIM, b.shape(kind, **v)) for v in _variants(api, kind)]
    world = b.world(rl, bare + under, lights=LIGHT)
    rng = np.random.default_rng(4100 + kind)
    lo, ld = [], []  # rays in the bare shapes' space; each set is sent as it is and once more through M_PRIM
    o, d = rays_at_origin_region(rng, 150)
    lo.append(o), ld.append(d)
    o, d = _inside_rays(rng, 50)
    lo.append(o), ld.append(d)
    o, d = _axis_rays(rng, 50)
    lo.append(o), ld.append(d)
    lo.append(np.array([r[0] for r in DIRECTED_RAYS], dtype=np.float64)), ld.append(np.array([r[1] for r in DIRECTED_RAYS], dtype=np.float64))
    o, d = _aimed_rays(rng, api, kind)
    lo.append(o), ld.append(d)
    lo, ld = np.concatenate(lo), np.concatenate(ld)
    n_local = lo.shape[0]
    o, d = np.concatenate([lo, apply_point(M_PRIM, lo)]), np.concatenate([ld, apply_vec(M_PRIM, ld)])
    lists = _equal_the_oracle(rl, oracle, world, o, d, kind_name)
    reach, hits = {}, 0
    for i in range(n_local):  # branch accounting on the bare shapes, whose local ray is the world ray
        ts, objs, normals = lists[i]
        hits += len(ts) > 0
        for ref in bare:
            sel = objs == b.leaf(ref)
            for k, v in _reach(api, b.shapes[ref[1]], lo[i], ld[i], ts[sel], normals[sel]).items():
                reach[k] = reach.get(k, 0) + v
    print(kind_name, "rays", o.shape[0], "bare-space rays that hit", hits, "longest list", max(len(l[0]) for l in lists), reach)
    assert hits >= 100, hits
    assert sum(len(l[0]) > 0 for l in lists[n_local:]) >= 100  # and the copies under the Transformed are met too
    for name in PRIM_REACH[kind_name]:
        assert reach.get(name, 0) >= 10, (name, reach)


# ----------------------------------------------------------------------------- scopes
def _patterns(b):
    api = b.api
    return [b.pattern(api.PAT_CHECKER3D, (1, 1, 1), (0.1, 0.2, 0.6), T(0.1, 0.2, 0.3) @ R(1, 0.5) @ S(0.4, 0.3, 0.5)),
            b.pattern(api.PAT_STRIPE, (0.9, 0.3, 0.1), (0.1, 0.8, 0.3), R(2, 0.7) @ S(0.25, 1, 1)),
            b.pattern(api.PAT_RING, (0.2, 0.3, 0.9), (1, 0.9, 0.2), T(0.2, 0, -0.1) @ S(0.3, 0.3, 0.3)),
            b.pattern(api.PAT_GRADIENT, (1, 0, 0), (0, 0, 1), R(1, -0.4) @ S(0.7, 1, 1))]


def _link(i):
    """the i-th matrix of a Transformed chain: translate . rotate . non-uniform scale, kept close to the identity so that a chain of
    eight leaves its shape near the origin"""
    return T(0.11 * ((i % 3) - 1), 0.07 * ((i % 2) * 2 - 1), -0.05 * (i % 4)) @ R(i % 3, 0.35 + 0.2 * i) @ S(1.0 + 0.15 * ((i % 3) - 1), 1.0 - 0.1 * (i % 2), 1.0 + 0.12 * (i % 4) - 0.2)


def _chain(b, depth, child, first=0):
    for i in range(depth):
        child = b.xf(_link(first + depth - 1 - i), child)
    return child


@pytest.mark.parametrize("depth", [1, 3, 8])
def test_transformed_chains_around_a_patterned_shape(rl, oracle, depth):
    """ROP_EXIT re-normalises the normals of its own range only, and the hit's pattern colour comes from rtc_local_ray's replay of the
    whole ENTER chain: 8 is the deepest the library accepts."""
    rl.init(0)
    api = rl.api
    b = WorldBuilder(api)
    pats = _patterns(b)
    cube = b.shape(api.O_CUBE, material=b.material(pattern=pats[0]))
    cone = b.shape(api.O_CONE, minimum=-1.0, maximum=1.0, closed=1, material=b.material(pattern=pats[1]))
    floor = b.xf(T(0, -2.5, 0), b.shape(api.O_PLANE, material=b.material(pattern=pats[2])))
    world = b.world(rl, [_chain(b, depth, cube), b.xf(T(0.4, 0.2, 0.3), _chain(b, depth - 1, cone, first=3)) if depth > 1 else cone, floor], lights=LIGHT)
    o, d = _standard_rays(np.random.default_rng(4200 + depth))
    lists = _equal_the_oracle(rl, oracle, world, o, d, f"chain{depth}")
    assert sum(_hit_of(l[0]) >= 0 and l[1][_hit_of(l[0])] == b.leaf(cube) for l in lists) >= 60  # the hit colour is the chained cube's pattern


def test_a_sibling_after_a_nested_scope_and_nested_groups(rl, oracle):
    """cur_enter must be back at the outer ENTER (op.b) when a later sibling of a nested Transformed is hit, three scopes deep; and Groups
    of overlapping shapes nested in Groups (group.rs:29-42 sorts each group's list) under and beside Transformeds."""
    rl.init(0)
    api = rl.api
    b = WorldBuilder(api)
    pats = _patterns(b)
    mat = [b.material(pattern=p) for p in pats]
    inner = b.group([b.xf(_link(5), b.shape(api.O_CONE, minimum=-1.0, maximum=0.5, closed=1, material=mat[1])), b.shape(api.O_CYLINDER, minimum=-0.5, maximum=0.5, closed=1, material=mat[2])])
    middle = b.group([b.xf(_link(2) @ S(0.8, 0.8, 0.8), inner), b.shape(api.O_CUBE, material=mat[0])])
    scopes = b.xf(T(-1.2, 0, 0) @ _link(1) @ S(0.7, 0.9, 0.6), b.group([b.xf(_link(4), middle), b.shape(api.O_SPHERE, material=mat[3])]))
    overlapping = b.group([b.shape(api.O_SPHERE, material=mat[0]), b.xf(T(0.5, 0.1, 0), b.shape(api.O_SPHERE, material=mat[1])),
                           b.group([b.shape(api.O_CUBE, material=mat[2]), b.xf(R(0, 0.6) @ S(0.6, 1.4, 0.6), b.shape(api.O_CYLINDER, minimum=-1.0, maximum=1.0, closed=1, material=mat[3]))])])
    world = b.world(rl, [scopes, b.xf(T(1.4, 0, 0.2) @ S(0.7, 0.7, 0.7), overlapping)], lights=LIGHT)
    o, d = _standard_rays(np.random.default_rng(4300), 300, 150)
    lists = _equal_the_oracle(rl, oracle, world, o, d, "siblings")
    hit_leaf = [l[1][_hit_of(l[0])] for l in lists if _hit_of(l[0]) >= 0]
    for ref in ((api.O_CUBE, 2), (api.O_SPHERE, 3)):  # the siblings that follow a nested EXIT, as the visible hit
        assert sum(h == b.leaf(ref) for h in hit_leaf) >= 10, (ref, len(hit_leaf))
    assert max(len(l[0]) for l in lists) >= 8


def test_bounded_boxes_that_reject(rl, oracle):
    """bounded.rs:100-124: a ray that misses the box never reaches the child.  One box holds only the x < 0 half of its sphere, one
    lies entirely beside its sphere, one cuts a Group of two under a Transformed: rays through what is cut off return nothing, and the
    node_tests (one per box test) of a frame equal the oracle's."""
    rl.init(0)
    api = rl.api
    b = WorldBuilder(api)
    pats = _patterns(b)
    half = b.bounded((-1, -1, -1), (0, 1, 1), b.shape(api.O_SPHERE, material=b.material(pattern=pats[0])))
    beside = b.bounded((2, 2, 2), (2.5, 2.5, 2.5), b.shape(api.O_SPHERE, material=b.material(pattern=pats[1])))
    world = b.world(rl, [half, beside], lights=LIGHT, camera=api.rtc_camera(48, 32, 1.0, (0.5, 1.0, -5.0), (0, 0, 0), (0, 1, 0)))
    rng = np.random.default_rng(4400)
    n_cut = 60  # parallel to y through the x > 0 half: the sphere is there, the boxes are not
    oc = np.stack([rng.uniform(0.05, 0.9, n_cut), np.full(n_cut, -5.0), rng.uniform(-0.4, 0.4, n_cut)], axis=1)
    dc = np.tile([0.0, 1.0, 0.0], (n_cut, 1))
    n_both = 20  # through the box that lies beside its sphere and on into the sphere
    ob = np.array([2.25, 2.25, 2.25]) * 3.0 + rng.uniform(-0.1, 0.1, (n_both, 3))
    db = rng.uniform(-0.15, 0.15, (n_both, 3)) - ob
    o, d = _standard_rays(rng)
    lists = _equal_the_oracle(rl, oracle, world, np.concatenate([oc, o, ob]), np.concatenate([dc, d, db]), "bounded")
    assert all(len(l[0]) == 0 for l in lists[:n_cut])
    assert (oc[:, 0] ** 2 + oc[:, 2] ** 2 < 1).all()  # each of them crosses the sphere itself
    assert sum(len(l[0]) == 2 for l in lists[n_cut:-n_both]) >= 40 and sum(len(l[0]) == 4 for l in lists[-n_both:]) >= 10
    gs, cs = {}, {}
    img = world.render(1, stats=gs)
    cpu = oracle.rtc_render(world.desc, world.camera, aa=1, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    assert gs["node_tests"] >= 2 * 48 * 32
    assert (np.abs(img - cpu) <= REL * np.maximum(1.0, np.abs(cpu))).all() and img.max() > 0.2
    # a box whose skip spans several ops, inside a scope: the ops after it must still run
    b = WorldBuilder(api)
    pair = b.group([b.shape(api.O_CUBE), b.xf(T(0, 1.5, 0), b.shape(api.O_SPHERE))])
    cut = b.xf(_link(3), b.group([b.bounded((-1, -1, -1), (1, 0, 1), pair), b.xf(T(2.2, 0, 0), b.shape(api.O_CYLINDER, minimum=-1.0, maximum=1.0, closed=1))]))
    world = b.world(rl, [cut, b.xf(T(-2.2, 0, 0), b.shape(api.O_CONE, minimum=-1.0, maximum=0.0, closed=1))], lights=LIGHT)
    o, d = rays_at_origin_region(rng, 500, extent=2.5)
    lists = _equal_the_oracle(rl, oracle, world, o, d, "bounded group")
    per_leaf = [sum((l[1] == leaf).any() for l in lists) for leaf in range(4)]
    assert min(per_leaf) >= 10, per_leaf


# ----------------------------------------------------------------------------- CSG
@pytest.mark.parametrize("first", [0, 6, 12, 18])
def test_random_csg_trees_equal_the_oracle(rl, oracle, first):
    """The worlds of the CPU tier's membership test, six per case, 200 rays each."""
    rl.init(0)
    hit = 0
    for w in range(first, first + 6):
        world, inside, rng = random_csg_world(rl, 1000 + w, lights=LIGHT)
        o, d = rays_at_origin_region(rng, 200)
        lists = _equal_the_oracle(rl, oracle, world, o, d, f"tree{w}", inside=inside)
        hit += sum(len(l[0]) > 0 for l in lists)
    assert hit >= 100, hit  # of 1200: the share over all trees is the CPU tier's to assert


def _octahedron(b, r, material=0):
    """eight smooth triangles, outward vertex normals: one ROP_TRIS range long enough for the kernel's guard tree"""
    refs = []
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                p = [np.array([sx * r, 0, 0.0]), np.array([0, sy * r, 0.0]), np.array([0, 0, sz * r])]
                refs.append(b.triangle(p[0], p[1], p[2], normals=[v / r for v in p], material=material))
    return b.group(refs), (lambda p: np.abs(p).sum(-1) < r)


def _directed_csg(rl, name):
    """-> (world, inside or None, extent of the region the rays are aimed at)"""
    api = rl.api
    U, I, D = api.CSG_UNION, api.CSG_INTERSECTION, api.CSG_DIFFERENCE
    b = WorldBuilder(api)
    solid = lambda which, m: transformed_solid(b, m, *closed_solid(b, which))
    if name == "group as left child":  # two disjoint spheres, the farther one first, minus a bar through both
        s1, f1 = solid(0, T(1.1, 0, 0))
        s2, f2 = solid(0, T(-1.1, 0.2, 0))
        bar, fb = solid(1, S(1.6, 0.4, 0.5))
        return b.world(rl, [b.csg(D, b.group([s1, s2]), bar)], lights=LIGHT), csg_predicate(D, lambda p: f1(p) | f2(p), fb), 1.5
    if name == "bounded as right child":  # the box is the moved cube's own
        s, fs = solid(0, np.eye(4))
        c, fc = solid(1, T(0.5, 0.5, 0))
        return b.world(rl, [b.csg(I, s, b.bounded((-0.5, -0.5, -1), (1.5, 1.5, 1), c))], lights=LIGHT), csg_predicate(I, fs, fc), 1.2
    if name == "smooth mesh as a child":
        c, fc = solid(1, S(0.8, 0.8, 0.8))
        mesh, fm = _octahedron(b, 1.25)
        assert len(b.tris) >= 8
        return b.world(rl, [b.csg(D, c, mesh)], lights=LIGHT), csg_predicate(D, fc, fm), 1.2
    if name == "sibling csgs":  # as two world objects and as the two children of a third: csg_start / csg_mid of a finished scope
        a1, g1 = solid(0, T(-2.4, 0, 0))
        a2, g2 = solid(1, T(-2.0, 0.4, 0.3) @ S(0.6, 0.6, 0.6))
        c1, h1 = solid(2, T(1.0, 0, 0))
        c2, h2 = solid(0, T(1.5, 0.3, 0))
        c3, h3 = solid(4, T(1.6, 0, 0.2) @ R(2, 0.5))
        c4, h4 = solid(1, T(1.9, 0, 0) @ S(0.7, 0.7, 0.7))
        left, fl = b.csg(D, a1, a2), csg_predicate(D, g1, g2)
        right, fr = b.csg(U, b.csg(D, c1, c2), b.csg(I, c3, c4)), csg_predicate(U, csg_predicate(D, h1, h2), csg_predicate(I, h3, h4))
        return b.world(rl, [left, right], lights=LIGHT), (lambda p: fl(p) | fr(p)), 3.0  # the two are disjoint: x < -1 and x > -0.1
    if name == "csg under non-uniform scale":
        s, fs = solid(0, np.eye(4))
        c, fc = solid(2, T(0.5, 0, 0) @ R(0, 1.0) @ S(0.5, 1.5, 0.5))
        node, f = transformed_solid(b, T(0.2, -0.1, 0) @ R(1, 0.6) @ S(1.8, 0.5, 1.1), b.csg(D, s, c), csg_predicate(D, fs, fc))
        return b.world(rl, [node], lights=LIGHT), f, 1.8
    assert name == "depth 4, another operation at each level"
    node, f = solid(0, np.eye(4))
    for level, (op, which, m) in enumerate([(U, 1, T(0.6, 0, 0) @ S(0.6, 0.6, 0.6)), (D, 2, T(0, 0.3, 0) @ R(2, 1.2) @ S(0.4, 1.6, 0.4)),
                                            (I, 1, T(0.2, 0, 0) @ R(1, 0.5) @ S(1.0, 0.8, 1.0)), (D, 0, T(-0.5, 0.2, -0.4) @ S(0.6, 0.6, 0.6))]):
        other, fo = solid(which, m)
        node, f = (b.csg(op, other, node), csg_predicate(op, fo, f)) if level == 2 else (b.csg(op, node, other), csg_predicate(op, f, fo))  # the nest goes down the right side once
    return b.world(rl, [node], lights=LIGHT), f, 1.1


@pytest.mark.parametrize("name", ["group as left child", "bounded as right child", "smooth mesh as a child", "sibling csgs", "csg under non-uniform scale",
                                  "depth 4, another operation at each level"])
def test_directed_csg_trees_equal_the_oracle(rl, oracle, name):
    rl.init(0)
    world, inside, extent = _directed_csg(rl, name)
    rng = np.random.default_rng(4500 + len(name))
    o, d = rays_at_origin_region(rng, 300, extent=extent)
    lists = _equal_the_oracle(rl, oracle, world, o, d, name, inside=inside)
    skipped = 0
    for i, (ts, _, _) in enumerate(lists):  # the oracle's own lists against the membership reference, on these trees too
        bad = membership_disagreement(ts, o[i], d[i], inside)
        skipped += bad == "skip"
        assert bad in (None, "skip"), (name, i, bad)
    assert skipped <= 6, skipped
    counts = [len(l[0]) for l in lists]
    print(name, "rays with 2 or more intersections", sum(c >= 2 for c in counts), "with 4 or more", sum(c >= 4 for c in counts), "longest list", max(counts))
    assert sum(c >= 2 for c in counts) >= 75, name
    assert name == "bounded as right child" or sum(c >= 4 for c in counts) >= 10, name  # that one is convex: a sphere and a cube intersected


# ----------------------------------------------------------------------------- limits
def _nested_csg(rl, depth):
    api = rl.api
    b = WorldBuilder(api)
    node = b.shape(api.O_SPHERE)
    for i in range(depth):
        node = b.csg((api.CSG_UNION, api.CSG_DIFFERENCE, api.CSG_INTERSECTION)[i % 3], node, b.xf(T(0.3 * (i + 1), 0.1 * i, 0), b.shape(api.O_CUBE if i % 2 else api.O_SPHERE)))
    return b.world(rl, [node], lights=LIGHT)


def _nested_transformed(rl, depth):
    b = WorldBuilder(rl.api)
    return b.world(rl, [_chain(b, depth, b.shape(rl.api.O_CUBE))], lights=LIGHT)


@pytest.mark.parametrize("build, accepted, message", [(_nested_csg, 4, "CSG nesting deeper than 4"), (_nested_transformed, 8, "Transformed nesting deeper than 8")])
def test_nesting_limits_are_loud_and_the_deepest_accepted_worlds_equal_the_oracle(rl, oracle, build, accepted, message):
    rl.init(0)
    o, d = rays_at_origin_region(np.random.default_rng(4600 + accepted), 120)
    lists = _equal_the_oracle(rl, oracle, build(rl, accepted), o, d, message)
    assert sum(len(l[0]) > 0 for l in lists) >= 40
    with pytest.raises(rl.api.RLError) as e:
        build(rl, accepted + 1).intersect_rays(o, d, k=K)
    assert message in str(e.value), str(e.value)


# ----------------------------------------------------------------------------- shading
def _shading_world(rl, pattern_kind):
    """One pattern kind on every patterned surface, each with a transform of its own, on shapes that straddle the origin under
    Transformed chains; glass (ior 1.5) around glass (ior 1.3) as the left child of a CSG difference; a reflective floor; two lights."""
    api = rl.api
    b = WorldBuilder(api)
    colors = [((1, 1, 1), (0.1, 0.2, 0.6)), ((0.9, 0.3, 0.1), (0.1, 0.8, 0.3)), ((0.2, 0.3, 0.9), (1, 0.9, 0.2))]
    mats = [T(0.1, 0.2, 0.3) @ R(1, 0.5) @ S(0.4, 0.3, 0.5), R(2, 0.7) @ S(0.25, 0.6, 0.5), T(0.2, 0, -0.1) @ S(0.3, 0.3, 0.3)]
    pm = [b.material(pattern=b.pattern(pattern_kind, ca, cb, m), reflectivity=r) for (ca, cb), m, r in zip(colors, mats, (0.3, 0.0, 0.0))]
    outer = b.shape(api.O_SPHERE, material=b.material((0.9, 0.95, 1.0), diffuse=0.1, ambient=0.05, transparency=0.9, reflectivity=0.1, refractive_index=1.5))
    inner = b.shape(api.O_SPHERE, material=b.material((1.0, 0.9, 0.9), diffuse=0.1, ambient=0.05, transparency=0.9, refractive_index=1.3))
    notch = b.xf(T(0.9, 0.9, -0.9) @ S(0.5, 0.5, 0.5), b.shape(api.O_CUBE, material=b.material((0.9, 0.2, 0.2))))
    glass = b.xf(T(0, 0.2, 0), b.csg(api.CSG_DIFFERENCE, b.group([outer, b.xf(S(0.5, 0.5, 0.5), inner)]), notch))
    floor = b.xf(T(0, -1.5, 0), b.shape(api.O_PLANE, material=pm[0]))
    cube = b.xf(T(-2.0, 0, 0.8), _chain(b, 2, b.shape(api.O_CUBE, material=pm[1])))
    cyl = b.xf(T(2.0, 0, 0.8) @ R(0, 0.5), b.xf(S(0.7, 1.2, 0.7), b.shape(api.O_CYLINDER, minimum=-1.0, maximum=1.0, closed=1, material=pm[2])))
    lights = [((-5.0, 8.0, -8.0), (0.7, 0.7, 0.7)), ((6.0, 5.0, -4.0), (0.4, 0.4, 0.3))]
    cam = api.rtc_camera(48, 32, 1.0, (0.3, 1.2, -6.0), (0, 0, 0), (0, 1, 0))
    world = b.world(rl, [floor, glass, cube, cyl], lights=lights, camera=cam, max_reflection_depth=4, void_color=(0.05, 0.05, 0.1))
    return world, b.leaf(outer), b.leaf(inner)


@pytest.mark.parametrize("pattern_name", ["PAT_STRIPE", "PAT_RING", "PAT_GRADIENT", "PAT_CHECKER3D"])
def test_shading_of_patterns_and_nested_glass_equals_the_oracle(rl, oracle, pattern_name):
    rl.init(0)
    world, outer, inner = _shading_world(rl, getattr(rl.api, pattern_name))
    rng = np.random.default_rng(4700)
    eye = np.array([0.3, 1.2, -6.0])
    n_glass, n_scene = 250, 250
    aim = np.concatenate([rng.uniform(-0.6, 0.6, (n_glass, 3)) + (0, 0.2, 0), rng.uniform(-3.0, 3.0, (n_scene, 3)) * (1, 0.5, 0.5)])
    o1, d1 = np.tile(eye, (n_glass + n_scene, 1)), aim - eye
    d1 /= np.linalg.norm(d1, axis=1, keepdims=True)
    o2, d2 = _inside_rays(rng, 100, extent=2.5)
    o, d = np.concatenate([o1, o2]), np.concatenate([d1, d2])
    assert o.shape[0] == 600
    lists = _equal_the_oracle(rl, oracle, world, o, d, pattern_name)
    through_both = 0  # the hit is the outer glass from outside and the ray refracted there (world.rs:138-159, 1 -> 1.5) meets the inner glass next
    for i, (ts, objs, normals) in enumerate(lists[:n_glass + n_scene]):  # unit directions
        h = _hit_of(ts)
        if h < 0 or objs[h] != outer or (objs[:h] == outer).any():
            continue
        eye, nv = -d[i], normals[h]
        if nv @ eye < 0.0:
            nv = -nv
        ratio, cos_i = 1.0 / 1.5, float(nv @ eye)
        cos_t = math.sqrt(1.0 - ratio * ratio * (1.0 - cos_i * cos_i))
        ts2, objs2, _ = oracle.rtc_intersect(world.desc, o[i] + d[i] * ts[h] - nv * 1e-5, nv * (ratio * cos_i - cos_t) - eye * ratio)
        h2 = _hit_of(ts2)
        through_both += h2 >= 0 and objs2[h2] == inner
    assert through_both >= 50, through_both
    gs, cs = {}, {}
    img = world.render(2, stats=gs)
    cpu = oracle.rtc_render(world.desc, world.camera, aa=2, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    assert gs["flagged"] == 0 and gs["rays"] > 3 * 48 * 32 * 4
    assert (np.abs(img - cpu) <= REL * np.maximum(1.0, np.abs(cpu))).all(), np.abs(img - cpu).max()
    assert img.std() > 0.05
