"""GPU tier: the batched ray queries (World.hit_rays, RtcWorld.intersect_rays / color_at_rays; include/rl_render.h rl_*_rays*).

  * the reference's unit known-answers (the ray cases of tests/test_known_answers.py and tests/test_known_answers_rtc_shapes.py, tables
    copied here) executed ON THE DEVICE, asserting the same values;
  * random rays (camera-like, from inside the scene, axis-parallel, far origins) against the oracle's probes, ray by ray: hit / miss,
    material, object, front_face, counts and hit index EQUAL, t / p / normal bit-equal (+, -, *, /, sqrt without contraction on both
    sides), u / v and RTC colours (libm: atan2, acos, pow) within the 1e-9 relative bar of tests/test_gpu_parity.py;
  * argument errors, media scenes, n = 0, the device-pointer forms on a non-default stream, a degenerate ray inside a batch, a query
    between two renders, the C++ mirror.

The oracle's per-ray probes return no counters, so of the seven counters only `rays` (= the batch size) and `flagged` are asserted
for hit / intersect; for color_at all seven are compared with the counting render of the same primary rays (whose counters the
existing parity tests compare with the oracle's)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INF = float("inf")
SQ2 = math.sqrt(2.0)
REL = 1e-9  # tests/test_gpu_parity.py: colour-only (libm) quantities


def _norm(v):  # Vec3d::norm (math/vector.rs:32-43)
    x, y, z = (float(c) for c in v)
    m = math.sqrt(x * x + y * y + z * z)
    return (x / m, y / m, z / m)


def _rays(cases):
    return np.array([c[0] for c in cases], dtype=np.float64), np.array([c[1] for c in cases], dtype=np.float64)


# ----------------------------------------------------------------------------- RTIOW known answers (sphere.rs:118-179, hittable/mod.rs:226-250)
def _sphere_world(rl, spheres, use_bvh=False, n_mats=1):
    api = rl.api
    tex = np.zeros(1, dtype=api.TEXTURE)
    mats = np.zeros(n_mats, dtype=api.MATERIAL)  # Flat
    sph = np.zeros(len(spheres), dtype=api.SPHERE)
    for i, s in enumerate(spheres):
        sph[i]["center0"], sph[i]["radius"] = s[0], s[1]
        sph[i]["material"] = s[2] if len(s) > 2 else 0
    return rl.World.from_spheres(sph, mats, tex, use_bvh)


def test_sphere_hit_known_answers_on_the_device(rl):
    rl.init(0)
    w = _sphere_world(rl, [((0, 0, 0), 1.0)])
    o, d = _rays([((0, 2, 5), (0, 0, -1)), ((0, 1, 5), (0, 0, -1)), ((0, 0, 5), (0, 0, -1)), ((0, 0, 0), (0, 0, -1))])
    st = {}
    h = w.hit_rays(o, d, tmin=0.0, tmax=INF, stats=st)
    assert st["rays"] == 4 and st["flagged"] == 0 and st["sphere_tests"] == 4
    assert h["hit"][0] == 0 and h["t"][0] == INF and not h["p"][0].any() and not h["normal"][0].any() and h["material"][0] == 0  # misses
    assert h["hit"][1] == 1 and h["t"][1] == 5.0 and h["front_face"][1] == 1 and np.allclose(h["normal"][1], (0, 1, 0))  # tangent
    assert h["hit"][2] == 1 and h["t"][2] == 4.0 and h["front_face"][2] == 1 and np.allclose(h["normal"][2], (0, 0, 1))  # through
    assert tuple(h["p"][2]) == (0.0, 0.0, 1.0)
    assert h["hit"][3] == 1 and h["t"][3] == 1.0 and h["front_face"][3] == 0 and np.allclose(h["normal"][3], (0, 0, 1))  # from inside
    o1, d1 = _rays([((0, 0, 5), (0, 0, -1))])
    assert w.hit_rays(o1, d1, tmin=0.0, tmax=1.0)["hit"][0] == 0
    h = w.hit_rays(o1, d1, tmin=0.0, tmax=4.0)  # the interval is closed
    assert h["hit"][0] == 1 and h["t"][0] == 4.0
    h = w.hit_rays(o1, d1, tmin=4.0, tmax=4.0)
    assert h["hit"][0] == 1 and h["t"][0] == 4.0
    assert w.hit_rays(o1, d1, tmin=6.5, tmax=INF)["hit"][0] == 0


def test_slice_and_bvh_return_closest_of_three_and_later_wins_ties(rl):
    rl.init(0)
    o, d = _rays([((0, 0, 5), (0, 0, -1))])
    three = [((0, 0, -10), 1.0), ((0, 0, 0), 1.0), ((0, 0, -5), 1.0)]
    assert _sphere_world(rl, three).hit_rays(o, d)["t"][0] == 4.0
    assert _sphere_world(rl, three, use_bvh=True).hit_rays(o, d)["t"][0] == 4.0
    # two coincident spheres: the fold replaces on t <= closest, so the LATER one is reported (hittable/mod.rs:90-105)
    w = _sphere_world(rl, [((0, 0, 0), 1.0, 0), ((0, 0, 0), 1.0, 1)], n_mats=2)
    h = w.hit_rays(o, d)
    assert h["hit"][0] == 1 and h["material"][0] == 1
    # the counters of the counting kernel, by hand: a slice tests every sphere for every ray and has no boxes (hittable/mod.rs:88-111)
    rng = np.random.default_rng(1)
    ro, rd = rng.uniform(-12, 12, size=(777, 3)), rng.normal(size=(777, 3))
    st = {}
    _sphere_world(rl, three).hit_rays(ro, rd, stats=st)
    assert (st["rays"], st["sphere_tests"], st["node_tests"], st["planar_tests"], st["instance_enters"], st["rng_words"]) == (777, 3 * 777, 0, 0, 0, 0)


def test_sphere_hit_record_carries_uv_on_the_device(rl):  # sphere.rs:70
    rl.init(0)
    world = rl.World.build(lambda b: b.sphere((0, 0, 0), 2.0, b.lambertian(b.solid((1, 1, 1)))))
    o, d = _rays([((0, 0, 12), (0, 0, -1)), ((12, 0, 0), (-1, 0, 0)), ((0, 12, 0), (0, -1, 0))])
    h = world.hit_rays(o, d, tmin=1e-10, tmax=INF)
    assert h["hit"].all() and np.abs(h["t"] - 10.0).max() < 1e-12
    assert abs(h["u"][0] - 0.25) < 1e-12 and abs(h["v"][0] - 0.5) < 1e-12  # the +z pole of get_sphere_uv
    assert abs(h["u"][1] - 0.5) <= 0.01 and abs(h["v"][1] - 0.5) <= 0.01    # sphere.rs:198-205 table
    assert abs(h["u"][2] - 0.5) <= 0.01 and abs(h["v"][2] - 1.0) <= 0.01


# ----------------------------------------------------------------------------- RTC known answers
def _material(api, **kw):
    m = np.zeros(1, dtype=api.RTC_MATERIAL)
    m["color"], m["ambient"], m["diffuse"], m["specular"], m["shininess"], m["refractive_index"] = (1, 1, 1), 0.1, 0.9, 0.9, 200.0, 1.0
    for k, v in kw.items():
        m[k] = v
    return m[0]


def _shape_world(rl, kind, minimum=None, maximum=None, closed=False):
    api = rl.api
    sh = np.zeros(1, dtype=api.RTC_SHAPE)
    sh["kind"], sh["material"], sh["closed"] = kind, 0, 1 if closed else 0
    if minimum is not None:
        sh["has_minimum"], sh["minimum"] = 1, minimum
    if maximum is not None:
        sh["has_maximum"], sh["maximum"] = 1, maximum
    objs = np.zeros(1, dtype=api.HREF)
    objs["kind"], objs["index"] = kind, 0
    mats = np.array([_material(api)], dtype=api.RTC_MATERIAL)
    return rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), mats, objs, np.zeros(0, dtype=api.RTC_LIGHT), shapes=sh)


def _batch(world, cases, normalise=False):
    """All cases of one scene in ONE batch -> per case (list of t, normals[count, 3])."""
    o = np.array([c[0] for c in cases], dtype=np.float64)
    d = np.array([(_norm(c[1]) if normalise else c[1]) for c in cases], dtype=np.float64)
    counts, isects, hit_index = world.intersect_rays(o, d, k=8)
    return [([float(t) for t in isects["t"][i, :counts[i]]], isects["normal"][i, :counts[i]]) for i in range(len(cases))], hit_index


def test_rtc_sphere_and_plane_known_answers_on_the_device(rl):
    rl.init(0)
    w = _shape_world(rl, rl.api.O_SPHERE)
    t3 = math.sqrt(3.0) / 3.0
    cases = [((0, 0, -5), (0, 0, 1)), ((0, 1, -5), (0, 0, 1)), ((0, 2, -5), (0, 0, 1)), ((0, 0, 0), (0, 0, 1)), ((0, 0, 5), (0, 0, 1)),
             ((5, 0, 0), (-1, 0, 0)), ((0, 5, 0), (0, -1, 0)), ((0, 0, 5), (0, 0, -1)), ((5 * t3, 5 * t3, 5 * t3), (-t3, -t3, -t3))]
    r, hi = _batch(w, cases)
    assert [x[0] for x in r[:5]] == [[4.0, 6.0], [5.0, 5.0], [], [-1.0, 1.0], [-6.0, -4.0]]
    assert list(hi[:5]) == [0, 1, rl.api.NO_HIT, 1, rl.api.NO_HIT]  # hit(): lowest t >= 0, later wins ties
    for i, n in ((5, (1, 0, 0)), (6, (0, 1, 0)), (7, (0, 0, 1))):
        assert np.allclose(r[i][1][0], n, atol=1e-15)
    assert np.allclose(r[8][1][0], (t3, t3, t3), atol=1e-12) and abs(np.linalg.norm(r[8][1][0]) - 1.0) < 1e-15
    w = _shape_world(rl, rl.api.O_PLANE)
    r, _ = _batch(w, [((0, 10, 0), (0, 0, 1)), ((0, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, -1, 0)), ((0, -1, 0), (0, 1, 0)), ((10, 1, -10), (0, -1, 0))])
    assert [x[0] for x in r[:4]] == [[], [], [1.0], [1.0]]
    assert tuple(r[4][1][0]) == (0.0, 1.0, 0.0)


CUBE_T = [((5, 0.5, 0), (-1, 0, 0), [4.0, 6.0]), ((-5, 0.5, 0), (1, 0, 0), [4.0, 6.0]), ((0.5, 5, 0), (0, -1, 0), [4.0, 6.0]),
          ((0.5, -5, 0), (0, 1, 0), [4.0, 6.0]), ((0.5, 0, 5), (0, 0, -1), [4.0, 6.0]), ((0.5, 0, -5), (0, 0, 1), [4.0, 6.0]),
          ((0, 0.5, 0), (0, 0, 1), [-1.0, 1.0]),
          ((-2, 0, 0), (0.2673, 0.5345, 0.8018), []), ((0, -2, 0), (0.8018, 0.2673, 0.5345), []), ((0, 0, -2), (0.5345, 0.8018, 0.2673), []),
          ((2, 0, 2), (0, 0, -1), []), ((0, 2, 2), (0, -1, 0), []), ((2, 2, 0), (-1, 0, 0), [])]
CUBE_N = [((5, 0.5, -0.8), (-1, 0, 0), (1, 0, 0)), ((-5, -0.2, 0.9), (1, 0, 0), (-1, 0, 0)), ((-0.4, 5, -0.1), (0, -1, 0), (0, 1, 0)),
          ((0.3, -5, -0.7), (0, 1, 0), (0, -1, 0)), ((-0.6, 0.3, 5), (0, 0, -1), (0, 0, 1)), ((0.4, 0.4, -5), (0, 0, 1), (0, 0, -1))]


def test_rtc_cube_known_answers_on_the_device(rl):
    rl.init(0)
    r, _ = _batch(_shape_world(rl, rl.api.O_CUBE), CUBE_T + CUBE_N)
    for i, c in enumerate(CUBE_T):
        assert r[i][0] == c[2], (c, r[i][0])
    for i, c in enumerate(CUBE_N):
        assert tuple(r[len(CUBE_T) + i][1][0]) == tuple(float(x) for x in c[2]), c


CYL_T = [((1, 0, 0), (0, 1, 0), []), ((0, 0, 0), (0, 1, 0), []), ((0, 0, -5), (1, 1, 1), []),
         ((1, 0, -5), (0, 0, 1), [5.0, 5.0]), ((0, 0, -5), (0, 0, 1), [4.0, 6.0]), ((0.5, 0, -5), (0.1, 1, 1), [6.80798191702732, 7.088723439378861])]
CYL_TRUNC = [((0, 1.5, 0), (0.1, 1, 0), 0), ((0, 3, -5), (0, 0, 1), 0), ((0, 0, -5), (0, 0, 1), 0),
             ((0, 2, -5), (0, 0, 1), 0), ((0, 1, -5), (0, 0, 1), 0), ((0, 1.5, -2), (0, 0, 1), 2)]
CYL_CAP = [((0, 3, 0), (0, -1, 0), 2), ((0, 3, -2), (0, -1, 2), 2), ((0, 4, -2), (0, -1, 1), 2), ((0, 0, -2), (0, 1, 2), 2), ((0, -1, -2), (0, 1, 1), 2)]
CYL_N = [((5, 0, 0), (-1, 0, 0), (1, 0, 0)), ((0, 5, -5), (0, 0, 1), (0, 0, -1)), ((0, -2, 5), (0, 0, -1), (0, 0, 1)), ((-5, 1, 0), (1, 0, 0), (-1, 0, 0))]


def test_rtc_cylinder_known_answers_on_the_device(rl):
    rl.init(0)
    api = rl.api
    r, _ = _batch(_shape_world(rl, api.O_CYLINDER), CYL_T, normalise=True)
    for i, c in enumerate(CYL_T):
        assert r[i][0] == c[2], (c, r[i][0])
    r, _ = _batch(_shape_world(rl, api.O_CYLINDER), CYL_N)
    for i, c in enumerate(CYL_N):
        assert tuple(r[i][1][0]) == tuple(float(x) for x in c[2]), c
    r, _ = _batch(_shape_world(rl, api.O_CYLINDER, 1.0, 2.0), CYL_TRUNC, normalise=True)
    assert [len(x[0]) for x in r] == [c[2] for c in CYL_TRUNC]
    r, _ = _batch(_shape_world(rl, api.O_CYLINDER, 1.0, 2.0, closed=True), CYL_CAP + [((0.5, 5, 0), (0, -1, 0), 2)], normalise=True)
    assert [len(x[0]) for x in r[:len(CYL_CAP)]] == [c[2] for c in CYL_CAP]
    assert tuple(r[-1][1][0]) == (0.0, 1.0, 0.0) and tuple(r[-1][1][1]) == (0.0, -1.0, 0.0)  # cap normals point along +y / -y


CONE_T = [((0, 1e-6, -5), (0, 0, 1), [4.999999000844085, 5.000000999155915]), ((0, 0, -5), (1, 1, 1), [8.660254037844386, 8.660254037844386]),
          ((1, 1, -5), (-0.5, -1, 1), [4.550055679356349, 49.449944320643645]), ((0, 0, -1), (0, 1, 1), [0.3535533905932738])]
CONE_CAP = [((0, 0, -5), (0, 1, 0), 0), ((0, 0, -0.25), (0, 1, 1), 2), ((0, 0, -0.25), (0, 1, 0), 4)]


def test_rtc_cone_known_answers_on_the_device(rl):
    rl.init(0)
    api = rl.api
    r, _ = _batch(_shape_world(rl, api.O_CONE), CONE_T + [((-5, -1, 0), (1, 0, 0), None)], normalise=True)
    for i, c in enumerate(CONE_T):
        assert r[i][0] == c[2], (c, r[i][0])
    assert np.allclose(r[-1][1][0], _norm((-1, 1, 0)), atol=1e-15)
    r, _ = _batch(_shape_world(rl, api.O_CONE, -0.5, 0.5, closed=True), CONE_CAP, normalise=True)
    assert [len(x[0]) for x in r] == [c[2] for c in CONE_CAP]


def _csg_world(rl, op, right_kind, right_translate_z=None):
    api = rl.api
    sh = np.zeros(2, dtype=api.RTC_SHAPE)
    sh["kind"], sh["material"] = [api.O_SPHERE, right_kind], [0, 0]
    tr = np.zeros(0, dtype=api.RTC_TRANSFORMED)
    right = (right_kind, 1)
    if right_translate_z is not None:
        T = np.eye(4)
        T[2, 3] = right_translate_z
        tr = np.array([api.rtc_transformed(T, right_kind, 1)], dtype=api.RTC_TRANSFORMED)
        right = (api.O_TRANSFORMED, 0)
    csg = np.zeros(1, dtype=api.RTC_CSG)
    csg["operation"] = op
    csg["left"]["kind"], csg["left"]["index"] = api.O_SPHERE, 0
    csg["right"]["kind"], csg["right"]["index"] = right
    objs = np.zeros(1, dtype=api.HREF)
    objs["kind"], objs["index"] = api.O_CSG, 0
    mats = np.array([_material(api)], dtype=api.RTC_MATERIAL)
    return rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), mats, objs, np.zeros(0, dtype=api.RTC_LIGHT), shapes=sh, csgs=csg, transformeds=tr)


def test_rtc_csg_known_answers_on_the_device(rl):
    rl.init(0)
    api = rl.api
    ts = lambda w, o, d: _batch(w, [(o, d)])[0][0][0]
    assert ts(_csg_world(rl, api.CSG_UNION, api.O_CUBE), (0, 2, -5), (0, 0, 1)) == []
    assert ts(_csg_world(rl, api.CSG_UNION, api.O_SPHERE, 0.5), (0, 0, -5), (0, 0, 1)) == [4.0, 6.5]
    assert ts(_csg_world(rl, api.CSG_INTERSECTION, api.O_SPHERE, 0.5), (0, 0, -5), (0, 0, 1)) == [4.5, 6.0]
    assert ts(_csg_world(rl, api.CSG_DIFFERENCE, api.O_SPHERE, 0.5), (0, 0, -5), (0, 0, 1)) == [4.0, 4.5]


def _basic_world(rl, extra_shapes=(), extra_mats=(), extra_tr=(), light=((-10, 10, -10), (1, 1, 1)), s1=None, s2=None, lights=None):
    """World::basic() (world.rs:34-44,173-198): two concentric spheres, one light; plus optional extra transformed shapes."""
    api = rl.api
    mats = [s1 if s1 is not None else _material(api, color=(0.8, 1.0, 0.6), diffuse=0.7, specular=0.2), s2 if s2 is not None else _material(api)] + list(extra_mats)
    sh = np.zeros(2 + len(extra_shapes), dtype=api.RTC_SHAPE)
    sh["kind"][:2], sh["material"][:2] = api.O_SPHERE, [0, 1]
    for i, (kind, mat) in enumerate(extra_shapes):
        sh["kind"][2 + i], sh["material"][2 + i] = kind, mat
    S = np.diag([0.5, 0.5, 0.5, 1.0])
    tr = [api.rtc_transformed(np.eye(4), api.O_SPHERE, 0), api.rtc_transformed(S, api.O_SPHERE, 1)]
    for i, m in enumerate(extra_tr):
        tr.append(api.rtc_transformed(m, extra_shapes[i][0], 2 + i))
    tr = np.array(tr, dtype=api.RTC_TRANSFORMED)
    objs = np.zeros(len(tr), dtype=api.HREF)
    objs["kind"], objs["index"] = api.O_TRANSFORMED, np.arange(len(tr))
    if lights is None:
        lights = [light]
    lt = np.zeros(len(lights), dtype=api.RTC_LIGHT)
    for i, (pos, inten) in enumerate(lights):
        lt["position"][i], lt["intensity"][i] = pos, inten
    return rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), np.array(mats, dtype=api.RTC_MATERIAL), objs, lt, transformeds=tr, shapes=sh)


def _T(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def _close(c, want):
    return np.abs(np.asarray(c) - np.asarray(want)).max() <= 1e-5  # color::test_utils::assert_colors_approx_equal


def _color(world, o, d):
    return world.color_at_rays(np.array([o], dtype=np.float64), np.array([d], dtype=np.float64))[0]


def test_world_color_at_known_answers_on_the_device(rl):
    rl.init(0)
    api = rl.api
    w = _basic_world(rl)
    assert _batch(w, [((0, 0, -5), (0, 0, 1))])[0][0][0] == [4.0, 4.5, 5.5, 6.0]  # intersect_world_with_ray
    c = w.color_at_rays(*_rays([((0, 0, -5), (0, 1, 0)), ((0, 0, -5), (0, 0, 1))]))  # one batch: a miss and a hit
    assert tuple(c[0]) == (0.0, 0.0, 0.0) and _close(c[1], (0.38066, 0.47583, 0.2855))
    inside = _basic_world(rl, light=((0, 0.25, 0), (1, 1, 1)))
    assert _close(_color(inside, (0, 0, 0), (0, 0, 1)), (0.90498, 0.90498, 0.90498))
    dark = _basic_world(rl, lights=[])
    assert tuple(_color(dark, (0, 0, -5), (0, 0, 1))) == (0.0, 0.0, 0.0)
    amb = _basic_world(rl, s1=_material(api, color=(0.8, 1.0, 0.6), diffuse=0.7, specular=0.2, ambient=1.0), s2=_material(api, ambient=1.0))
    assert _close(_color(amb, (0, 0, 0.75), (0, 0, -1)), (1.0, 1.0, 1.0))


def test_world_reflection_and_refraction_known_answers_on_the_device(rl):
    rl.init(0)
    api = rl.api
    ray = ((0, 0, -3), (0, -SQ2 / 2.0, SQ2 / 2.0))
    refl = _basic_world(rl, extra_shapes=[(api.O_PLANE, 2)], extra_mats=[_material(api, reflectivity=0.5)], extra_tr=[_T(0, -1, 0)])
    assert _close(_color(refl, *ray), (0.87675, 0.92434, 0.82917))
    red_ball = _material(api, color=(1, 0, 0), ambient=0.5)
    transp = _basic_world(rl, extra_shapes=[(api.O_PLANE, 2), (api.O_SPHERE, 3)], extra_mats=[_material(api, transparency=0.5, refractive_index=1.5), red_ball],
                          extra_tr=[_T(0, -1, 0), _T(0, -3.5, -0.5)])
    assert _close(_color(transp, *ray), (1.12546, 0.68642, 0.68642))
    both = _basic_world(rl, extra_shapes=[(api.O_PLANE, 2), (api.O_SPHERE, 3)],
                        extra_mats=[_material(api, transparency=0.5, refractive_index=1.5, reflectivity=0.5), red_ball], extra_tr=[_T(0, -1, 0), _T(0, -3.5, -0.5)])
    assert _close(_color(both, *ray), (1.11500, 0.69643, 0.69243))
    sh = np.zeros(2, dtype=api.RTC_SHAPE)
    sh["kind"], sh["material"] = api.O_PLANE, 0
    tr = np.array([api.rtc_transformed(_T(0, -1, 0), api.O_PLANE, 0), api.rtc_transformed(_T(0, 1, 0), api.O_PLANE, 1)], dtype=api.RTC_TRANSFORMED)
    objs = np.zeros(2, dtype=api.HREF)
    objs["kind"], objs["index"] = api.O_TRANSFORMED, [0, 1]
    lt = np.zeros(1, dtype=api.RTC_LIGHT)
    lt["position"], lt["intensity"] = (0, 0, 0), (1, 1, 1)
    mirrors = rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), np.array([_material(api, reflectivity=1.0)], dtype=api.RTC_MATERIAL), objs, lt,
                                      transformeds=tr, shapes=sh)
    assert np.isfinite(_color(mirrors, (0, 0, 0), (0, 1, 0))).all()  # mutually reflective surfaces terminate


# ----------------------------------------------------------------------------- random rays against the oracle
def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


def _random_rays(rng, eye, target, extent, n_cam, n_inside, n_axis, n_far):
    """Camera-like rays from `eye` towards a disc around `target`, rays starting inside the scene's extent, axis-parallel rays, and a
    handful of rays from ~1e6 scene sizes away aimed at the scene."""
    eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
    o, d = [], []
    aim = target + rng.uniform(-extent, extent, size=(n_cam, 3)) * 0.5
    o.append(np.tile(eye, (n_cam, 1))), d.append(aim - eye)
    o.append(target + rng.uniform(-extent, extent, size=(n_inside, 3)) * 0.5), d.append(rng.normal(size=(n_inside, 3)))
    ax = np.zeros((n_axis, 3))
    ax[np.arange(n_axis), rng.integers(0, 3, n_axis)] = rng.choice([-1.0, 1.0], n_axis)
    o.append(target + rng.uniform(-extent, extent, size=(n_axis, 3)) * 0.5), d.append(ax)
    u = rng.normal(size=(n_far, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    far = target + u * extent * 1e6
    o.append(far), d.append((target + rng.uniform(-extent, extent, size=(n_far, 3)) * 0.1) - far)
    return np.concatenate(o), np.concatenate(d)


def _uv_agree(got, want):
    """get_sphere_uv of a far-origin hit can be acos of a value beyond 1: NaN on both sides is agreement."""
    if math.isnan(want) or math.isnan(got):
        return math.isnan(want) and math.isnan(got)
    return abs(got - want) <= REL * max(1.0, abs(want))


def _rtiow_scene(rl, golden, name):
    if name == "golden_test_scene":
        return rl.World.golden_test_scene()
    if name == "bouncing_spheres":
        return rl.World.bouncing_spheres(1)
    if name == "stress60":
        return rl.World.stress_scene(60, 1, golden("spot_triangulated.obj.gz"), _spot_texture())
    return rl.World.example_scene(name)


@pytest.mark.parametrize("name", ["golden_test_scene", "bouncing_spheres", "cornell_box", "quads", "flat_world", "stress60"])
def test_hit_rays_equal_the_oracle_ray_by_ray(rl, oracle, golden, name):
    rl.init(0)
    world = _rtiow_scene(rl, golden, name)
    p = world.params
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    extent = float(np.linalg.norm(target - eye))
    rng = np.random.default_rng(20240 + len(name))
    o, d = _random_rays(rng, eye, target, extent, 1200, 500, 300, 16)
    times = rng.uniform(0.0, 1.0, o.shape[0])  # bouncing_spheres: moving centres (sphere.rs:36)
    for tmin, tmax in ((1e-10, INF), (0.0, 1.0)):  # directions are not normalised: the camera-like rays reach their target at t = 1
        st = {}
        # the far-origin rays may reach Sphere::hit's unit-length check of the outward normal (vec3.rs:219-222 from_normalized, a counted panic site: p is
        # computed 1e6 scene sizes away); the probe returns the record all the same, on both sides
        h = world.hit_rays(o, d, times=times, tmin=tmin, tmax=tmax, stats=st, allow_degenerate=True)
        assert st["rays"] == o.shape[0]
        near = {}
        plain = world.hit_rays(o[:-16], d[:-16], times=times[:-16], tmin=tmin, tmax=tmax, stats=near)  # without them: nothing is flagged, same bits
        assert near["flagged"] == 0 and near["rays"] == o.shape[0] - 16 and h[:-16].tobytes() == plain.tobytes()
        n_hit = 0
        for i in range(o.shape[0]):
            ref = oracle.rtiow_hit(world.desc, o[i], d[i], times[i], tmin, tmax)
            if ref is None:
                assert h["hit"][i] == 0 and h["t"][i] == INF, (name, i)
                continue
            n_hit += 1
            assert h["hit"][i] == 1 and h["material"][i] == ref["mat"] and bool(h["front_face"][i]) == ref["front"], (name, i)
            assert h["t"][i] == ref["t"] and np.array_equal(h["p"][i], ref["p"]) and np.array_equal(h["normal"][i], ref["normal"]), (name, i, h[i], ref)
            assert _uv_agree(h["u"][i], ref["u"]) and _uv_agree(h["v"][i], ref["v"]), (name, i, h[i], ref)
        assert tmax != INF or n_hit > 100, (name, n_hit)  # the rays do meet the scene


def _rtc_scene(rl, golden, name):
    if name == "teapot":
        return rl.RtcWorld.test_obj_scene(golden("teapot-low.obj"), 90, 60)
    return rl.RtcWorld.test_mirror_scene(90, 60) if name == "mirror" else rl.RtcWorld.test_csg_scene(90, 60)


def _rtc_camera_rays(cam):
    """rays_for_pixel (scene/camera.rs:63-91) at one sample per pixel, in the device's order of operations (csrc/rl_rtc_full_kernel.h:
    4-term sums accumulated from 0.0, true division by the magnitude), so that the rays are bit for bit those of an AA 1 render."""
    inv = np.array(list(cam.inverse)).reshape(4, 4)
    px, py = np.meshgrid(np.arange(cam.hsize, dtype=np.float64), np.arange(cam.vsize, dtype=np.float64))
    px, py = px.reshape(-1), py.reshape(-1)
    sample_offset = 1.0 / 1.0
    x = cam.half_width - (px + sample_offset * (0.0 + 0.5)) * cam.pixel_size
    y = cam.half_height - (py + sample_offset * (0.0 + 0.5)) * cam.pixel_size
    z = np.full_like(x, -1.0)

    def mul_point(vx, vy, vz):
        out = []
        for r in range(3):
            acc = 0.0 + inv[r, 0] * vx
            acc = acc + inv[r, 1] * vy
            acc = acc + inv[r, 2] * vz
            acc = acc + inv[r, 3] * 1.0
            out.append(acc)
        return out
    pix = mul_point(x, y, z)
    org = mul_point(np.zeros_like(x), np.zeros_like(x), np.zeros_like(x))
    v = [pix[k] - org[k] for k in range(3)]
    m = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return np.stack(org, axis=1), np.stack([v[0] / m, v[1] / m, v[2] / m], axis=1)


@pytest.mark.parametrize("name", ["teapot", "mirror", "csg"])
def test_rtc_queries_equal_the_oracle_ray_by_ray(rl, oracle, golden, name):
    rl.init(0)
    world = _rtc_scene(rl, golden, name)
    co, cd = _rtc_camera_rays(world.camera)
    rng = np.random.default_rng(77)
    pick = rng.choice(co.shape[0], 700, replace=False)
    eye = co[0]
    ro, rd = _random_rays(rng, eye, eye + cd[co.shape[0] // 2] * 5.0, 6.0, 0, 200, 100, 8)
    o, d = np.concatenate([co[pick], ro]), np.concatenate([cd[pick], rd])
    K = 12
    st = {}
    counts, isects, hit_index = world.intersect_rays(o, d, k=K, stats=st, allow_degenerate=True)
    assert st["rays"] == o.shape[0]
    counts_only, _, hi2 = world.intersect_rays(o, d, k=0, allow_degenerate=True)
    assert np.array_equal(counts, counts_only) and np.array_equal(hit_index, hi2)
    rgb = world.color_at_rays(o, d, allow_degenerate=True)
    n_hit = 0
    for i in range(o.shape[0]):
        ts, objs, normals = oracle.rtc_intersect(world.desc, o[i], d[i], cap=64)
        if len(ts) > 48:
            continue  # beyond the device's list (flagged there, as in the renders)
        assert counts[i] == len(ts), (name, i, counts[i], len(ts))
        m = min(len(ts), K)
        assert np.array_equal(isects["t"][i, :m], ts[:m]) and np.array_equal(isects["object"][i, :m], objs[:m]), (name, i)
        assert np.array_equal(isects["normal"][i, :m], normals[:m]), (name, i)
        want = -1  # intersect.rs:159-168
        for j in range(len(ts)):
            if ts[j] >= 0.0 and (want < 0 or not (ts[want] < ts[j])):
                want = j
        assert hit_index[i] == (rl.api.NO_HIT if want < 0 else want), (name, i)
        n_hit += want >= 0
        ref = oracle.rtc_color_at(world.desc, o[i], d[i])
        assert np.abs(rgb[i] - ref).max() <= REL * max(1.0, np.abs(ref).max()), (name, i, rgb[i], ref)
    assert n_hit > 100, (name, n_hit)


def test_color_at_rays_of_the_camera_rays_is_the_frame_with_its_counters(rl, golden):
    """The per-ray body is shared with rtc_full_kernel (csrc/rl_rtc_color_at_body.inc): the pixel-centre rays of a frame through
    color_at_rays give the AA 1 frame bit for bit (mean of one sample: c * (1 / 1)) and every counter of its counting render."""
    rl.init(0)
    for name in ("mirror", "csg", "teapot"):
        world = _rtc_scene(rl, golden, name)
        fs, qs = {}, {}
        frame = world.render(1, stats=fs)
        o, d = _rtc_camera_rays(world.camera)
        rgb = world.color_at_rays(o, d, stats=qs).reshape(frame.shape)
        assert np.array_equal(rgb, frame), name
        for k in ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged"):
            assert qs[k] == fs[k], (name, k, qs[k], fs[k])


# ----------------------------------------------------------------------------- errors and plumbing
def _media_world(rl):
    def build(b):
        fog = b.isotropic(b.solid((1, 1, 1)))
        return b.list([b.constant_medium(b.sphere((0, 0, 0), 1.0, b.lambertian(b.solid((1, 1, 1)))), 0.5, fog)])
    return rl.World.build(build)


def test_errors_and_empty_batches(rl, golden):
    rl.init(0)
    api = rl.api
    lib = api.render_lib()
    o, d = _rays([((0, 0, 5), (0, 0, -1))])
    with pytest.raises(rl.RLError) as e:
        _media_world(rl).hit_rays(o, d)
    assert e.value.code == api.RL_E_UNSUPPORTED
    world = rl.World.golden_test_scene()
    rw = _rtc_scene(rl, golden, "csg")
    assert world.hit_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)  # n = 0
    assert rw.color_at_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 3)
    assert rw.intersect_rays(np.zeros((0, 3)), np.zeros((0, 3)))[0].shape == (0,)
    assert lib.rl_rtiow_hit_rays(world.device(), None, 0, 1e-10, INF, None, None) == api.RL_OK
    rays = api.pack_rays(o, d)
    hits = np.zeros(1, dtype=api.RTIOW_HIT)
    rgb = np.zeros((1, 3))
    cnt = np.zeros(1, dtype=np.uint32)
    assert lib.rl_rtiow_hit_rays(world.device(), None, 1, 1e-10, INF, hits.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_hit_rays(world.device(), rays.ctypes.data, 1, 1e-10, INF, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_hit_rays(world.device(), rays.ctypes.data, 1, float("nan"), INF, hits.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_hit_rays(world.device(), rays.ctypes.data, 1, 1e-10, float("nan"), hits.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_hit_rays(rw.device(), rays.ctypes.data, 1, 1e-10, INF, hits.ctypes.data, None) == api.RL_E_INVALID  # RTC handle
    assert lib.rl_rtc_color_at_rays(world.device(), rays.ctypes.data, 1, rgb.ctypes.data, None) == api.RL_E_INVALID       # RTIOW handle
    assert lib.rl_rtc_intersect_rays(world.device(), rays.ctypes.data, 1, 0, None, cnt.ctypes.data, None, None) == api.RL_E_INVALID
    assert lib.rl_rtc_intersect_rays(rw.device(), rays.ctypes.data, 1, 0, None, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtc_intersect_rays(rw.device(), rays.ctypes.data, 1, 4, None, cnt.ctypes.data, None, None) == api.RL_E_INVALID
    assert lib.rl_rtc_color_at_rays(rw.device(), rays.ctypes.data, 1, None, None) == api.RL_E_INVALID


def test_device_pointer_forms_on_a_side_stream_then_render_status(rl, golden):
    import torch
    rl.init(0)
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    p = world.params
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    o, d = _random_rays(np.random.default_rng(3), eye, target, float(np.linalg.norm(target - eye)), 3000, 500, 100, 0)
    rays = api.pack_rays(o, d)
    want = world.hit_rays(o, d)
    n = rays.shape[0]
    stream = torch.cuda.Stream()
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 56).copy()).to("cuda:0")
    d_out = torch.zeros((n, 88), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    world.hit_rays_device(d_rays.data_ptr(), d_out.data_ptr(), n, stream=stream.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == n and st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert d_out.cpu().numpy().tobytes() == want.tobytes()
    assert api.render_status(world)["rays"] == 0  # each query counts once
    rw = _rtc_scene(rl, golden, "mirror")
    co, cd = _rtc_camera_rays(rw.camera)
    rrays = api.pack_rays(co, cd)
    m = rrays.shape[0]
    want_rgb = rw.color_at_rays(co, cd)
    want_counts, want_isects, want_hi = rw.intersect_rays(co, cd, k=4)
    d_rr = torch.from_numpy(rrays.view(np.uint8).reshape(m, 56).copy()).to("cuda:0")
    d_rgb = torch.zeros((m, 3), dtype=torch.float64, device="cuda:0")
    d_is = torch.zeros((m, 4, 40), dtype=torch.uint8, device="cuda:0")
    d_cnt = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    d_hi = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    rw.color_at_rays_device(d_rr.data_ptr(), d_rgb.data_ptr(), m, stream=stream.cuda_stream)
    rw.intersect_rays_device(d_rr.data_ptr(), m, 4, d_is.data_ptr(), d_cnt.data_ptr(), d_hi.data_ptr(), stream=stream.cuda_stream)
    st = api.render_status(rw)
    assert st["rays"] == m and st["flagged"] == 0  # rays: of the most recently enqueued query (intersect: the batch)
    assert np.array_equal(d_rgb.cpu().numpy(), want_rgb)
    assert np.array_equal(d_cnt.cpu().numpy().view(np.uint32), want_counts) and np.array_equal(d_hi.cpu().numpy().view(np.uint32), want_hi)
    got_is = d_is.cpu().numpy().reshape(-1).view(api.RTC_ISECT).reshape(m, 4)
    for i in range(m):
        c = min(int(want_counts[i]), 4)
        assert got_is[i, :c].tobytes() == want_isects[i, :c].tobytes()


def _zero_normal_triangle_world(rl):
    """One smooth triangle whose vertex normals (0,0,1), (0,0,-1), (0,0,-1) interpolate to exactly zero at u = v = 0.25: the reference's
    normalisation of the interpolated normal panics there (triangle.rs:95-101), a counted site."""
    api = rl.api
    t = np.zeros(1, dtype=api.RTC_TRIANGLE)
    p1, p2, p3 = np.array([0, 1, 0.0]), np.array([-1, 0, 0.0]), np.array([1, 0, 0.0])
    t["p1"], t["e1"], t["e2"] = p1, p2 - p1, p3 - p1
    t["smooth"], t["n1"], t["n2"], t["n3"] = 1, (0, 0, 1), (0, 0, -1), (0, 0, -1)
    objs = np.zeros(1, dtype=api.HREF)
    objs["kind"], objs["index"] = api.O_TRIANGLE, 0
    return rl.RtcWorld.from_arrays(t, np.array([_material(api)], dtype=api.RTC_MATERIAL), objs, np.zeros(0, dtype=api.RTC_LIGHT))


def test_a_degenerate_ray_in_a_batch_flags_that_ray_only(rl):
    """A ray that reaches a counted panic site: RL_E_DEGENERATE with every output written, flagged == 1, the other rays' records unchanged;
    the asynchronous form reports the same through render_status.  (A zero direction is NOT such a ray: Sphere::hit gets a = 0 and NaN roots,
    the RTC shapes find no intersection, so nothing is hit and no normalisation is reached; checked below.)
    RTIOW: a unit sphere seen from 1e13 radii away: len2(oc) - r^2 rounds to len2(oc), the discriminant is 0, p = o + d * 1e13 = 0, the
    outward normal is the zero vector and NormalizedVec3::from_normalized's unit-length check fails (vec3.rs:219-222)."""
    import torch
    rl.init(0)
    api = rl.api
    w = _sphere_world(rl, [((0, 0, 0), 1.0)])
    o, d = _rays([((0, 0, 5), (0, 0, -1)), ((0, 2, 5), (0, 0, -1)), ((0, 0, 1e13), (0, 0, -1)), ((0.5, 0, 5), (0, 0, -1)), ((0, 0, 0), (0, 0, 0))])
    clean_o, clean_d = np.delete(o, 2, axis=0), np.delete(d, 2, axis=0)
    cst = {}
    clean = w.hit_rays(clean_o, clean_d, stats=cst)  # the zero direction among them: no hit, no flag
    assert cst["flagged"] == 0 and cst["rc"] == api.RL_OK and clean["hit"][3] == 0
    with pytest.raises(rl.RLError) as e:
        w.hit_rays(o, d)
    assert e.value.code == api.RL_E_DEGENERATE
    keep = np.arange(5) != 2
    for stats in ({}, None):  # the counting and the counter-free host form
        st = {} if stats is not None else None
        h = w.hit_rays(o, d, stats=st, allow_degenerate=True)
        assert h[keep].tobytes() == clean.tobytes()
        assert h["hit"][2] == 1 and h["t"][2] == 1e13 and not h["p"][2].any()
        if st is not None:
            assert st["flagged"] == 1 and st["rc"] == api.RL_E_DEGENERATE and st["rays"] == 5
    rays = api.pack_rays(o, d)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(5, 56).copy()).to("cuda:0")
    d_out = torch.zeros((5, 88), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    w.hit_rays_device(d_rays.data_ptr(), d_out.data_ptr(), 5, stream=stream.cuda_stream)
    with pytest.raises(rl.RLError) as e:
        api.render_status(w)
    assert e.value.code == api.RL_E_DEGENERATE
    w.hit_rays_device(d_rays.data_ptr(), d_out.data_ptr(), 5, stream=stream.cuda_stream)
    st = api.render_status(w, allow_degenerate=True)
    assert st["flagged"] == 1 and st["rays"] == 5 and st["rc"] == api.RL_E_DEGENERATE
    assert d_out.cpu().numpy().tobytes() == h.tobytes()
    assert api.render_status(w)["flagged"] == 0  # counted once
    # RTC
    rw = _zero_normal_triangle_world(rl)
    ro, rd = _rays([((0.2, 0.3, -2), (0, 0, 1)), ((0, 0.5, -2), (0, 0, 1)), ((0, 5, -2), (0, 0, 1)), ((0, 0.5, -2), (0, 0, 0))])
    keep = np.arange(4) != 1
    cst = {}
    cc, ci, ch = rw.intersect_rays(ro[keep], rd[keep], k=2, stats=cst)
    assert cst["flagged"] == 0 and list(cc) == [1, 0, 0]
    st = {}
    counts, isects, hi = rw.intersect_rays(ro, rd, k=2, stats=st, allow_degenerate=True)
    assert st["flagged"] == 1 and st["rc"] == api.RL_E_DEGENERATE and st["rays"] == 4
    assert np.array_equal(counts[keep], cc) and isects[keep].tobytes() == ci.tobytes() and np.array_equal(hi[keep], ch)
    assert counts[1] == 1 and isects["t"][1, 0] == 2.0
    st = {}
    rgb = rw.color_at_rays(ro, rd, stats=st, allow_degenerate=True)
    assert st["flagged"] == 1 and st["rc"] == api.RL_E_DEGENERATE and np.array_equal(rgb[keep], rw.color_at_rays(ro[keep], rd[keep]))
    rr = api.pack_rays(ro, rd)
    d_rr = torch.from_numpy(rr.view(np.uint8).reshape(4, 56).copy()).to("cuda:0")
    d_rgb = torch.zeros((4, 3), dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    rw.color_at_rays_device(d_rr.data_ptr(), d_rgb.data_ptr(), 4, stream=stream.cuda_stream)
    st = api.render_status(rw, allow_degenerate=True)
    assert st["flagged"] == 1 and st["rc"] == api.RL_E_DEGENERATE and np.array_equal(d_rgb.cpu().numpy(), rgb)


def test_a_query_between_two_renders_changes_neither_frames_nor_accounting(rl):
    import torch
    rl.init(0)
    api = rl.api
    world = rl.World.golden_test_scene()
    p = world.params
    p.image_width, p.samples_per_pixel = 96, 4
    cam = rl.Camera(p)
    gs = {}
    want = cam.render(world, stats=gs).data
    H, W = cam.c.image_height, cam.c.image_width
    a = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    b = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    o, d = _random_rays(np.random.default_rng(4), eye, target, float(np.linalg.norm(target - eye)), 2000, 0, 0, 0)
    rays = api.pack_rays(o, d)
    n = rays.shape[0]
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 56).copy()).to("cuda:0")
    d_out = torch.zeros((n, 88), dtype=torch.uint8, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    cam.render_device(world, a.data_ptr(), stream=s1.cuda_stream)
    world.hit_rays_device(d_rays.data_ptr(), d_out.data_ptr(), n, stream=s2.cuda_stream)
    cam.render_device(world, b.data_ptr(), stream=s1.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == gs["rays"] and st["flagged"] == 0  # rays: of the most recently enqueued one, the second render
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    assert d_out.cpu().numpy().tobytes() == world.hit_rays(o, d).tobytes()
    assert api.render_status(world)["rays"] == 0


@pytest.mark.skipif(bool(os.environ.get("RL_RENDER_LIB")), reason="the C++ host mirror links librl_render.so (the product library)")
def test_cpp_mirror_probe_agrees_with_the_python_path(rl):
    rl.init(0)
    api = rl.api
    H = api.host_lib()
    H.rlh_ray_query_probe.argtypes = [C.c_int, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_void_p]
    world = rl.World.golden_test_scene()
    p = world.params
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    o, d = _random_rays(np.random.default_rng(11), eye, target, float(np.linalg.norm(target - eye)), 500, 100, 50, 0)
    rays = api.pack_rays(o, d)
    hits = np.zeros(rays.shape[0], dtype=api.RTIOW_HIT)
    assert H.rlh_ray_query_probe(0, rays.ctypes.data, rays.shape[0], 1e-10, INF, hits.ctypes.data) == 0, H.rlh_last_error()
    assert hits.tobytes() == world.hit_rays(o, d).tobytes()
    rw = rl.RtcWorld.test_mirror_scene(60, 40)
    co, cd = _rtc_camera_rays(rw.camera)
    rr = api.pack_rays(co, cd)
    rgb = np.zeros((rr.shape[0], 3))
    assert H.rlh_ray_query_probe(1, rr.ctypes.data, rr.shape[0], 0.0, 0.0, rgb.ctypes.data) == 0, H.rlh_last_error()
    assert np.array_equal(rgb, rw.color_at_rays(co, cd))
    cnt = np.zeros(rr.shape[0], dtype=np.uint32)
    assert H.rlh_ray_query_probe(2, rr.ctypes.data, rr.shape[0], 0.0, 0.0, cnt.ctypes.data) == 0, H.rlh_last_error()
    assert np.array_equal(cnt, rw.intersect_rays(co, cd, k=0)[0])


# ----------------------------------------------------------------------------- fast path
def _frame_rays(rl, world, width):
    """The pixel-centre rays of a frame of the world's own camera (camera.rs:232-262 without the sample offset)."""
    p = world.params
    p.image_width = width
    c = rl.Camera(p).c
    W, H = c.image_width, c.image_height
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    p00, du, dv, eye = (np.array(list(v)) for v in (c.pixel_00, c.pixel_du, c.pixel_dv, c.lookfrom))
    centre = (p00 + x.reshape(-1, 1) * du) + y.reshape(-1, 1) * dv
    return np.tile(eye, (W * H, 1)), centre - eye


@pytest.mark.parametrize("name", ["bouncing_spheres", "stress60", "flat_world"])
def test_fast_path_equals_reference_order_bit_for_bit_and_did_run(rl, oracle, golden, name):
    """>= 1 M rays — the pixel-centre rays of a frame plus their first-bounce continuations (origin = the returned p, mirror direction:
    rays that start ON a surface) — through the counter-free call (fast walk) and the counting call (reference order): same bytes.  Also
    with a finite tmax (half the median hit distance) and with tmin = 0.0, which must take the reference-order kernel and agree with the
    oracle.  The fast kernel must have served the counter-free calls with at most 1 in 20 rays re-traced."""
    rl.init(0)
    api = rl.api
    world = _rtiow_scene(rl, golden, name)
    o, d = _frame_rays(rl, world, 1280)
    first = world.hit_rays(o, d)
    assert api.last_query()["kernel"] == "fast"
    hit = first["hit"] == 1
    n_ = first["normal"][hit]
    dd = d[hit]
    refl = dd - 2.0 * np.sum(dd * n_, axis=1, keepdims=True) * n_
    o2, d2 = np.concatenate([o, first["p"][hit]]), np.concatenate([d, refl])
    assert o2.shape[0] >= 1_000_000, o2.shape
    times = np.random.default_rng(6).uniform(0.0, 1.0, o2.shape[0])
    half = 0.5 * float(np.median(first["t"][hit]))
    for tmax in (INF, half):
        fast = world.hit_rays(o2, d2, times=times, tmax=tmax, allow_degenerate=True)
        q = api.last_query()
        print(name, "tmax", tmax, "rays", o2.shape[0], "re-traced", q["retraced"])
        assert q["kernel"] == "fast" and q["retraced"] * 20 <= o2.shape[0], q
        st = {}
        ref = world.hit_rays(o2, d2, times=times, tmax=tmax, stats=st, allow_degenerate=True)
        assert api.last_query()["kernel"] == "reference" and st["rays"] == o2.shape[0]
        assert np.array_equal(fast.view(np.uint8), ref.view(np.uint8))
    zero = world.hit_rays(o2, d2, times=times, tmin=0.0, allow_degenerate=True)
    assert api.last_query()["kernel"] == "reference"
    for i in np.random.default_rng(8).choice(o2.shape[0], 400, replace=False):
        r = oracle.rtiow_hit(world.desc, o2[i], d2[i], times[i], 0.0, INF)
        assert (r is None) == (zero["hit"][i] == 0), (name, i)
        if r is not None:
            assert zero["t"][i] == r["t"] and np.array_equal(zero["p"][i], r["p"]) and zero["material"][i] == r["mat"], (name, i)
