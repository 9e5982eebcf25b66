"""The RTC shading queries on the device (include/rl_render.h "RTC shading queries"): rl_rtc_prepare_rays (hit +
Intersection::prepare_computations), rl_rtc_shade_hits (World::shade_hit up to its recursion), rl_rtc_shadow_attenuation and
rl_rtc_lighting.

  * the header's loop of prepare_rays + shade_hits gives color_at_rays' colours byte for byte, and its ray count;
  * shade_hits is shadow_attenuation + lighting, light by light;
  * prepare_rays against the CPU oracle's intersection lists, ray by ray, and lighting against the oracle's;
  * the known answers of the reference's own unit tests (world.rs, intersect.rs, material.rs);
  * plumbing: batch sizes, device forms, errors, degenerate elements, the status ring.
"""
import math
import struct

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REL = 1e-9  # tests/test_gpu_parity.py: colour-only (libm) quantities
SQ2 = math.sqrt(2.0)
W, H = 90, 60


# ----------------------------------------------------------------------------- worlds and rays
def _material(api, **kw):
    m = np.zeros(1, dtype=api.RTC_MATERIAL)
    m["color"], m["ambient"], m["diffuse"], m["specular"], m["shininess"], m["refractive_index"] = (1, 1, 1), 0.1, 0.9, 0.9, 200.0, 1.0
    for k, v in kw.items():
        m[k] = v
    return m[0]


def _basic_world(rl, extra_shapes=(), extra_mats=(), extra_tr=(), light=((-10, 10, -10), (1, 1, 1)), s1=None, s2=None, lights=None, depth=5):
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
    return rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), np.array(mats, dtype=api.RTC_MATERIAL), objs, lt, transformeds=tr, shapes=sh,
                                   max_reflection_depth=depth)


def _shapes_world(rl, shapes, lights=(((-10, 10, -10), (1, 1, 1)),)):
    """shapes: (kind, 4x4 transform, material record) -> a world of Transformed shapes, in order."""
    api = rl.api
    sh = np.zeros(len(shapes), dtype=api.RTC_SHAPE)
    sh["kind"], sh["material"] = [s[0] for s in shapes], np.arange(len(shapes))
    tr = np.array([api.rtc_transformed(s[1], s[0], i) for i, s in enumerate(shapes)], dtype=api.RTC_TRANSFORMED)
    objs = np.zeros(len(shapes), dtype=api.HREF)
    objs["kind"], objs["index"] = api.O_TRANSFORMED, np.arange(len(shapes))
    lt = np.zeros(len(lights), dtype=api.RTC_LIGHT)
    for i, (pos, inten) in enumerate(lights):
        lt["position"][i], lt["intensity"][i] = pos, inten
    return rl.RtcWorld.from_arrays(np.zeros(0, dtype=api.RTC_TRIANGLE), np.array([s[2] for s in shapes], dtype=api.RTC_MATERIAL), objs, lt,
                                   transformeds=tr, shapes=sh)


def _T(x, y, z):
    m = np.eye(4)
    m[:3, 3] = (x, y, z)
    return m


def _rays(cases):
    return np.array([c[0] for c in cases], dtype=np.float64), np.array([c[1] for c in cases], dtype=np.float64)


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


GOLDEN_SCENES = ["mirror", "csg", "teapot"]
HAND_SCENES = ["reflective_plane", "schlick_plane", "two_lights"]
RAY = ((0, 0, -3), (0, -SQ2 / 2.0, SQ2 / 2.0))  # world.rs: the ray of the reflection / refraction tests
_SCENES = {}


def _scene(rl, golden, name):
    """-> (world, origins, dirs): the pixel-centre rays of a 90x60 frame; built once per session and left unchanged."""
    if name in _SCENES:
        return _SCENES[name]
    rl.init(0)
    api = rl.api
    if name == "teapot":
        world = rl.RtcWorld.test_obj_scene(golden("teapot-low.obj"), W, H)
    elif name == "mirror":
        world = rl.RtcWorld.test_mirror_scene(W, H)
    elif name == "csg":
        world = rl.RtcWorld.test_csg_scene(W, H)
    else:
        red_ball = _material(api, color=(1, 0, 0), ambient=0.5)
        if name == "reflective_plane":
            world = _basic_world(rl, extra_shapes=[(api.O_PLANE, 2)], extra_mats=[_material(api, reflectivity=0.5)], extra_tr=[_T(0, -1, 0)])
        elif name == "schlick_plane":
            world = _basic_world(rl, extra_shapes=[(api.O_PLANE, 2), (api.O_SPHERE, 3)],
                                 extra_mats=[_material(api, transparency=0.5, refractive_index=1.5, reflectivity=0.5), red_ball],
                                 extra_tr=[_T(0, -1, 0), _T(0, -3.5, -0.5)])
        else:  # two lights: every secondary ray is evaluated once per light by the reference (mult > 1)
            glass = _material(api, color=(0.1, 0.1, 0.2), diffuse=0.2, transparency=0.9, reflectivity=0.9, refractive_index=1.5)
            world = _basic_world(rl, s1=glass, extra_shapes=[(api.O_PLANE, 2)], extra_mats=[_material(api, reflectivity=0.5)], extra_tr=[_T(0, -1, 0)],
                                 lights=[((-10, 10, -10), (0.6, 0.6, 0.6)), ((10, 10, -10), (0.4, 0.4, 0.4))], depth=3)
        world.camera = api.rtc_camera(W, H, math.pi / 3.0, (0.0, 1.5, -5.0), (0.0, -0.25, 0.0), (0.0, 1.0, 0.0))
    o, d = _rtc_camera_rays(world.camera)
    _SCENES[name] = (world, o, d)
    return _SCENES[name]


def _first_hit(rl, golden, name):
    """-> (comps, shade, shadow) of the scene's pixel-centre rays; computed once and left unchanged."""
    key = ("first", name)
    if key not in _SCENES:
        world, o, d = _scene(rl, golden, name)
        comps = world.prepare_rays(o, d)
        shade, shadow = world.shade_hits(comps)
        _SCENES[key] = (comps, shade, shadow)
    return _SCENES[key]


# ----------------------------------------------------------------------------- 1. the composition
def _compose(rl, world, o, d):
    """The loop of include/rl_render.h, level by level over whole batches -> (rgb [n, 3], rays, flagged).  Every node's contribution is
    kept with its root and its path (0: reflected, 1: refracted); a root's contributions are added in depth-first preorder, reflection
    first, which is the order of the sorted path tuples."""
    api = rl.api
    desc = api.RtcSceneDesc.from_address(world.desc)
    mats, nl = world.materials(), len(world.lights())
    void = np.array(list(desc.void_color), dtype=np.float64)
    n = o.shape[0]
    root, paths, w = np.arange(n), [()] * n, np.ones(n)
    remaining, mult, rays, flagged = int(desc.max_reflection_depth), 1, 0, 0
    contrib = []  # (root, path, rgb)
    while root.size:
        ps, ss = {}, {}
        k = world.prepare_rays(o, d, stats=ps)
        rays += mult * ps["rays"]
        flagged += ps["flagged"]
        hit = (k["hit"] != 0) & (nl != 0)
        for i in np.nonzero(~hit)[0]:
            contrib.append((int(root[i]), paths[i], void * w[i]))
        idx = np.nonzero(hit)[0]
        if not idx.size:
            break
        k, w_, root_, paths_ = k[idx], w[idx], root[idx], [paths[i] for i in idx]
        s, _ = world.shade_hits(k, stats=ss)
        rays += mult * ss["rays"]
        flagged += ss["flagged"]
        for i in range(idx.size):
            contrib.append((int(root_[i]), paths_[i], s["surface"][i] * w_[i]))
        m = mats[k["material"]]
        wl = w_ * float(nl)
        both = (m["reflectivity"] > 0.0) & (m["transparency"] > 0.0)
        wt = wl * m["transparency"] * np.where(both, 1.0 - s["schlick"], 1.0)
        wr = wl * m["reflectivity"] * np.where(both, s["schlick"], 1.0)
        fr = np.nonzero(s["refract"] != 0)[0] if remaining > 0 else np.zeros(0, dtype=np.int64)
        fl = np.nonzero(s["reflect"] != 0)[0] if remaining > 0 else np.zeros(0, dtype=np.int64)
        o = np.concatenate([s["reflected"]["origin"][fl], s["refracted"]["origin"][fr]])
        d = np.concatenate([s["reflected"]["dir"][fl], s["refracted"]["dir"][fr]])
        w = np.concatenate([wr[fl], wt[fr]])
        root = np.concatenate([root_[fl], root_[fr]])
        paths = [paths_[i] + (0,) for i in fl] + [paths_[i] + (1,) for i in fr]
        remaining, mult = remaining - 1, mult * nl
    contrib.sort(key=lambda c: (c[0], c[1]))
    rgb = np.zeros((n, 3))
    for r, _, c in contrib:
        rgb[r] = rgb[r] + c
    return rgb, rays, flagged


@pytest.mark.parametrize("name", GOLDEN_SCENES + HAND_SCENES)
def test_the_loop_of_prepare_and_shade_is_color_at_rays_byte_for_byte(rl, golden, name):
    world, o, d = _scene(rl, golden, name)
    st = {}
    want = world.color_at_rays(o, d, stats=st)
    rgb, rays, flagged = _compose(rl, world, o, d)
    assert rgb.tobytes() == want.tobytes(), (name, int((rgb != want).any(axis=1).sum()), float(np.abs(rgb - want).max()))
    assert rays == st["rays"], (name, rays, st["rays"])
    assert flagged == 0 and st["flagged"] == 0
    if name in HAND_SCENES:  # the hand-built worlds do reach what they are there for
        comps, shade, _ = _first_hit(rl, golden, name)
        assert (shade["reflect"] != 0).any()
        if name != "reflective_plane":
            assert ((shade["reflect"] != 0) & (shade["refract"] != 0)).any()
    if name == "schlick_plane":  # the reference's own colour for the Schlick branch (world.rs shade_hit_with_a_reflective_transparent_material)
        c = _compose(rl, world, *_rays([RAY]))[0][0]
        assert np.abs(c - (1.11500, 0.69643, 0.69243)).max() <= 1e-5


# ----------------------------------------------------------------------------- 2. shade_hits equals its parts
@pytest.mark.parametrize("name", GOLDEN_SCENES + HAND_SCENES)
def test_shade_hits_is_shadow_attenuation_then_lighting_light_by_light(rl, golden, name):
    world, o, d = _scene(rl, golden, name)
    comps, shade, shadow = _first_hit(rl, golden, name)
    lights = world.lights()
    hit = comps["hit"] != 0
    assert hit.any()
    st = {}
    shade2, shadow2 = world.shade_hits(comps, stats=st)
    assert shade2.tobytes() == shade.tobytes() and shadow2.tobytes() == shadow.tobytes()  # (a repeated call gives the same bytes)
    total, pairs = None, 0
    for li in range(len(lights)):
        pos, inten = lights["position"][li], lights["intensity"][li]
        att = world.shadow_attenuation(comps["over_point"], pos)
        want_att = np.where(hit, att, 0.0)  # hit == 0: no ray, and zeros in opt_out_shadow
        assert want_att.tobytes() == np.ascontiguousarray(shadow[:, li]).tobytes(), (name, li)
        surface = world.lighting(comps, pos, inten, att)
        assert not surface[~hit].any()
        total = surface if total is None else total + surface
        pairs += int((hit & (comps["over_point"] != pos).any(axis=1)).sum())
    assert total.tobytes() == np.ascontiguousarray(shade["surface"]).tobytes(), name
    assert st["rays"] == pairs, (name, st["rays"], pairs)


# ----------------------------------------------------------------------------- 3. against the oracle
def _are_equal(a, b):  # math/util.rs:4-22
    if math.isnan(a) or math.isnan(b):
        return False
    if math.isinf(a) and math.isinf(b):
        return a == b
    if abs(a - b) <= 2.220446049250313e-16 * 2.0:
        return True
    au, bu = struct.unpack("<Q", struct.pack("<d", a))[0], struct.unpack("<Q", struct.pack("<d", b))[0]
    return abs(au - bu) <= 8


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(v):  # Vec3d::norm (math/vector.rs:32-43): true division by the magnitude
    m = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return None if m == 0.0 else (v[0] / m, v[1] / m, v[2] / m)


def _py_prepare(o, d, ts, objs, normals, ior_of):
    """hit (intersect.rs:159-168) and prepare_computations (intersect.rs:48-115) in Python floats on the oracle's sorted list."""
    hi = -1
    for j in range(len(ts)):
        if ts[j] >= 0.0 and (hi < 0 or not (ts[hi] < ts[j])):
            hi = j
    if hi < 0:
        return None
    t = float(ts[hi])
    o, d = [float(x) for x in o], [float(x) for x in d]
    point = tuple(o[k] + d[k] * t for k in range(3))
    eye = _norm((-d[0], -d[1], -d[2]))
    nv = tuple(float(x) for x in normals[hi])
    inside = _dot(nv, eye) < 0.0
    if inside:
        nv = (-nv[0], -nv[1], -nv[2])
    over = tuple(point[k] + nv[k] * 1e-5 for k in range(3))
    under = tuple(point[k] - nv[k] * 1e-5 for k in range(3))
    containers, n1, n2 = [], 1.0, 1.0
    for j in range(len(ts)):
        same = _are_equal(float(ts[j]), t) and objs[j] == objs[hi]
        if same:
            n1 = ior_of(containers[-1]) if containers else 1.0
        if objs[j] in containers:
            containers.remove(objs[j])
        else:
            containers.append(objs[j])
        if same:
            n2 = ior_of(containers[-1]) if containers else 1.0
            break
    return dict(t=t, object=int(objs[hi]), point=point, eye_v=eye, normal_v=nv, inside=inside, over_point=over, under_point=under, n1=n1, n2=n2)


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_prepare_rays_and_lighting_equal_the_oracle_ray_by_ray(rl, oracle, golden, name):
    api = rl.api
    world, co, cd = _scene(rl, golden, name)
    rng = np.random.default_rng(77)
    pick = rng.choice(co.shape[0], 600, replace=False)
    eye = co[0]
    ro, rd = _random_rays(rng, eye, eye + cd[co.shape[0] // 2] * 5.0, 6.0, 0, 200, 100, 8)
    o, d = np.concatenate([co[pick], ro]), np.concatenate([cd[pick], rd])
    mats = world.materials()
    tris, shapes = world._table("triangles", api.RTC_TRIANGLE), world._table("shapes", api.RTC_SHAPE)
    obj_mat = np.concatenate([tris["material"], shapes["material"]])  # object identity: triangles first, then shapes
    ior_of = lambda obj: float(mats["refractive_index"][obj_mat[obj]])  # noqa: E731
    st = {}
    comps = world.prepare_rays(o, d, stats=st, allow_degenerate=True)
    assert st["rays"] == o.shape[0]
    skipped = n_hit = n_refr = 0
    for i in range(o.shape[0]):
        ts, objs, normals = oracle.rtc_intersect(world.desc, o[i], d[i], cap=64)
        if len(ts) > 48:
            skipped += 1  # beyond the device's list (flagged there, as in the renders)
            continue
        want = _py_prepare(o[i], d[i], ts, objs, normals, ior_of)
        k = comps[i]
        if want is None:
            assert k["hit"] == 0 and not np.frombuffer(k.tobytes(), dtype=np.uint8).any(), (name, i)
            continue
        n_hit += 1
        n_refr += want["n1"] != 1.0 or want["n2"] != 1.0
        assert k["hit"] == 1 and k["t"] == want["t"] and k["object"] == want["object"] and k["material"] == obj_mat[want["object"]], (name, i)
        assert k["inside"] == int(want["inside"]), (name, i)
        for f in ("normal_v", "point", "over_point", "under_point", "eye_v"):
            assert tuple(k[f]) == want[f], (name, i, f, tuple(k[f]), want[f])
        assert k["n1"] == want["n1"] and k["n2"] == want["n2"], (name, i, k["n1"], k["n2"], want["n1"], want["n2"])
    assert skipped * 100 < o.shape[0], (name, skipped)
    assert n_hit > 100, (name, n_hit)
    if name == "mirror":
        assert n_refr > 0  # the glass ball: the containers walk found something other than air
    # lighting against the oracle's, the material's plain colour as object_color
    light = world.lights()[0]
    hit = np.nonzero(comps["hit"] != 0)[0]
    kk = comps[hit].copy()
    kk["object_color"] = mats["color"][kk["material"]]
    att = np.where(np.arange(hit.size) % 2 == 0, 1.0, 0.25)
    got = world.lighting(kk, light["position"], light["intensity"], att)
    n_exact = 0
    for j in range(hit.size):
        k = kk[j]
        ref = oracle.rtc_lighting(mats[k["material"]], k["point"], light["position"], light["intensity"], k["eye_v"], k["normal_v"], float(att[j]))
        lightv = _norm(tuple(float(light["position"][c]) - float(k["point"][c]) for c in range(3)))
        nv, ev = tuple(float(x) for x in k["normal_v"]), tuple(float(x) for x in k["eye_v"])
        ldn = _dot(lightv, nv)
        exact = ldn < 0.0
        if not exact:  # -reflect(lightv, normal_v) . eye_v (vector.rs:57-59)
            dn = _dot(lightv, nv)
            refl = tuple(-(lightv[c] - (nv[c] * 2.0) * dn) for c in range(3))
            exact = _dot(refl, ev) <= 0.0
        if exact:  # no pow is reached
            n_exact += 1
            assert tuple(got[j]) == tuple(ref), (name, j, got[j], ref)
        else:
            assert np.abs(got[j] - ref).max() <= REL * max(1.0, np.abs(ref).max()), (name, j, got[j], ref)
    assert 0 < n_exact < hit.size, (name, n_exact, hit.size)


# ----------------------------------------------------------------------------- 4. the reference's known answers
def _close(c, want, eps=1e-5):
    return np.abs(np.asarray(c) - np.asarray(want)).max() <= eps  # color::test_utils::assert_colors_approx_equal


def test_world_basic_shading_and_shadow_known_answers(rl):
    rl.init(0)
    w = _basic_world(rl)
    k = w.prepare_rays(*_rays([((0, 0, -5), (0, 0, 1))]))  # world.rs shading_an_intersection
    assert k["hit"][0] == 1 and k["t"][0] == 4.0 and k["object"][0] == 0 and k["inside"][0] == 0
    s, sh = w.shade_hits(k)
    assert _close(s["surface"][0], (0.38066, 0.47583, 0.2855)) and sh[0, 0] == 1.0 and s["reflect"][0] == 0 and s["refract"][0] == 0
    inside = _basic_world(rl, light=((0, 0.25, 0), (1, 1, 1)))  # world.rs shading_an_intersection_from_the_inside
    k = inside.prepare_rays(*_rays([((0, 0, 0), (0, 0, 1))]))
    assert k["t"][0] == 0.5 and k["object"][0] == 1 and k["inside"][0] == 1 and tuple(k["normal_v"][0]) == (0.0, 0.0, -1.0)
    assert _close(inside.shade_hits(k)[0]["surface"][0], (0.90498, 0.90498, 0.90498))
    # world.rs is_shadowed: nothing collinear; an object between point and light; behind the light; behind the point
    pts = np.array([(0, 10, 0), (10, -10, 10), (-20, 20, -20), (-2, 2, -2)], dtype=np.float64)
    st = {}
    assert w.shadow_attenuation(pts, (-10.0, 10.0, -10.0), stats=st).tolist() == [1.0, 0.0, 1.0, 1.0] and st["rays"] == 4
    half = _basic_world(rl, s1=_material(rl.api, transparency=0.5), s2=_material(rl.api, transparency=1.0))  # world.rs partial_shadow...
    assert half.shadow_attenuation(pts[1:2], (-10.0, 10.0, -10.0)).tolist() == [0.5]
    st = {}  # coincident point and light: 1.0, no ray
    assert w.shadow_attenuation(pts[:2], pts[:2], stats=st).tolist() == [1.0, 1.0] and st["rays"] == 0


def test_prepare_computations_known_answers(rl):
    rl.init(0)
    api = rl.api
    plane = _shapes_world(rl, [(api.O_PLANE, np.eye(4), _material(api))])  # intersect.rs precomputing_the_reflection_vector
    k = plane.prepare_rays(*_rays([((0, 1, -1), (0, -SQ2 / 2.0, SQ2 / 2.0))]))
    assert k["hit"][0] == 1 and _close(k["reflect_v"][0], (0.0, SQ2 / 2.0, SQ2 / 2.0), 1e-12)
    glass = _material(api, transparency=1.0, refractive_index=1.5)
    ball = _shapes_world(rl, [(api.O_SPHERE, _T(0, 0, 1), glass)])  # intersect.rs the_under_point_is_offset_below_the_surface
    k = ball.prepare_rays(*_rays([((0, 0, -5), (0, 0, 1))]))
    assert k["t"][0] == 5.0 and k["under_point"][0][2] > 1e-5 / 2.0 and k["point"][0][2] < k["under_point"][0][2]
    assert k["over_point"][0][2] < -1e-5 / 2.0 and k["point"][0][2] > k["over_point"][0][2]
    # intersect.rs finding_n1_and_n2_at_various_intersections: A (scale 2, 1.5) contains B (z - 0.25, 2.0) and C (z + 0.25, 2.5); each ray
    # starts where hit() picks the next of the six intersections, so the lists carry negative t
    nested = _shapes_world(rl, [(api.O_SPHERE, np.diag([2.0, 2.0, 2.0, 1.0]), _material(api, transparency=1.0, refractive_index=1.5)),
                                (api.O_SPHERE, _T(0, 0, -0.25), _material(api, transparency=1.0, refractive_index=2.0)),
                                (api.O_SPHERE, _T(0, 0, 0.25), _material(api, transparency=1.0, refractive_index=2.5))])
    zs = [-4.0, -1.6, -1.0, 0.0, 1.0, 1.6]
    k = nested.prepare_rays(*_rays([((0, 0, z), (0, 0, 1)) for z in zs]))
    assert [(float(a), float(b)) for a, b in zip(k["n1"], k["n2"])] == [(1.0, 1.5), (1.5, 2.0), (2.0, 2.5), (2.5, 2.5), (2.5, 1.5), (1.5, 1.0)]
    assert k["object"].tolist() == [0, 1, 2, 1, 2, 0] and k["inside"].tolist() == [0, 0, 0, 1, 1, 1]


def test_schlick_known_answers(rl):
    rl.init(0)
    api = rl.api
    w = _shapes_world(rl, [(api.O_SPHERE, np.eye(4), _material(api, transparency=1.0, refractive_index=1.5))])
    # intersect.rs: total internal reflection; a perpendicular viewing angle; a small angle with n2 > n1
    k = w.prepare_rays(*_rays([((0, 0, SQ2 / 2.0), (0, 1, 0)), ((0, 0, 0), (0, 1, 0)), ((0, 0.99, -2), (0, 0, 1))]))
    assert [(float(a), float(b)) for a, b in zip(k["n1"], k["n2"])] == [(1.5, 1.0), (1.5, 1.0), (1.0, 1.5)]
    s, _ = w.shade_hits(k)
    assert s["schlick"][0] == 1.0 and s["refract"][0] == 0 and not np.frombuffer(s["refracted"][0].tobytes(), dtype=np.uint8).any()
    assert abs(s["schlick"][1] - 0.04) <= 1e-5 and s["refract"][1] == 1
    # 0.48873 is the figure for a refractive index of 1.5, printed to five digits for a comparison at 1e-4; the formula's value there is
    # r0 + (1 - r0) (1 - cos)^5 = 0.04 + 0.96 * (1 - sqrt(1 - 0.99^2))^5 = 0.4888144, 8.4e-5 away.  The reference's own test
    # (intersect.rs:492-505) uses its glass_sphere, index 1.52, and expects 0.49018 within 1e-5: checked below as it stands there.
    assert abs(s["schlick"][2] - 0.48873) <= 1e-4 and abs(s["schlick"][2] - 0.4888144) <= 1e-7 and s["refract"][2] == 1
    assert tuple(s["refracted"]["origin"][2]) == tuple(k["under_point"][2]) and s["reflect"].tolist() == [0, 0, 0]
    g152 = _shapes_world(rl, [(api.O_SPHERE, np.eye(4), _material(api, transparency=1.0, refractive_index=1.52))])  # sphere.rs glass_sphere
    s152, _ = g152.shade_hits(g152.prepare_rays(*_rays([((0, 0.99, -2), (0, 0, 1)), ((0, 0, 0), (0, 1, 0)), ((0, 0, SQ2 / 2.0), (0, 1, 0))])))
    assert abs(s152["schlick"][0] - 0.49018) <= 1e-5 and abs(s152["schlick"][1] - 0.04) <= 1e-2 and s152["schlick"][2] == 1.0
    opaque = _basic_world(rl)  # always computed: an opaque material in air gives r0 = 0 and (1 - cos)^5
    ko = opaque.prepare_rays(*_rays([((0, 0, -5), (0, 0, 1))]))
    assert opaque.shade_hits(ko)[0]["schlick"][0] == 0.0


# ----------------------------------------------------------------------------- 5. plumbing
def test_batch_sizes_and_slices_give_the_same_records(rl, golden):
    world, o, d = _scene(rl, golden, "mirror")
    comps, shade, shadow = _first_hit(rl, golden, "mirror")
    n = o.shape[0]
    assert n == W * H
    light = world.lights()[0]
    att = world.shadow_attenuation(comps["over_point"], light["position"])
    rgb = world.lighting(comps, light["position"], light["intensity"], att)
    for m in (1, 63, 64, 65):
        for lo in (0, n - m, 2000):
            sl = slice(lo, lo + m)
            st = {}
            assert world.prepare_rays(o[sl], d[sl], stats=st).tobytes() == comps[sl].tobytes(), (m, lo)
            assert st["rays"] == m
            s2, sh2 = world.shade_hits(comps[sl])
            assert s2.tobytes() == shade[sl].tobytes() and sh2.tobytes() == shadow[sl].tobytes(), (m, lo)
            assert world.shadow_attenuation(comps["over_point"][sl], light["position"]).tobytes() == att[sl].tobytes()
            assert world.lighting(comps[sl], light["position"], light["intensity"], att[sl]).tobytes() == rgb[sl].tobytes()


def test_device_forms_on_a_side_stream_then_render_status(rl, golden):
    import torch
    api = rl.api
    world, o, d = _scene(rl, golden, "mirror")
    comps, shade, shadow = _first_hit(rl, golden, "mirror")
    n = o.shape[0]
    light = world.lights()[0]
    lp, li = np.tile(light["position"], (n, 1)), np.tile(light["intensity"], (n, 1))
    att = world.shadow_attenuation(comps["over_point"], lp)
    rgb = world.lighting(comps, lp, li, att)
    stream = torch.cuda.Stream()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(n, -1).copy()).to("cuda:0")  # noqa: E731
    out = lambda nbytes: torch.zeros((n, nbytes), dtype=torch.uint8, device="cuda:0")  # noqa: E731
    d_rays, d_lp, d_li = dev(api.pack_rays(o, d)), dev(lp), dev(li)
    d_comps, d_shade, d_shadow, d_att, d_rgb = out(208), out(152), out(8), out(8), out(24)
    d_over = dev(comps["over_point"])
    torch.cuda.synchronize()
    s = stream.cuda_stream
    api.render_status(world)  # (drain whatever the host forms left in the ring)
    world.prepare_rays_device(d_rays.data_ptr(), n, d_comps.data_ptr(), stream=s)
    st = api.render_status(world)
    assert st["rays"] == n and st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert api.render_status(world)["rays"] == 0  # each query counts once
    world.shade_hits_device(d_comps.data_ptr(), n, d_shade.data_ptr(), d_shadow.data_ptr(), stream=s)
    n_shadow = int((comps["hit"] != 0).sum())
    assert api.render_status(world)["rays"] == n_shadow and api.render_status(world)["rays"] == 0
    world.shadow_attenuation_device(d_over.data_ptr(), d_lp.data_ptr(), n, d_att.data_ptr(), stream=s)
    assert api.render_status(world)["rays"] == n
    world.lighting_device(d_comps.data_ptr(), d_lp.data_ptr(), d_li.data_ptr(), d_att.data_ptr(), n, d_rgb.data_ptr(), stream=s)
    st = api.render_status(world)
    assert st["rays"] == 0 and st["rc"] == api.RL_OK  # a query of 0 rays
    stream.synchronize()
    assert d_comps.cpu().numpy().tobytes() == comps.tobytes()
    assert d_shade.cpu().numpy().tobytes() == shade.tobytes() and d_shadow.cpu().numpy().tobytes() == shadow.tobytes()
    assert d_att.cpu().numpy().tobytes() == att.tobytes() and d_rgb.cpu().numpy().tobytes() == rgb.tobytes()
    ss = {}  # with stats the device form is synchronous and reports the host form's counters
    world.shade_hits_device(d_comps.data_ptr(), n, d_shade.data_ptr(), 0, stream=s, stats=ss)
    assert ss["rays"] == n_shadow and d_shade.cpu().numpy().tobytes() == shade.tobytes()


def test_errors_empty_batches_and_material_range(rl, golden):
    import torch
    api = rl.api
    lib = api.render_lib()
    world, o, d = _scene(rl, golden, "mirror")
    comps, shade, shadow = _first_hit(rl, golden, "mirror")
    e3 = np.zeros((0, 3))
    st = {"rays": 7}
    assert world.prepare_rays(e3, e3, stats=st).shape == (0,) and st["rays"] == 0  # n = 0
    s0, sh0 = world.shade_hits(np.zeros(0, dtype=api.RTC_COMPS))
    assert s0.shape == (0,) and sh0.shape == (0, 1)
    assert world.shadow_attenuation(e3, e3).shape == (0,) and world.lighting(comps[:0], e3, e3, np.zeros(0)).shape == (0, 3)
    h = world.device()
    assert lib.rl_rtc_prepare_rays(h, None, 0, None, None) == api.RL_OK  # the empty batch touches nothing
    assert lib.rl_rtc_shade_hits(h, None, 0, None, None, None) == api.RL_OK
    assert lib.rl_rtc_shadow_attenuation(h, None, None, 0, None, None) == api.RL_OK
    assert lib.rl_rtc_lighting(h, None, None, None, None, 0, None) == api.RL_OK
    rays = api.pack_rays(o[:1], d[:1])
    k1, s1, v3, a1, rgb = comps[:1].copy(), np.zeros(1, dtype=api.RTC_SHADE), np.zeros((1, 3)), np.ones(1), np.zeros((1, 3))
    p = lambda a: a.ctypes.data  # noqa: E731
    INV = api.RL_E_INVALID
    assert lib.rl_rtc_prepare_rays(h, None, 1, p(k1), None) == INV and lib.rl_rtc_prepare_rays(h, p(rays), 1, None, None) == INV
    assert lib.rl_rtc_shade_hits(h, None, 1, p(s1), None, None) == INV and lib.rl_rtc_shade_hits(h, p(k1), 1, None, None, None) == INV
    assert lib.rl_rtc_shadow_attenuation(h, None, p(v3), 1, p(a1), None) == INV and lib.rl_rtc_shadow_attenuation(h, p(v3), None, 1, p(a1), None) == INV
    assert lib.rl_rtc_shadow_attenuation(h, p(v3), p(v3), 1, None, None) == INV
    assert lib.rl_rtc_lighting(h, None, p(v3), p(v3), p(a1), 1, p(rgb)) == INV and lib.rl_rtc_lighting(h, p(k1), None, p(v3), p(a1), 1, p(rgb)) == INV
    assert lib.rl_rtc_lighting(h, p(k1), p(v3), None, p(a1), 1, p(rgb)) == INV and lib.rl_rtc_lighting(h, p(k1), p(v3), p(v3), None, 1, p(rgb)) == INV
    assert lib.rl_rtc_lighting(h, p(k1), p(v3), p(v3), p(a1), 1, None) == INV
    assert lib.rl_rtc_prepare_rays_device(h, None, 1, p(k1), None, None) == INV and lib.rl_rtc_lighting_device(h, p(k1), p(v3), p(v3), p(a1), 1, None, None) == INV
    rtiow = rl.World.golden_test_scene()  # a scene of the RTIOW family
    rt = rtiow.device()
    assert lib.rl_rtc_prepare_rays(rt, p(rays), 1, p(k1), None) == INV and lib.rl_rtc_shade_hits(rt, p(k1), 1, p(s1), None, None) == INV
    assert lib.rl_rtc_shadow_attenuation(rt, p(v3), p(v3), 1, p(a1), None) == INV and lib.rl_rtc_lighting(rt, p(k1), p(v3), p(v3), p(a1), 1, p(rgb)) == INV
    assert lib.rl_rtc_shade_hits_device(rt, p(k1), 1, p(s1), None, None, None) == INV
    assert lib.rl_rtc_shadow_attenuation_device(rt, p(v3), p(v3), 1, p(a1), None, None) == INV
    # a material index outside the table: refused by the host forms before launch, zeros from the device forms
    hit = np.nonzero(comps["hit"] != 0)[0][:5]
    bad = comps[hit].copy()
    bad["material"][2] = len(world.materials())
    light = world.lights()[0]
    for call in (lambda: world.shade_hits(bad), lambda: world.lighting(bad, light["position"], light["intensity"], 1.0)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == INV
    d_bad = torch.from_numpy(bad.view(np.uint8).reshape(5, 208).copy()).to("cuda:0")
    d_s = torch.full((5, 152), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_sh = torch.full((5, 8), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_rgb = torch.full((5, 24), 0xAB, dtype=torch.uint8, device="cuda:0")
    d_lp = torch.from_numpy(np.tile(light["position"], (5, 1))).to("cuda:0")
    d_li = torch.from_numpy(np.tile(light["intensity"], (5, 1))).to("cuda:0")
    d_att = torch.ones(5, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    st = {}
    world.shade_hits_device(d_bad.data_ptr(), 5, d_s.data_ptr(), d_sh.data_ptr(), stats=st)
    world.lighting_device(d_bad.data_ptr(), d_lp.data_ptr(), d_li.data_ptr(), d_att.data_ptr(), 5, d_rgb.data_ptr())
    torch.cuda.synchronize()
    got = d_s.cpu().numpy().reshape(-1).view(api.RTC_SHADE)
    keep = np.arange(5) != 2
    assert got[keep].tobytes() == shade[hit][keep].tobytes() and not d_s.cpu().numpy()[2].any() and not d_sh.cpu().numpy()[2].any()
    assert st["rays"] == 4
    want_rgb = world.lighting(comps[hit][keep], light["position"], light["intensity"], 1.0)
    got_rgb = d_rgb.cpu().numpy().reshape(-1).view(np.float64).reshape(5, 3)
    assert got_rgb[keep].tobytes() == want_rgb.tobytes() and not got_rgb[2].any()


def test_missed_elements_no_lights_and_degenerate_rays(rl, golden):
    api = rl.api
    world, o, d = _scene(rl, golden, "reflective_plane")  # its top rows look over the horizon
    comps, shade, shadow = _first_hit(rl, golden, "reflective_plane")
    miss = comps["hit"] == 0
    assert miss.any() and not miss.all()
    assert not np.frombuffer(comps[miss].tobytes(), dtype=np.uint8).any()  # hit == 0: every other field is 0
    assert not np.frombuffer(shade[miss].tobytes(), dtype=np.uint8).any() and not shadow[miss].any()
    # a hand-made hit == 0 record carrying garbage in its other fields gives zeros too, and its neighbours are unchanged
    hit = np.nonzero(~miss)[0][:6]
    mixed = comps[hit].copy()
    mixed["hit"][[1, 4]] = 0
    st = {}
    s, sh = world.shade_hits(mixed, stats=st)
    keep = np.ones(6, dtype=bool)
    keep[[1, 4]] = False
    assert s[keep].tobytes() == shade[hit][keep].tobytes() and sh[keep].tobytes() == shadow[hit][keep].tobytes()
    assert not np.frombuffer(s[~keep].tobytes(), dtype=np.uint8).any() and not sh[~keep].any() and st["rays"] == 4
    light = world.lights()[0]
    assert not world.lighting(mixed, light["position"], light["intensity"], 1.0)[~keep].any()
    # a world without lights: the reference's reduce over no lights is None
    glass = _material(api, transparency=0.9, reflectivity=0.9, refractive_index=1.5)
    dark = _basic_world(rl, s1=glass, lights=[])
    k = dark.prepare_rays(*_rays([((0, 0, -5), (0, 0, 1)), ((0, 0, -5), (0, 1, 0))]))
    assert k["hit"].tolist() == [1, 0] and k["n2"][0] == 1.5
    st = {}
    s, sh = dark.shade_hits(k, stats=st)
    assert sh.shape == (2, 0) and st["rays"] == 0
    assert not s["surface"].any() and s["reflect"].tolist() == [0, 0] and s["refract"].tolist() == [0, 0]
    assert not np.frombuffer(s["reflected"].tobytes(), dtype=np.uint8).any() and not np.frombuffer(s["refracted"].tobytes(), dtype=np.uint8).any()
    assert _compose(rl, dark, *_rays([((0, 0, -5), (0, 0, 1))]))[0].tobytes() == dark.color_at_rays(*_rays([((0, 0, -5), (0, 0, 1))])).tobytes()
    # degenerate rays: a zero direction finds nothing and reaches no panic site; a NaN ray changes no other element
    w = _basic_world(rl)
    ro, rd = _rays([((0, 0, -5), (0, 0, 1)), ((0, 0.2, -5), (0, 0, 1)), ((0, 0, -5), (0, 0, 0)), ((0.3, 0, -5), (0, 0, 1)), ((0, 0, 0), (0, 0, 1))])
    st = {}
    clean = w.prepare_rays(ro, rd, stats=st)
    assert st["flagged"] == 0 and st["rc"] == api.RL_OK and clean["hit"].tolist() == [1, 1, 0, 1, 1]
    no, nd = ro.copy(), rd.copy()
    no[2], nd[2] = (float("nan"), 0.0, -5.0), (0.0, float("nan"), 1.0)
    got = w.prepare_rays(no, nd, allow_degenerate=True)
    keep = np.arange(5) != 2
    assert got[keep].tobytes() == clean[keep].tobytes()
    s_clean, _ = w.shade_hits(clean)
    s_got, _ = w.shade_hits(got, allow_degenerate=True)
    assert s_got[keep].tobytes() == s_clean[keep].tobytes()
