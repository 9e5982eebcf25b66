"""GPU tier: the material queries (World.scatter_rays = Material::scatter + Material::emitted for buffers of hit records with per-element
RNG cursors, World.texture_values = Texture::value; include/rl_render.h).

The main yardstick is the library's own ray_color_rays, whose kernels this feature does not touch and which the path-query tests pin to
the renders and, through them, to the oracle: a host loop built from hit_rays and scatter_rays must give its colours, cursors and ray
counts back bit for bit.  Beside it: known answers against a NumPy restatement of material.rs on the oracle's ChaCha8 draws."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SCENES = ["golden_test_scene", "bouncing_spheres", "cow_scene", "perlin_spheres", "simple_light"]


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


def _compose(world, p, rays, cur):
    """ray_color (camera.rs:232-260) as a host loop over hit_rays and scatter_rays.  Only live paths are passed on, so the batch shrinks
    and every path changes its place in it from bounce to bounce.  -> colours, final cursors, per-path ray counts, the summed rng_words of
    the scatter calls, and the first bounce's (hits, scatter records) of the paths that hit something."""
    n = rays.shape[0]
    bg = np.array(p.background, dtype=np.float64)
    total, thr = np.zeros((n, 3)), np.ones((n, 3))
    counts = np.zeros(n, dtype=np.uint32)
    out_cur = cur.copy()
    live = np.arange(n)
    r, c = rays.copy(), cur.copy()
    words, first = 0, None
    for _ in range(p.max_depth):
        if live.size == 0:
            break
        hits = world.hit_rays(r["origin"], r["dir"], r["time"], tmin=1e-10)
        counts[live] += 1
        miss = hits["hit"] == 0
        total[live[miss]] = total[live[miss]] + thr[live[miss]] * bg
        live, r, c, hits = live[~miss], r[~miss], c[~miss], hits[~miss]
        if live.size == 0:
            break
        st = {}
        rec, c = world.scatter_rays(r, hits, c, p.seed, stats=st, allow_degenerate=True)
        assert st["rays"] == live.size and st["flagged"] == 0
        assert st["node_tests"] == st["sphere_tests"] == st["planar_tests"] == st["instance_enters"] == 0
        words += st["rng_words"]
        if first is None:
            first = (hits, rec)
        total[live] = total[live] + thr[live] * rec["emitted"]
        out_cur[live] = c
        go = rec["scatter"] == 1
        thr[live[go]] = thr[live[go]] * rec["attenuation"][go]
        live, r, c = live[go], np.ascontiguousarray(rec["scattered"][go]), c[go]
    return total, out_cur, counts, words, first


_CASES = {}


def _case(rl, golden, name):
    """Per scene, computed once and shared: the 64-wide frame's camera rays (cursors at word 0, and the same pixels with every cursor
    started at word 7, the odd-position path), ray_color_rays of both, and the composition of both."""
    if name in _CASES:
        return _CASES[name]
    api = rl.api
    if name == "cow_scene":
        world = rl.World.cow_scene(golden("spot_triangulated.obj.gz"), _spot_texture())
    elif name == "bouncing_spheres":
        world = rl.World.bouncing_spheres(1)
    else:
        world = getattr(rl.World, name)()
    p = world.params
    p.image_width, p.samples_per_pixel = 64, 1
    p.max_depth = min(p.max_depth, 20)
    cam = rl.Camera(p)
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), W)
    case = {"world": world, "p": p, "cam": cam}
    for pos in (0, 7):
        cur0 = api.pack_cursors(x * np.uint64(W) + y, pos)
        rays, cur = cam.get_rays(x, y, cur0)
        want = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays, allow_degenerate=True)
        got = _compose(world, p, rays, cur)
        case[pos] = {"cur0": cur0, "rays": rays, "cur": cur, "want": want, "got": got}
    _CASES[name] = case
    return case


@pytest.mark.parametrize("name", SCENES)
def test_composition_of_hit_rays_and_scatter_rays_equals_ray_color_rays(rl, golden, name):
    """1: colours, final cursors and per-path ray counts byte-equal, with cursors at word 0 and at word 7; the word accounting closes;
    the composition is the same with the fast traversal switched off.  (The issue words the accounting as "scatter words + get_rays words
    = the rng_words of a counting ray_color_rays"; a counting ray_color_rays counts the path's words only — include/rl_render.h — so that
    is asserted as such, and scatter + get_rays words are held against the counting sample-parallel render of the same frame, which
    counts both.)"""
    api = rl.api
    case = _case(rl, golden, name)
    world, p, cam = case["world"], case["p"], case["cam"]
    for pos in (0, 7):
        k = case[pos]
        (rgb, cur, counts, words, _), (w_rgb, w_cur, w_counts) = k["got"], k["want"]
        print(name, "word_pos", pos, "paths", rgb.shape[0], "rays", int(counts.sum()), "scatter words", words)
        assert rgb.tobytes() == w_rgb.tobytes(), (name, pos, np.abs(rgb - w_rgb).max())
        assert cur.tobytes() == w_cur.tobytes(), (name, pos)
        assert counts.tobytes() == w_counts.tobytes(), (name, pos)
        st = {}
        world.ray_color_rays(None, None, None, k["cur"], p.seed, p.max_depth, p.background, rays=k["rays"], stats=st, allow_degenerate=True)
        assert words == st["rng_words"], (name, pos, words, st["rng_words"])
        assert words == int((cur["word_pos"] - k["cur"]["word_pos"]).sum(dtype=np.uint64))
        if pos == 0:
            gs = {}
            cam.render_independent_rows(world, 0, 1, stats=gs, allow_degenerate=True)
            get_words = int((k["cur"]["word_pos"] - k["cur0"]["word_pos"]).sum(dtype=np.uint64))
            assert words + get_words == gs["rng_words"], (name, words, get_words, gs["rng_words"])
    api.set_fast_traversal(False)
    try:
        off = _compose(world, p, case[7]["rays"], case[7]["cur"])
    finally:
        api.set_fast_traversal(True)
    for a, b in zip(off[:3], case[7]["got"][:3]):
        assert a.tobytes() == b.tobytes(), name


# ---------------------------------------------------------------------------------------------- 2: known answers
def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _normalize(a):  # vec3.rs:56: self * (1.0 / length)
    k = 1.0 / math.sqrt(_dot(a, a))
    return (a[0] * k, a[1] * k, a[2] * k)


def _approx0(x, eps):
    return x == 0.0 or abs(x - 0.0) <= eps


class _Draws:
    """The draws of ChaCha8Rng::seed_from_u64(seed) after set_stream(stream) from an even word position on, taken from the oracle."""

    def __init__(self, oracle, seed, stream, pos):
        assert pos % 2 == 0
        skip = [("u64",)] * (pos // 2)
        n = 96
        self.uni = oracle.chacha_script(seed, [("set_stream", stream)] + skip + [("uniform",)] * n)[0][1 + len(skip):]
        self.f64 = oracle.chacha_script(seed, [("set_stream", stream)] + skip + [("f64",)] * n)[0][1 + len(skip):]
        self.k = 0

    def uniform(self):
        self.k += 1
        return float(self.uni[self.k - 1])

    def gen_f64(self):
        self.k += 1
        return float(self.f64[self.k - 1])

    def unit_sphere(self):  # rand_distr 0.4.3 UnitSphere
        while True:
            x1, x2 = self.uniform(), self.uniform()
            s = x1 * x1 + x2 * x2
            if s >= 1.0:
                continue
            f = 2.0 * math.sqrt(1.0 - s)
            return (x1 * f, x2 * f, 1.0 - 2.0 * s)


def _scatter_ref(api, m, color, d, time, hit, rng):
    """material.rs under the arithmetic contract: -> (scatter, attenuation, emitted, scattered dir, side) with side =
    'reflect' / 'refract' for Dielectric.  `color` = the material's (solid) texture value."""
    n = tuple(float(v) for v in hit["normal"])
    zero = (0.0, 0.0, 0.0)
    kind = int(m["kind"])
    if kind == api.MAT_FLAT:
        return 0, zero, zero, zero, None
    if kind == api.MAT_DIFFUSE_LIGHT:
        return 0, zero, color, zero, None
    if kind == api.MAT_ISOTROPIC:
        return 1, color, zero, rng.unit_sphere(), None
    if kind == api.MAT_LAMBERTIAN:
        u = rng.unit_sphere()
        v = (n[0] + u[0], n[1] + u[1], n[2] + u[2])
        if _approx0(v[0], 1e-8) and _approx0(v[1], 1e-8) and _approx0(v[2], 1e-8):
            v = n
        return 1, color, zero, v, None
    if kind == api.MAT_METAL:
        k = 2.0 * _dot(d, n)
        r = _normalize((d[0] - n[0] * k, d[1] - n[1] * k, d[2] - n[2] * k))
        u, fz = rng.unit_sphere(), float(m["fuzz"])
        v = (r[0] + u[0] * fz, r[1] + u[1] * fz, r[2] + u[2] * fz)
        if _dot(v, n) > 0.0:
            return 1, tuple(float(x) for x in m["albedo"]), zero, v, None
        return 0, zero, zero, zero, None
    assert kind == api.MAT_DIELECTRIC
    ri = 1.0 / float(m["ior"]) if hit["front_face"] else float(m["ior"])
    ud = _normalize(d)
    cos_theta = min(_dot((-ud[0], -ud[1], -ud[2]), n), 1.0)
    sin_theta = math.sqrt(1.0 - cos_theta * cos_theta)
    reflect = ri * sin_theta > 1.0
    if not reflect:
        q = (1.0 - ri) / (1.0 + ri)
        r0 = q * q
        xx = 1.0 - cos_theta
        x2 = xx * xx
        reflect = r0 + (1.0 - r0) * (xx * (x2 * x2)) > rng.gen_f64()
    if reflect:
        k = 2.0 * _dot(ud, n)
        v = (ud[0] - n[0] * k, ud[1] - n[1] * k, ud[2] - n[2] * k)
    else:
        perp = ((ud[0] + n[0] * cos_theta) * ri, (ud[1] + n[1] * cos_theta) * ri, (ud[2] + n[2] * cos_theta) * ri)
        k = -math.sqrt(abs(1.0 - _dot(perp, perp)))
        v = (perp[0] + n[0] * k, perp[1] + n[1] * k, perp[2] + n[2] * k)
    return 1, (1.0, 1.0, 1.0), zero, v, "reflect" if reflect else "refract"


COLORS = {"lambertian": (0.25, 0.5, 0.125), "isotropic": (0.7, 0.3, 0.9), "light": (4.0, 3.0, 2.5)}


@pytest.fixture(scope="module")
def material_world(rl):
    """One sphere per material kind (the flattened scene holds the materials its objects use)."""
    api = rl.api

    def fn(b):
        mats = [b.lambertian(b.solid(COLORS["lambertian"])), b.metal((0.8, 0.6, 0.2), 0.3), b.metal((0.9, 0.9, 0.7), 0.0), b.dielectric(1.5),
                b.isotropic(b.solid(COLORS["isotropic"])), b.diffuse_light(b.solid(COLORS["light"])), b.flat()]
        return b.list([b.sphere((3.0 * i, 0.0, -5.0), 1.0, m) for i, m in enumerate(mats)])

    world = rl.World.build(fn)
    table = world.materials()
    kinds = {"lambertian": api.MAT_LAMBERTIAN, "dielectric": api.MAT_DIELECTRIC, "isotropic": api.MAT_ISOTROPIC, "light": api.MAT_DIFFUSE_LIGHT,
             "flat": api.MAT_FLAT}
    index = {k: int(np.flatnonzero(table["kind"] == v)[0]) for k, v in kinds.items()}
    index["metal_fuzzy"] = int(np.flatnonzero((table["kind"] == api.MAT_METAL) & (table["fuzz"] == 0.3))[0])
    index["metal_mirror"] = int(np.flatnonzero((table["kind"] == api.MAT_METAL) & (table["fuzz"] == 0.0))[0])
    return world, table, index


C14 = 0.14  # cos_theta of the mixed Schlick case: reflectance 0.04 + 0.96 * 0.86^5 = 0.4916
KNOWN = [  # (case, material, incident direction, normal, front_face)
    ("lambertian", "lambertian", (0.3, -1.0, 0.2), (0.0, 1.0, 0.0), 1),
    ("metal fuzz 0.3", "metal_fuzzy", (1.0, -1.0, 0.5), (0.0, 1.0, 0.0), 1),
    ("metal fuzz 0, normal facing away", "metal_mirror", (0.0, -1.0, 0.0), (0.0, -1.0, 0.0), 1),
    ("dielectric front, normal incidence", "dielectric", (0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 1),
    ("dielectric back, normal incidence", "dielectric", (0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 0),
    ("dielectric back, total internal reflection", "dielectric", (1.0, 0.0, -0.5), (0.0, 0.0, 1.0), 0),
    ("dielectric front, cos_theta 0.14", "dielectric", (math.sqrt(1.0 - C14 * C14), -C14, 0.0), (0.0, 1.0, 0.0), 1),
    ("isotropic", "isotropic", (0.0, 0.0, -1.0), (1.0, 0.0, 0.0), 1),
    ("diffuse light", "light", (0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 1),
    ("flat", "flat", (0.0, 0.0, -1.0), (0.0, 0.0, 1.0), 1),
]


@pytest.mark.parametrize("case", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers_against_a_numpy_restatement(rl, oracle, material_world, case):
    """2: 256 cursors per case on hand-made hit records; flags, cursors and draw counts exact, values array_equal (the restatement uses
    only IEEE + * / sqrt in the kernel's order)."""
    api = rl.api
    label, mat, d, normal, front = case
    world, table, index = material_world
    m = table[index[mat]]
    color = COLORS.get(mat, (0.0, 0.0, 0.0))
    n, seed = 256, 2024
    hits = np.zeros(n, dtype=api.RTIOW_HIT)
    hits["t"], hits["hit"], hits["front_face"], hits["material"] = 1.0, 1, front, index[mat]
    hits["p"] = np.stack([np.linspace(-2.0, 2.0, n), np.full(n, 0.25), np.linspace(1.0, -3.0, n)], axis=1)
    hits["normal"], hits["u"], hits["v"] = normal, 0.3, 0.6
    rays = api.pack_rays(np.zeros((n, 3)), np.tile(d, (n, 1)), np.linspace(0.0, 1.0, n))
    cur = api.pack_cursors(np.arange(n, dtype=np.uint64) + np.uint64(1000), 2 * (np.arange(n, dtype=np.uint64) % np.uint64(12)))
    st = {}
    rec, out_cur = world.scatter_rays(rays, hits, cur, seed, stats=st)
    want = np.zeros(n, dtype=api.SCATTER)
    want_cur = cur.copy()
    sides = {"reflect": 0, "refract": 0}
    for i in range(n):
        rng = _Draws(oracle, seed, int(cur["stream"][i]), int(cur["word_pos"][i]))
        some, att, emitted, v, side = _scatter_ref(api, m, color, d, float(rays["time"][i]), hits[i], rng)
        want_cur["word_pos"][i] += 2 * rng.k
        want["scatter"][i], want["attenuation"][i], want["emitted"][i] = some, att, emitted
        if some:
            want["scattered"]["origin"][i], want["scattered"]["dir"][i], want["scattered"]["time"][i] = hits["p"][i], v, rays["time"][i]
        if side:
            sides[side] += 1
    drawn = int((want_cur["word_pos"] - cur["word_pos"]).sum())
    print(label, "scattered", int(want["scatter"].sum()), "words drawn", drawn, "dielectric sides", sides)
    assert np.array_equal(rec["scatter"], want["scatter"]) and np.array_equal(out_cur, want_cur), label
    assert st["rays"] == n and st["flagged"] == 0 and st["rng_words"] == drawn, (label, st, drawn)
    for f in ("attenuation", "emitted"):
        assert np.array_equal(rec[f], want[f]), (label, f)
    for f in ("origin", "dir", "time"):
        assert np.array_equal(rec["scattered"][f], want["scattered"][f]), (label, f)
    assert not rec["_pad"].any()
    if label.startswith("metal fuzz 0,"):  # always absorbed, and the draws are consumed all the same
        assert not rec["scatter"].any() and (out_cur["word_pos"] >= cur["word_pos"] + np.uint64(4)).all()
    if label.endswith("total internal reflection"):  # no Schlick draw where refraction is impossible
        assert np.array_equal(out_cur, cur) and sides == {"reflect": n, "refract": 0}
    if label.endswith("cos_theta 0.14"):  # the restatement alone puts at least a quarter of the cursors on each side
        assert sides["reflect"] >= n // 4 and sides["refract"] >= n // 4, sides
    if mat in ("lambertian", "isotropic", "metal_fuzzy"):
        assert rec["scatter"].all() and (out_cur["word_pos"] >= cur["word_pos"] + np.uint64(4)).all()
    if mat == "light":
        assert np.array_equal(rec["emitted"], np.tile(COLORS["light"], (n, 1)))


# ---------------------------------------------------------------------------------------------- 3: textures
@pytest.mark.parametrize("name", SCENES)
def test_texture_values_equal_the_first_bounce_attenuation_and_emission(rl, golden, name):
    """3a: texture_values of (material.texture, u, v, p) for every Lambertian hit of the composition's first bounce is that bounce's
    attenuation, bit for bit; the same for DiffuseLight hits and `emitted` (simple_light)."""
    api = rl.api
    case = _case(rl, golden, name)
    world = case["world"]
    hits, rec = case[0]["got"][4]
    table = world.materials()
    kinds = table["kind"][hits["material"]]
    seen = 0
    for kind, field in ((api.MAT_LAMBERTIAN, "attenuation"), (api.MAT_DIFFUSE_LIGHT, "emitted")):
        sel = kinds == kind
        if not sel.any():
            continue
        seen += int(sel.sum())
        h = hits[sel]
        got = world.texture_values(table["texture"][h["material"]], np.stack([h["u"], h["v"]], axis=1), h["p"])
        assert got.tobytes() == np.ascontiguousarray(rec[field][sel]).tobytes(), (name, field)
    assert seen > 0, name
    if name == "simple_light":
        assert (kinds == api.MAT_DIFFUSE_LIGHT).any()


def test_noise_texture_against_the_oracle(rl, oracle, golden):
    """3b: Noise (texture.rs:84-94) = 0.5 * (1 + sin(scale * p.z + 10 * turb(p, 7))) on oracle.perlin_turb, at the project's 1e-9 bar
    for libm-dependent colour."""
    api = rl.api
    case = _case(rl, golden, "perlin_spheres")
    world = case["world"]
    tex, perlins = world.textures(), world.perlins()
    assert tex.shape[0] == 1 and tex[0]["kind"] == api.TEX_NOISE
    hits = case[0]["got"][4][0]
    pts = np.concatenate([hits["p"][:: max(1, hits.shape[0] // 200)], np.random.default_rng(3).uniform(-40.0, 40.0, (100, 3))])
    got = world.texture_values(np.zeros(pts.shape[0], dtype=np.uint32), np.zeros((pts.shape[0], 2)), pts)
    pn = perlins[int(tex[0]["image"]):int(tex[0]["image"]) + 1]
    want = np.array([0.5 * (1.0 + math.sin(float(tex[0]["inv_scale"]) * q[2] + 10.0 * oracle.perlin_turb(pn, q, 7))) for q in pts])
    err = np.abs(got - want[:, None]).max()
    print("noise points", pts.shape[0], "max |d|", err)
    assert err <= 1e-9, err
    assert (got[:, 0] == got[:, 1]).all() and (got[:, 1] == got[:, 2]).all()


def test_checker_texture_against_a_numpy_restatement(rl):
    """3c: Checker (texture.rs:41-55), nested, exact: floor(p * inv_scale) as integers, the parity of their sum picks the child."""
    api = rl.api
    ca, cb, cc = (0.1, 0.2, 0.3), (0.9, 0.8, 0.7), (0.5, 0.25, 0.125)

    def fn(b):
        inner = b.checker(1.7, b.solid(cb), b.solid(cc))
        return b.list([b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian(b.checker(0.32, b.solid(ca), inner)))])

    world = rl.World.build(fn)
    tex = world.textures()
    root = int(world.materials()[0]["texture"])
    assert tex[root]["kind"] == api.TEX_CHECKER
    rng = np.random.default_rng(11)
    pts = np.concatenate([rng.uniform(-6.0, 6.0, (500, 3)), rng.integers(-4, 5, (200, 3)) * 0.32, rng.integers(-4, 5, (57, 3)).astype(np.float64)])

    def value(t, q):
        while tex[t]["kind"] == api.TEX_CHECKER:
            s = sum(int(math.floor(q[a] * float(tex[t]["inv_scale"]))) for a in range(3))
            t = int(tex[t]["even"] if s % 2 == 0 else tex[t]["odd"])
        return tex[t]["color"]

    want = np.array([value(root, q) for q in pts])
    got = world.texture_values(np.full(pts.shape[0], root, dtype=np.uint32), np.zeros((pts.shape[0], 2)), pts)
    assert np.array_equal(got, want)
    assert len({tuple(c) for c in want.tolist()}) == 3  # all three leaves are reached


# ---------------------------------------------------------------------------------------------- 4: placement
def test_results_do_not_depend_on_placement(rl, golden):
    """4: the per-element bytes are the same for batch sizes 1, 63, 64, 65 and 257, for a batch larger than the launch has lanes (a lane
    then handles two elements on different streams: a stale ring would show), and in shuffled order."""
    api = rl.api
    case = _case(rl, golden, "golden_test_scene")
    world, p = case["world"], case["p"]
    hits = case[7]["got"][4][0]
    keep = np.flatnonzero(case[7]["want"][2] >= 1)  # (every path traces its first ray)
    first_hit = np.flatnonzero(world.hit_rays(case[7]["rays"]["origin"], case[7]["rays"]["dir"], case[7]["rays"]["time"])["hit"] == 1)
    assert first_hit.shape[0] == hits.shape[0] and keep.shape[0] == case[7]["rays"].shape[0]
    base = 257
    pick = np.linspace(0, hits.shape[0] - 1, base).astype(np.int64)
    h, r, c = hits[pick], case[7]["rays"][first_hit][pick], case[7]["cur"][first_hit][pick]
    kinds = set(world.materials()["kind"][h["material"]].tolist())
    assert {api.MAT_LAMBERTIAN, api.MAT_METAL, api.MAT_DIELECTRIC} <= kinds
    full, full_cur = world.scatter_rays(r, h, c, p.seed)
    for k in (1, 63, 64, 65):
        rec, cur = world.scatter_rays(r[:k], h[:k], c[:k], p.seed)
        assert rec.tobytes() == full[:k].tobytes() and cur.tobytes() == full_cur[:k].tobytes(), k
    perm = np.random.default_rng(29).permutation(base)
    rec, cur = world.scatter_rays(r[perm], h[perm], c[perm], p.seed)
    assert rec.tobytes() == full[perm].tobytes() and cur.tobytes() == full_cur[perm].tobytes()
    lanes = api.material_query_max_lanes()
    assert lanes % base != 0  # element i and element i + lanes, which share a lane, are different base elements
    idx = np.arange(lanes + 1000) % base
    st = {}
    rec, cur = world.scatter_rays(r[idx], h[idx], c[idx], p.seed, stats=st)
    assert rec.tobytes() == full[idx].tobytes() and cur.tobytes() == full_cur[idx].tobytes()
    assert st["rays"] == idx.shape[0]
    pts = np.random.default_rng(31).uniform(-3.0, 3.0, (base, 3))
    tex = np.arange(base, dtype=np.uint32) % np.uint32(world.textures().shape[0])
    want = world.texture_values(tex, np.zeros((base, 2)), pts)
    assert world.texture_values(tex[idx], np.zeros((idx.shape[0], 2)), pts[idx]).tobytes() == want[idx].tobytes()


# ---------------------------------------------------------------------------------------------- 5: edges
def test_edges(rl, golden, material_world):
    """5: n = 0, NULL buffers, an RTC scene, word_pos >= 2^31, a material index outside the table (host form: RL_E_INVALID; device form:
    zeros), hit == 0, aliasing cursors, and the one panic site (Dielectric with a zero incident direction)."""
    import torch
    api = rl.api
    lib = api.render_lib()
    world, table, index = material_world
    n = 8
    hits = np.zeros(n, dtype=api.RTIOW_HIT)
    hits["hit"], hits["front_face"], hits["material"], hits["normal"], hits["p"] = 1, 1, index["dielectric"], (0.0, 1.0, 0.0), (1.0, 2.0, 3.0)
    hits["material"][1], hits["material"][2] = index["lambertian"], index["metal_fuzzy"]
    rays = api.pack_rays(np.zeros((n, 3)), np.tile((0.5, -1.0, 0.25), (n, 1)), np.full(n, 0.5))
    cur = api.pack_cursors(np.arange(n, dtype=np.uint64) + np.uint64(40), 3)
    out = np.zeros(n, dtype=api.SCATTER)
    args = lambda sc=None, r=rays, h=hits, c=cur, k=n, o=out, oc=None: (sc or world.device(), r.ctypes.data if r is not None else None,  # noqa: E731
                                                                        h.ctypes.data if h is not None else None, c.ctypes.data if c is not None else None,
                                                                        k, 5, o.ctypes.data if o is not None else None, oc, None)
    # n = 0, NULL buffers, the other scene family
    assert lib.rl_rtiow_scatter_rays(world.device(), None, None, None, 0, 5, None, None, None) == api.RL_OK
    assert lib.rl_rtiow_texture_values(world.device(), None, None, None, 0, None) == api.RL_OK
    rec, c0 = world.scatter_rays(rays[:0], hits[:0], cur[:0], 5)
    assert rec.shape == (0,) and c0.shape == (0,) and world.texture_values([], np.zeros((0, 2)), np.zeros((0, 3))).shape == (0, 3)
    for kw in ({"r": None}, {"h": None}, {"c": None}, {"o": None}):
        assert lib.rl_rtiow_scatter_rays(*args(**kw)) == api.RL_E_INVALID, kw
    t1, uv1, p1, o1 = np.zeros(1, dtype=np.uint32), np.zeros((1, 2)), np.zeros((1, 3)), np.zeros((1, 3))
    for a in ((None, uv1.ctypes.data, p1.ctypes.data, 1, o1.ctypes.data), (t1.ctypes.data, None, p1.ctypes.data, 1, o1.ctypes.data),
              (t1.ctypes.data, uv1.ctypes.data, None, 1, o1.ctypes.data), (t1.ctypes.data, uv1.ctypes.data, p1.ctypes.data, 1, None)):
        assert lib.rl_rtiow_texture_values(world.device(), *a) == api.RL_E_INVALID
    rw = rl.RtcWorld.test_mirror_scene(30, 20)
    assert lib.rl_rtiow_scatter_rays(*args(sc=rw.device())) == api.RL_E_INVALID
    assert lib.rl_rtiow_texture_values(rw.device(), t1.ctypes.data, uv1.ctypes.data, p1.ctypes.data, 1, o1.ctypes.data) == api.RL_E_INVALID
    # word_pos >= 2^31
    for bad in (2 ** 31, 2 ** 40):
        with pytest.raises(rl.RLError) as e:
            world.scatter_rays(rays, hits, api.pack_cursors(np.arange(n, dtype=np.uint64), [0] * (n - 1) + [bad]), 5)
        assert e.value.code == api.RL_E_INVALID
    ok, _ = world.scatter_rays(rays, hits, api.pack_cursors(np.arange(n, dtype=np.uint64), 2 ** 31 - 9), 5)
    assert ok["scatter"].all()
    # a material index / texture id outside the table: refused before the launch by the host forms
    wild = hits.copy()
    wild["material"][5] = table.shape[0]
    with pytest.raises(rl.RLError) as e:
        world.scatter_rays(rays, wild, cur, 5)
    assert e.value.code == api.RL_E_INVALID
    with pytest.raises(rl.RLError) as e:
        world.texture_values([world.textures().shape[0]], np.zeros((1, 2)), np.zeros((1, 3)))
    assert e.value.code == api.RL_E_INVALID
    # ... and zeros from the device forms; hit == 0: zeros, cursor untouched; the output cursors may be the input's buffer
    want, want_cur = world.scatter_rays(rays, hits, cur, 5)
    assert want["scatter"].all()
    wild["material"][6] = 0xFFFFFFFF
    wild["hit"][3] = 0
    dev = "cuda:0"
    up = lambda a, w: torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], w).copy()).to(dev)  # noqa: E731
    d_r, d_h, d_c = up(rays, 56), up(wild, 88), up(cur, 16)
    d_o = torch.full((n, 112), 0x55, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    st = {}
    world.scatter_rays_device(d_r.data_ptr(), d_h.data_ptr(), d_c.data_ptr(), n, 5, d_o.data_ptr(), d_c.data_ptr(), stats=st)
    got = d_o.cpu().numpy().view(api.SCATTER).reshape(n)
    got_cur = d_c.cpu().numpy().view(api.RNG_CURSOR).reshape(n)
    zero = np.array([3, 5, 6])
    rest = np.array([0, 1, 2, 4, 7])
    assert not got[zero].view(np.uint8).any() and got_cur[zero].tobytes() == cur[zero].tobytes()
    assert got[rest].tobytes() == want[rest].tobytes() and got_cur[rest].tobytes() == want_cur[rest].tobytes()
    assert st["rays"] == 5 and st["rc"] == api.RL_OK
    miss = hits.copy()
    miss["hit"][[0, 4]] = 0
    rec, c2 = world.scatter_rays(rays, miss, cur, 5, stats=st)
    assert not rec[[0, 4]].view(np.uint8).any() and c2[[0, 4]].tobytes() == cur[[0, 4]].tobytes() and st["rays"] == n - 2
    d_t = torch.tensor([0, world.textures().shape[0], 2 ** 31], dtype=torch.int64, device=dev).to(torch.int32)
    d_uv, d_p = torch.zeros((3, 2), dtype=torch.float64, device=dev), torch.zeros((3, 3), dtype=torch.float64, device=dev)
    d_rgb = torch.full((3, 3), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    world.texture_values_device(d_t.data_ptr(), d_uv.data_ptr(), d_p.data_ptr(), 3, d_rgb.data_ptr())
    api.render_status(world)
    rgb = d_rgb.cpu().numpy()
    assert np.array_equal(rgb[0], world.texture_values([0], np.zeros((1, 2)), np.zeros((1, 3)))[0]) and not rgb[1:].any()
    # the panic site: one Dielectric element with dir = 0
    zr = rays.copy()
    zr["dir"][4] = 0.0
    st = {}
    rec, c2 = world.scatter_rays(zr, hits, cur, 5, stats=st, allow_degenerate=True)
    assert st["flagged"] == 1 and st["rc"] == api.RL_E_DEGENERATE
    with pytest.raises(rl.RLError) as e:
        world.scatter_rays(zr, hits, cur, 5)
    assert e.value.code == api.RL_E_DEGENERATE
    others = np.arange(n) != 4
    assert rec[others].tobytes() == want[others].tobytes() and c2[others].tobytes() == want_cur[others].tobytes()
    # ud = wd = 0: cos_theta = 0, sin_theta = 1, ri * 1 = 1 / 1.5: refraction possible, reflectance r0 + (1 - r0) * 1 = 1 > any draw: reflect, 0 - n * 0
    assert rec["scatter"][4] == 1 and not rec["scattered"]["dir"][4].any() and c2["word_pos"][4] == cur["word_pos"][4] + np.uint64(2)
    assert np.array_equal(rec["scattered"]["origin"][4], hits["p"][4]) and np.array_equal(rec["attenuation"][4], (1.0, 1.0, 1.0))


# ---------------------------------------------------------------------------------------------- 6: device forms
def test_device_forms_status_and_a_query_between_two_renders(rl, golden):
    """6: scatter_rays_device and texture_values_device on a side stream give the host forms' bytes; rl_render_status counts the query
    once; a query between two asynchronous renders changes neither the frames nor the accounting."""
    import torch
    api = rl.api
    case = _case(rl, golden, "golden_test_scene")
    world, p = case["world"], case["p"]
    hits = case[0]["got"][4][0]
    sel = np.flatnonzero(world.hit_rays(case[0]["rays"]["origin"], case[0]["rays"]["dir"], case[0]["rays"]["time"])["hit"] == 1)
    rays, cur = case[0]["rays"][sel], case[0]["cur"][sel]
    hits = hits.copy()
    hits["hit"][::7] = 0  # some misses: rays = elements with a hit
    n = hits.shape[0]
    want, want_cur = world.scatter_rays(rays, hits, cur, p.seed)
    dev = "cuda:0"
    up = lambda a, w: torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], w).copy()).to(dev)  # noqa: E731
    d_r, d_h, d_c = up(rays, 56), up(hits, 88), up(cur, 16)
    d_o = torch.zeros((n, 112), dtype=torch.uint8, device=dev)
    d_oc = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    world.scatter_rays_device(d_r.data_ptr(), d_h.data_ptr(), d_c.data_ptr(), n, p.seed, d_o.data_ptr(), d_oc.data_ptr(), stream=s2.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == int((hits["hit"] == 1).sum()) and st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert api.render_status(world)["rays"] == 0  # counted once
    assert d_o.cpu().numpy().tobytes() == want.tobytes() and d_oc.cpu().numpy().tobytes() == want_cur.tobytes()
    assert d_c.cpu().numpy().tobytes() == cur.tobytes()  # the input cursors are read only
    tex = (np.arange(n) % world.textures().shape[0]).astype(np.uint32)
    uv = np.ascontiguousarray(np.stack([hits["u"], hits["v"]], axis=1))
    pts = np.ascontiguousarray(hits["p"])
    want_rgb = world.texture_values(tex, uv, pts)
    d_t, d_uv, d_p = torch.from_numpy(tex.view(np.int32)).to(dev), torch.from_numpy(uv).to(dev), torch.from_numpy(pts).to(dev)
    d_rgb = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    world.texture_values_device(d_t.data_ptr(), d_uv.data_ptr(), d_p.data_ptr(), n, d_rgb.data_ptr(), stream=s2.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == 0 and st["rc"] == api.RL_OK
    assert d_rgb.cpu().numpy().tobytes() == want_rgb.tobytes()
    # between two asynchronous renders
    pr = rl.Camera(p).params
    pr.image_width, pr.samples_per_pixel = 96, 4
    cam = rl.Camera(pr)
    H, W = cam.c.image_height, cam.c.image_width
    gs = {}
    frame = cam.render(world, stats=gs).data
    a = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    b = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    d_o.zero_()
    d_oc.zero_()
    torch.cuda.synchronize()
    cam.render_device(world, a.data_ptr(), stream=s1.cuda_stream)
    world.scatter_rays_device(d_r.data_ptr(), d_h.data_ptr(), d_c.data_ptr(), n, p.seed, d_o.data_ptr(), d_oc.data_ptr(), stream=s2.cuda_stream)
    cam.render_device(world, b.data_ptr(), stream=s1.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == gs["rays"] and st["flagged"] == 0  # rays: of the most recently enqueued one, the second render
    assert np.array_equal(a.cpu().numpy(), frame) and np.array_equal(b.cpu().numpy(), frame)
    assert d_o.cpu().numpy().tobytes() == want.tobytes() and d_oc.cpu().numpy().tobytes() == want_cur.tobytes()
    assert api.render_status(world)["rays"] == 0
    # a flagged query reports through rl_render_status with every output written
    zr = rays.copy()
    k = int(np.flatnonzero((world.materials()["kind"][hits["material"]] == api.MAT_DIELECTRIC) & (hits["hit"] == 1))[0])
    zr["dir"][k] = 0.0
    ref, _ = world.scatter_rays(zr, hits, cur, p.seed, allow_degenerate=True)
    d_z = up(zr, 56)
    d_o.fill_(0x55)
    torch.cuda.synchronize()
    world.scatter_rays_device(d_z.data_ptr(), d_h.data_ptr(), d_c.data_ptr(), n, p.seed, d_o.data_ptr(), stream=s2.cuda_stream)
    stt = api.render_status(world, allow_degenerate=True)
    assert stt["rc"] == api.RL_E_DEGENERATE and stt["flagged"] == 1
    assert d_o.cpu().numpy().tobytes() == ref.tobytes()


# ---------------------------------------------------------------------------------------------- 7: the C++ mirror
@pytest.mark.skipif(bool(os.environ.get("RL_RENDER_LIB")), reason="the C++ host mirror links librl_render.so (the product library)")
def test_cpp_mirror_probe_agrees_with_the_python_path(rl, golden):
    api = rl.api
    Hh = api.host_lib()
    Hh.rlh_material_query_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    case = _case(rl, golden, "golden_test_scene")
    world, p = case["world"], case["p"]
    assert p.seed == rl.World.golden_test_scene().params.seed
    hits = np.ascontiguousarray(case[7]["got"][4][0][:300])
    sel = np.flatnonzero(world.hit_rays(case[7]["rays"]["origin"], case[7]["rays"]["dir"], case[7]["rays"]["time"])["hit"] == 1)[:300]
    rays, cur = np.ascontiguousarray(case[7]["rays"][sel]), case[7]["cur"][sel].copy()
    n = hits.shape[0]
    want, want_cur = world.scatter_rays(rays, hits, cur, p.seed)
    out = np.zeros(n, dtype=api.SCATTER)
    assert Hh.rlh_material_query_probe(0, rays.ctypes.data, hits.ctypes.data, cur.ctypes.data, n, out.ctypes.data) == 0, Hh.rlh_last_error()
    assert out.tobytes() == want.tobytes() and cur.tobytes() == want_cur.tobytes()
    tex = (np.arange(n) % world.textures().shape[0]).astype(np.uint32)
    uv = np.ascontiguousarray(np.stack([hits["u"], hits["v"]], axis=1))
    pts = np.ascontiguousarray(hits["p"])
    rgb = np.zeros((n, 3))
    assert Hh.rlh_material_query_probe(1, tex.ctypes.data, uv.ctypes.data, pts.ctypes.data, n, rgb.ctypes.data) == 0, Hh.rlh_last_error()
    assert rgb.tobytes() == world.texture_values(tex, uv, pts).tobytes()
