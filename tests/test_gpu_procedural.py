"""GPU tier: the procedural textures on the device against tests/procedural_model.py (the reference's text in mpmath, independent of
the oracle and the kernels); tests/test_procedural_model.py holds the same model to by-hand answers and the oracle to the model.

  a. Noise (perlin_noise, perlin_turb, texture_value<2>) through rl_rtiow_texture_values on scenes whose Perlin table is replaced by
     the hand-made and the asymmetric tables of the CPU tier.
  b. Checker beyond +-2^63: Rust's saturating `as i64`, flat and nested, against the restatement and the oracle.
  c. RTC patterns through prepare_rays' object_color, color_at_rays and a 12 x 8 render of ambient-only worlds: the pattern point is
     pattern.inverse * (object chain inverse * world point), decided in mpmath from the record's t.
"""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import procedural_model as P
from test_gpu_ray_query import _rtc_camera_rays
from test_procedural_model import AT_LOCAL, BLACK, IDENT, LIGHT, TURB7_BY_HAND, WHITE, _set_inverse, ambient_only, plane_world, probe_world
from test_rtc_solids_oracle import R, S, T, WorldBuilder

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module", autouse=True)
def _init(rl):
    rl.init(0)


# ----------------------------------------------------------------------------- a. Noise
SCALES = [0.0, 0.2, 4.0, 1e3, 1e6]  # 0: the argument is 10 turb alone, whatever z is
ARG_MAX = 1e9  # scale * z beyond this is left to the NaN / range checks: the argument's own rounding is then >= 1e-7
# The device sin (ocml, binary64) is not specified anywhere in this repository's reach, so its share is measured: the largest
# |value - model| - arithmetic bound over the arguments of this module (|arg| <= 1e9), in units of u = 2^-53 of the value
# 0.5 (1 + sin).  Measured on an MI355X: 0.442 u, at sin(7.12e8) (sin_points(), where nothing but sin and the rounding of 1 + sin is
# left): sin itself is within 0.89 u = 0.89 ulp there.  The tests allow twice the measured figure, the argument set being a finite sample.
SIN_U_MEASURED = 0.442
SIN_ALLOWED = 2.0 * SIN_U_MEASURED * P.U


class NoiseScene:
    """A one-sphere Noise world's description with its Perlin table replaced and one Noise texture per scale, created through the C ABI"""

    def __init__(self, rl, table):
        api = rl.api
        self.api, self.L = api, api.render_lib()
        self.world = rl.World.build(lambda b: b.list([b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian(b.noise(4.0, 1)))]))
        base = self.world.textures()
        assert base.shape == (1,) and base[0]["kind"] == api.TEX_NOISE and base[0]["image"] == 0 and self.world.perlins().shape == (1,)
        self.textures = np.repeat(base, len(SCALES))
        self.textures["inv_scale"] = SCALES  # a Noise texture keeps its scale here
        self.table = np.ascontiguousarray(table.astype(api.PERLIN))
        d = api.RtiowSceneDesc.from_buffer_copy(api.RtiowSceneDesc.from_address(self.world.desc))
        d.textures, d.n_textures, d.perlins = self.textures.ctypes.data, len(SCALES), self.table.ctypes.data
        self.desc = d
        self.handle = self.L.rl_rtiow_scene_create(C.addressof(d))
        assert self.handle, self.L.rl_last_error().decode()

    def values(self, tex, pts):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        n = pts.shape[0]
        tex = np.ascontiguousarray(np.broadcast_to(np.asarray(tex, dtype=np.uint32), (n,)))
        uv, rgb = np.zeros((n, 2)), np.zeros((n, 3))
        assert self.L.rl_rtiow_texture_values(self.handle, tex.ctypes.data, uv.ctypes.data, pts.ctypes.data, n, rgb.ctypes.data) == 0
        assert np.array_equal(rgb[:, 0], rgb[:, 1], equal_nan=True) and np.array_equal(rgb[:, 1], rgb[:, 2], equal_nan=True)
        return rgb[:, 0].copy()

    def close(self):
        self.L.rl_scene_destroy(self.handle)
        self.handle = None


def sin_points():
    """lattice points: every octave of turb is an exact 0 there, so the argument is the one product scale * z and the value 0.5 (1 + sin)
    of an argument known to the last bit: what is left beside sin's own error is the rounding of 1 + sin.  z over the integers up to
    +-1000: arguments up to 1e9 at scale 1e6"""
    rng = np.random.default_rng(4242)
    z = np.concatenate([rng.integers(-1000, 1001, 150), [1000, -1000, 999, 1, -1]]).astype(np.float64)
    return np.stack([rng.integers(-300, 300, z.size).astype(np.float64), rng.integers(-300, 300, z.size).astype(np.float64), z], axis=1)


_MODEL = {}


def noise_model():
    """per random table: the model's turb(p, 7) of every point, once per module"""
    if not _MODEL:
        pts, bad = P.perlin_points()
        pts = np.concatenate([pts, sin_points()])
        _MODEL["pts"], _MODEL["bad"], _MODEL["tables"] = pts, bad, P.random_tables()
        _MODEL["turb"] = [[P.turb(tab[0], q, 7) for q in pts] for tab in _MODEL["tables"]]
    return _MODEL


def test_noise_by_hand(rl):
    """Texture::value is the only view of turb the library gives, and sin keeps == out of reach unless turb is 0: there the value is 0.5
    exactly.  Everywhere else the by-hand turb(p, 7) of the CPU tier goes through sin in mpmath: 0.5 (1 + sin(10 turb)) at scale 0, within
    the arithmetic bound and the sin allowance.  A slip in the hashing or the weights moves turb by 1e-2 and more."""
    zero = 0
    for rows, p, turb7 in TURB7_BY_HAND:
        scene = NoiseScene(rl, P.lattice_table(rows))
        try:
            got = float(scene.values(0, [p])[0])
        finally:
            scene.close()
        with mp.workdps(P.DPS):
            want = float((1 + mp.sin(10 * mp.mpf(turb7))) / 2)
        model, bound, _ = P.noise_value(P.lattice_table(rows)[0], 0.0, p)
        assert abs(model - want) <= P.U, (rows["vectors"], p, model, want)
        if turb7 == 0.0:
            zero += 1
            assert got == 0.5, (rows["vectors"], p, got)
        assert abs(got - want) <= bound + SIN_ALLOWED, (rows["vectors"], p, got, want, (got - want) / P.U)
    assert zero >= 2


@pytest.mark.parametrize("which", [0, 1])
def test_noise_meets_the_model(rl, which):
    """the point set of the CPU tier at every scale whose argument stays within ARG_MAX; non-finite points and arguments give NaN"""
    m = noise_model()
    pts, bad, tab = m["pts"], m["bad"], m["tables"][which]
    scene = NoiseScene(rl, tab)
    try:
        got = [scene.values(k, pts) for k in range(len(SCALES))]
        got_bad = [scene.values(k, bad) for k in range(len(SCALES))]
        huge = scene.values(2, [(0.5, 0.5, 1e308)])  # 4 * 1e308 overflows: sin(inf)
        # batches of 1, 64 and 65, each lane with a texture of its own choosing
        order = np.arange(65) % len(SCALES)
        for n in (1, 64, 65):
            part = scene.values(order[:n], pts[:n])
            assert np.array_equal(part, np.array([got[order[i]][i] for i in range(n)]), equal_nan=True), n
    finally:
        scene.close()
    rows = []  # (|d|, arithmetic bound, scale, point, value, model, argument)
    n_general = len(P.perlin_points()[0])  # sin_points() follow
    for k, scale in enumerate(SCALES):
        assert np.isnan(got_bad[k]).all(), (scale, got_bad[k])
        for i, q in enumerate(pts):
            if abs(scale * q[2]) > ARG_MAX:
                assert 0.0 <= got[k][i] <= 1.0, (scale, tuple(q), got[k][i])
                continue
            want, bound, arg = P.noise_value(tab[0], scale, q, turb7=m["turb"][which][i])
            if i >= n_general:
                # turb is 0 to within underflow, so 10 * turb vanishes against scale * z, the sum is that one product as binary64 computes
                # it, and only 1 + sin rounds: the model's bound, which charges the product and the sum a rounding each, is replaced
                assert m["turb"][which][i][0] == 0.0 and m["turb"][which][i][1] < 1e-300
                with mp.workdps(P.DPS):
                    arg = scale * q[2]
                    sn = mp.sin(mp.mpf(arg))
                    want, bound = float((1 + sn) / 2), float(P.U * abs(1 + sn) / 2)
            rows.append((abs(got[k][i] - want), bound, scale, tuple(q), got[k][i], want, arg))
    assert np.isnan(huge[0])
    worst = max(rows, key=lambda r: r[0] - r[1])
    print(f"table {which}: {len(rows)} values; worst |d| / (bound + allowance) {max(r[0] / (r[1] + SIN_ALLOWED) for r in rows):.3f}; "
          f"largest (|d| - arithmetic bound) / u = {(worst[0] - worst[1]) / P.U:.3f} at scale {worst[2]} p {worst[3]} arg {worst[6]!r}; "
          f"largest |d| / u = {max(r[0] for r in rows) / P.U:.3f}")
    assert worst[0] <= worst[1] + SIN_ALLOWED, worst
    assert len(rows) >= 4 * len(pts)


# ----------------------------------------------------------------------------- b. Checker beyond +-2^63
COLOURS = [(0.1, 0.2, 0.3), (0.9, 0.8, 0.7), (0.5, 0.25, 0.125), (0.0, 1.0, 0.0)]
BELOW = float(np.nextafter(2.0 ** 63, 0.0))
EDGES = [BELOW, 2.0 ** 63, 1e19, 1e300, INF, -(2.0 ** 63), -1e19, -INF, NAN, -BELOW, 2.0 ** 53 + 2.0, 2.0 ** 62]


def _checker_points():
    pts = []
    for axis in range(3):
        for x in EDGES:
            for other in ((0.1, 0.1), (0.1, 1.5), (1.5, 0.1), (1.5, 1.5)):
                q = [other[0], other[1]]
                q.insert(axis, x)
                pts.append(tuple(q))
    # two and three saturated axes: i64::MAX + i64::MAX wraps to -2 (even), + i64::MAX again to 2^63 - 3 (odd); MAX + MIN = -1
    big = [(1e19, 1e19, 0.1), (1e19, 1e19, 1.5), (1e19, 1e19, 1e19), (1e19, -1e19, 0.1), (INF, -INF, 1.5), (-1e19, -1e19, 1.5), (INF, INF, INF),
           (2.0 ** 63, BELOW, 0.1)]
    return np.array(pts + big + [tuple(q) for q in np.random.default_rng(8).uniform(-3.0, 3.0, (24, 3))])  # ordinary points: every leaf


@pytest.mark.parametrize("nested", [False, True])
def test_checker_saturates_as_rust_does(rl, oracle, nested):
    a, b, c, d = COLOURS
    tree = ((1.0,), a, ((0.5,), ((2.0,), c, b), d)) if nested else ((1.0,), a, b)

    def fn(bld):
        def tex(t):
            return bld.solid(t) if isinstance(t[0], float) else bld.checker(t[0][0], tex(t[1]), tex(t[2]))
        return bld.list([bld.sphere((0.0, 0.0, 0.0), 1.0, bld.lambertian(tex(tree)))])

    world = rl.World.build(fn)
    root = int(world.materials()["texture"][0])
    pts = _checker_points()
    want = np.array([P.checker_leaf(tree, q) for q in pts])
    assert len({tuple(w) for w in want.tolist()}) == (4 if nested else 2)
    ref = np.array([oracle.texture_value(world.desc, root, 0.0, 0.0, q) for q in pts])
    assert np.array_equal(ref, want), pts[np.flatnonzero((ref != want).any(axis=1))]
    got = world.texture_values(np.full(len(pts), root, dtype=np.uint32), np.zeros((len(pts), 2)), pts)
    wrong = np.flatnonzero((got != want).any(axis=1))
    assert wrong.size == 0, [(tuple(pts[i]), tuple(got[i]), tuple(want[i])) for i in wrong[:8]]


# ----------------------------------------------------------------------------- c. RTC patterns
KINDS = ["PAT_STRIPE", "PAT_RING", "PAT_GRADIENT", "PAT_CHECKER3D"]
SHAPES = ["O_PLANE", "O_CUBE", "O_SPHERE"]
DEPTHS = [0, 1, 3, 8]
CA, CB = (0.9, 0.3, 0.1), (0.1, 0.8, 0.35)


def _link(i):
    """translate . rotate . non-uniform scale, another one per level"""
    return T(0.3 - 0.1 * i, 0.2 * ((i % 3) - 1), -0.25 + 0.07 * i) @ R(i % 3, 0.35 + 0.4 * i) @ S(1.0 + 0.06 * ((i % 4) - 1.5), 0.9 + 0.05 * (i % 3), 1.1 - 0.04 * (i % 5))


def _pattern_world(rl, kind, shape, depth, pattern_transform):
    """-> (world, pattern inverse as stored, chain inverses as stored, outermost first, chain matrix)"""
    api = rl.api
    b = WorldBuilder(api)
    pat = b.pattern(kind, CA, CB, pattern_transform)
    node = b.shape(shape, material=ambient_only(b, pat))
    chain = [_link(i) for i in range(depth)]
    total = np.eye(4)
    for m in chain:
        total = total @ m
    for m in reversed(chain):
        node = b.xf(m, node)
    centre = total[:3, 3]
    cam = api.rtc_camera(12, 8, 1.0, tuple(centre + np.array([1.2, 1.6, -2.8])), tuple(centre), (0, 1, 0))
    world = b.world(rl, [node], lights=LIGHT, camera=cam)
    return world, b.pats[0]["inverse"].copy(), [b.tr[k]["inverse"].copy() for k in range(depth - 1, -1, -1)], total


def _rays_at(rng, api, shape, total, n):
    if shape == api.O_PLANE:
        local = np.stack([rng.uniform(-6, 6, n), np.zeros(n), rng.uniform(-6, 6, n)], axis=1)
        away = np.stack([rng.uniform(-1, 1, n), rng.uniform(0.5, 2, n) * rng.choice([-1.0, 1.0], n), rng.uniform(-1, 1, n)], axis=1)
    elif shape == api.O_CUBE:
        local = rng.uniform(-1, 1, (n, 3))
        face = rng.integers(0, 3, n)
        local[np.arange(n), face] = rng.choice([-1.0, 1.0], n)
        away = local * rng.uniform(1.5, 3.0, (n, 1)) + rng.uniform(-0.5, 0.5, (n, 3))
    else:
        local = rng.normal(size=(n, 3))
        local /= np.linalg.norm(local, axis=1, keepdims=True)
        away = local * rng.uniform(1.5, 3.0, (n, 1)) + rng.uniform(-0.5, 0.5, (n, 3))
    target = local @ total[:3, :3].T + total[:3, 3]
    origin = (local + away) @ total[:3, :3].T + total[:3, 3]
    return origin, target - origin


def _decide(kind, pinv, chain, o, d, t):
    """-> (colour, margin, bound): the model at the exact o + t d, and how far binary64 can put the decided quantity from the true one.
    t is the record's own, pinned bit for bit to the oracle's elsewhere: the kernel forms its local point from the same t, so t adds
    nothing beyond the |t| * (direction's bound) inside local_point_bound.  A ring decides on sqrt(x^2 + z^2): its derivative in x and z is
    at most 1 each, and two products, a sum and the square root round: 2 * bound + 4 u r."""
    with mp.workdps(P.DPS):
        wp = [mp.mpf(float(o[k])) + mp.mpf(float(t)) * mp.mpf(float(d[k])) for k in range(3)]
        colour, second = P.rtc_pattern_at(kind, CA, CB, pinv, chain, wp)
        bound = P.local_point_bound(pinv, chain, o, d, t)
        if kind == P.RING:
            x, _, z = P.pattern_point(pinv, chain, wp)
            bound = 2 * bound + 4 * P.U * float(mp.sqrt(x * x + z * z))
    return colour, second, bound


@pytest.mark.parametrize("kind_name", KINDS)
def test_rtc_patterns_meet_the_model(rl, kind_name):
    api = rl.api
    kind = getattr(api, kind_name)
    ki = KINDS.index(kind_name)
    n = 280
    for si, shape_name in enumerate(SHAPES):
        shape, depth = getattr(api, shape_name), DEPTHS[(ki + si) % 4]
        ptf = T(0.15, -0.2, 0.1) @ R(1, 0.6 + 0.2 * si) @ S(0.35, 0.5, 0.45)
        world, pinv, chain, total = _pattern_world(rl, kind, shape, depth, ptf)
        rng = np.random.default_rng(100 * ki + si)
        o, d = _rays_at(rng, api, shape, total, n)
        co, cd = _rtc_camera_rays(world.camera)
        o, d = np.concatenate([o, co]), np.concatenate([d, cd])
        comps = world.prepare_rays(o, d)
        rgb = world.color_at_rays(o, d)
        hit = comps["hit"] == 1
        assert int(hit[:n].sum()) >= 0.9 * n, (shape_name, int(hit[:n].sum()))
        # ambient 1, diffuse = specular = 0, one white light: color_at is the pattern colour, and the void colour is black
        assert np.array_equal(rgb[hit], comps["object_color"][hit]) and not rgb[~hit].any()
        frame = world.render(1)
        assert frame.shape == (8, 12, 3) and np.array_equal(frame.reshape(-1, 3), rgb[n:])
        assert int(hit[n:].sum()) >= 10, (shape_name, int(hit[n:].sum()))
        left_out, decided, worst = 0, {tuple(CA): 0, tuple(CB): 0}, 0.0
        for i in np.flatnonzero(hit):
            colour, second, bound = _decide(kind, pinv, chain, o[i], d[i], comps["t"][i])
            got = comps["object_color"][i]
            if kind == P.GRADIENT:
                own, margin = second
                if margin <= bound:
                    left_out += 1
                    continue
                allowed = own + max(abs(cb - ca) for ca, cb in zip(CA, CB)) * bound
                worst = max(worst, float(np.abs(got - colour).max()) / allowed)
                assert np.abs(got - colour).max() <= allowed, (shape_name, depth, i, got, colour, allowed)
            else:
                if second <= bound:
                    left_out += 1
                    continue
                decided[tuple(colour)] += 1
                assert tuple(got) == tuple(colour), (shape_name, depth, i, tuple(got), tuple(colour), second, bound)
        total_hits = int(hit.sum())
        print(f"{kind_name} {shape_name} depth {depth}: {total_hits} hits, left out {left_out}, decided {list(decided.values())}, worst / allowed {worst:.3f}")
        assert left_out <= 0.01 * total_hits, (shape_name, left_out)
        if kind != P.GRADIENT:
            assert min(decided.values()) >= 50, (shape_name, decided)


def test_the_references_pattern_tables_on_the_device(rl):
    """the rows of stripe.rs, ring.rs, gradient.rs and checker3d.rs (tests/test_procedural_model.py AT_LOCAL) and the probe cases of
    pattern/mod.rs and transformed.rs, with =="""
    api = rl.api
    for name, rows in AT_LOCAL.items():
        for point, want in rows:
            world = plane_world(rl, getattr(api, name), WHITE, BLACK, T(0.0, float(point[1]), 0.0))
            o, d = [(float(point[0]), 1.0, float(point[2]))], [(0.0, -1.0, 0.0)]
            comps = world.prepare_rays(o, d)
            assert comps["hit"][0] == 1 and comps["t"][0] == 1.0 and tuple(comps["object_color"][0]) == tuple(want), (name, point, comps["object_color"][0])
            assert tuple(world.color_at_rays(o, d)[0]) == tuple(want), (name, point)
    for axis, (w0, w1, w2) in enumerate(zip((0.625, 0.5, 0.75), (0.5625, 0.59375, 0.375), (0.5, 0.46875, 0.1875))):
        world = probe_world(rl, api.O_PLANE, [], S(2, 2, 2), axis)[0]
        assert tuple(world.prepare_rays([(2.0, 1.0, 4.0)], [(0.0, -1.0, 0.0)])["object_color"][0]) == (w0,) * 3, axis
        for ptf, want in ((IDENT, w1), (T(0.5, 1, 1.5), w2)):
            world = probe_world(rl, api.O_CUBE, [S(2, 2, 2)], ptf, axis)[0]
            comps = world.prepare_rays([(1.0, 1.5, -5.0)], [(0.0, 0.0, 1.0)])
            assert comps["t"][0] == 3.0 and tuple(comps["object_color"][0]) == (want,) * 3, (axis, comps["object_color"][0])
            assert tuple(world.color_at_rays([(1.0, 1.5, -5.0)], [(0.0, 0.0, 1.0)])[0]) == (want,) * 3, axis


# (pattern kind, pattern inverse as a diagonal, object scale, (x, z) of the ray straight down from y = 1) -> a (True) or b (False).
# Everything is a power of two or a short dyadic: the pattern point is exact, and so is the answer.
A, B = True, False
DIRECTED = [
    # stripe boundaries: floor(x) even -> a.  -0.0 floors to -0.0, which casts to 0; -1.0 is odd (-1 % 2 = -1 != 0)
    ("PAT_STRIPE", (1, 1, 1), 1, [((0.0, 0.0), A), ((-0.0, 0.0), A), ((1.0, 0.0), B), ((-1.0, 0.0), B), ((2.0, 3.0), A), ((-2.0, 0.0), A), ((-0.5, 0.0), B),
                                 ((1.5, 0.0), B), ((-1.5, 0.0), A)]),
    # pattern scaled by 2 (inverse 1/2): x = 2 is the pattern's 1; object scaled by 4 on top: x = 8 is the pattern's 1
    ("PAT_STRIPE", (0.5, 0.5, 0.5), 1, [((2.0, 0.0), B), ((1.0, 0.0), A), ((-2.0, 0.0), B), ((4.0, 0.0), A), ((-0.0, 0.0), A)]),
    ("PAT_STRIPE", (0.5, 0.5, 0.5), 4, [((8.0, 0.0), B), ((4.0, 0.0), A), ((-8.0, 0.0), B), ((-4.0, 0.0), B), ((16.0, 0.0), A)]),
    # checker3d on the plane: y = 1 - 1 * 1 = 0 exactly, floor 0; floors summed
    ("PAT_CHECKER3D", (1, 1, 1), 1, [((0.0, 0.0), A), ((-0.0, -0.0), A), ((1.0, 0.0), B), ((1.0, 1.0), A), ((-1.0, 0.0), B), ((-1.0, 1.0), A), ((-1.0, -1.0), A),
                                    ((0.5, -0.5), B), ((-0.5, -0.5), A), ((2.0, -1.0), B)]),
    ("PAT_CHECKER3D", (0.25, 0.25, 0.25), 2, [((8.0, 0.0), B), ((8.0, 8.0), A), ((-8.0, 0.0), B), ((4.0, 0.0), A), ((-4.0, 0.0), B)]),
    ("PAT_RING", (1, 1, 1), 1, [((0.0, 0.0), A), ((1.0, 0.0), B), ((0.0, -1.0), B), ((-2.0, 0.0), A), ((3.0, 4.0), B), ((-0.0, -0.0), A), ((0.0, 2.0), A)]),
    # saturation with sane geometry: the pattern x is p.x * 2^70 exactly; 2^69 casts to i64::MAX, odd: b; -2^69 to i64::MIN, even: a
    ("PAT_STRIPE", (2.0 ** 70, 1, 1), 1, [((0.5, 0.25), B), ((-0.5, 0.25), A), ((0.0, 0.25), A), ((2.0 ** -8, 0.0), A), ((2.0 ** -7, 0.0), B)]),
    ("PAT_CHECKER3D", (2.0 ** 70, 1, 1), 1, [((0.5, 0.25), B), ((-0.5, 0.25), A), ((0.5, 1.25), B), ((-0.5, 1.25), A), ((0.0, 1.25), B)]),
    ("PAT_RING", (2.0 ** 70, 1, 2.0 ** 70), 1, [((0.5, 0.0), B), ((-0.5, 0.0), B), ((0.0, 0.5), B), ((0.0, 0.0), A)]),
]


def test_directed_pattern_boundaries_and_saturation(rl, oracle):
    """by hand first: the model and the oracle are held to the table, then the device, all with ==.  2^-8 * 2^70 = 2^62 is still an i64,
    and even; 2^-7 * 2^70 = 2^63 saturates to the odd i64::MAX.  checker3d adds the floors as f64 first: -2^69 + 1 rounds back to -2^69."""
    api = rl.api
    for name, diag, scale, rows in DIRECTED:
        kind = getattr(api, name)
        pinv = np.diag([float(diag[0]), float(diag[1]), float(diag[2]), 1.0])
        b = WorldBuilder(api)
        pat = b.pattern(kind, CA, CB, IDENT)
        _set_inverse(b, pat, pinv)
        node = b.shape(api.O_PLANE, material=ambient_only(b, pat))
        chain = []
        if scale != 1:
            node = b.xf(S(scale, scale, scale), node)
            chain = [b.tr[0]["inverse"].copy()]
        world = b.world(rl, [node], lights=LIGHT)
        o = np.array([(x, 1.0, z) for (x, z), _ in rows])
        d = np.tile((0.0, -1.0, 0.0), (len(rows), 1))
        want = np.array([CA if w else CB for _, w in rows])
        model = np.array([P.rtc_pattern_at(kind, CA, CB, pinv, chain, (x, 0.0, z))[0] for (x, z), _ in rows])
        assert np.array_equal(model, want), (name, diag, [rows[i][0] for i in np.flatnonzero((model != want).any(axis=1))])
        ref = np.array([oracle.rtc_color_at(world.desc, o[i], d[i]) for i in range(len(rows))])
        assert np.array_equal(ref, want), (name, diag, [rows[i][0] for i in np.flatnonzero((ref != want).any(axis=1))])
        comps = world.prepare_rays(o, d)
        assert (comps["hit"] == 1).all() and (comps["t"] == 1.0).all()
        bad = np.flatnonzero((comps["object_color"] != want).any(axis=1))
        assert bad.size == 0, (name, diag, scale, [rows[i][0] for i in bad])
        assert np.array_equal(world.color_at_rays(o, d), want), (name, diag, scale)
