"""GPU tier: the seeded hit queries (World.hit_rays_seeded = Hittable::hit for rays that carry an RNG cursor, scenes with ConstantMedium
objects included; include/rl_render.h).

Yardsticks are what this feature does not touch: the library's ray_color_rays (pinned to the renders and, through them, to the oracle by
the path-query tests), hit_rays and scatter_rays, the oracle's render counters, and answers worked out by hand on the oracle's ChaCha8
draws."""
import ctypes as C
import math
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INF = float("inf")
SCENES = ["cornell_smoke", "final_scene", "smoke_room"]
COUNTERS = ("node_tests", "sphere_tests", "planar_tests", "instance_enters")


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


def _synthetic_image():
    y, x = np.mgrid[0:12, 0:20]
    return np.stack([(x * 13) % 256, (y * 21) % 256, ((x + y) * 7) % 256], axis=-1).astype(np.uint8)


def _smoke_room(b):
    """examples/cornell_smoke.rs in miniature (tests/test_constant_medium.py::_smoke_scene restated): a room of quads, a light, two rotated /
    translated boxes of smoke, plus final_scene.rs's glass ball with a medium inside."""
    white = b.lambertian(b.solid((0.73, 0.73, 0.73)))
    green = b.lambertian(b.solid((0.12, 0.45, 0.15)))
    red = b.lambertian(b.solid((0.65, 0.05, 0.05)))
    light = b.diffuse_light(b.solid((7, 7, 7)))

    def box(lo, hi, m):
        (x0, y0, z0), (x1, y1, z1) = lo, hi
        dx, dy, dz = (x1 - x0, 0, 0), (0, y1 - y0, 0), (0, 0, z1 - z0)
        return b.list([b.quad((x0, y0, z1), dx, dy, m), b.quad((x1, y0, z1), (0, 0, -(z1 - z0)), dy, m), b.quad((x1, y0, z0), (-(x1 - x0), 0, 0), dy, m),
                       b.quad((x0, y0, z0), dz, dy, m), b.quad((x0, y1, z1), dx, (0, 0, -(z1 - z0)), m), b.quad((x0, y0, z0), dx, dz, m)])
    room = [b.quad((555, 0, 0), (0, 555, 0), (0, 0, 555), green), b.quad((0, 0, 0), (0, 555, 0), (0, 0, 555), red),
            b.quad((113, 554, 127), (330, 0, 0), (0, 0, 305), light), b.quad((0, 555, 0), (555, 0, 0), (0, 0, 555), white),
            b.quad((0, 0, 0), (555, 0, 0), (0, 0, 555), white), b.quad((0, 0, 555), (555, 0, 0), (0, 555, 0), white)]
    box1 = b.translate(b.rotate_y(box((0, 0, 0), (165, 330, 165), white), 15.0), (265, 0, 295))
    box2 = b.translate(b.rotate_y(box((0, 0, 0), (165, 165, 165), white), -18.0), (130, 0, 65))
    smoke1 = b.constant_medium(box1, 0.01, b.isotropic(b.solid((0, 0, 0))))
    smoke2 = b.constant_medium(box2, 0.01, b.isotropic(b.solid((1, 1, 1))))
    ball = b.sphere((400, 90, 120), 60, b.dielectric(1.5))
    haze = b.constant_medium(b.sphere((400, 90, 120), 60, b.dielectric(1.5)), 0.2, b.isotropic(b.solid((0.2, 0.4, 0.9))))
    return b.bvh(room + [smoke1, smoke2, ball, haze])


def _room_params(rl, max_depth):
    return rl.CameraParams(aspect_ratio=1.0, image_width=48, samples_per_pixel=1, max_depth=max_depth, vfov=40.0, lookfrom=(278, 278, -800),
                           lookat=(278, 278, 0), background=(0, 0, 0), seed=5)


def _frame(rl, cam, pos):
    """The frame's camera rays: cursors (x * W + y, pos) through get_rays -> (cursors before, rays, cursors behind get_rays)."""
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), W)
    cur0 = rl.api.pack_cursors(x * np.uint64(W) + y, pos)
    rays, cur = cam.get_rays(x, y, cur0)
    return cur0, rays, cur


def _compose(world, p, rays, cur, counting):
    """ray_color (camera.rs:232-260) as a host loop over hit_rays_seeded and scatter_rays.  Only live paths are passed on, so the batch
    shrinks and every path changes its place in it from bounce to bounce.  -> colours, final cursors, per-path ray counts, the words the
    seeded hits consumed and the words the scatter calls consumed (counting: from the calls' stats; else from the cursors)."""
    n = rays.shape[0]
    bg = np.array(p.background, dtype=np.float64)
    total, thr = np.zeros((n, 3)), np.ones((n, 3))
    counts = np.zeros(n, dtype=np.uint32)
    out_cur = cur.copy()
    live = np.arange(n)
    r, c = rays.copy(), cur.copy()
    hit_words = scatter_words = 0
    for _ in range(p.max_depth):
        if live.size == 0:
            break
        st = {} if counting else None
        hits, c2 = world.hit_rays_seeded(r, c, p.seed, tmin=1e-10, stats=st, allow_degenerate=True)
        assert np.array_equal(c2["stream"], c["stream"])
        moved = int((c2["word_pos"] - c["word_pos"]).sum(dtype=np.uint64))
        if counting:
            assert st["rays"] == live.size and st["rng_words"] == moved, (st, moved)
        hit_words += moved
        c = c2
        out_cur[live] = c  # (a path that leaves a medium unscattered and then misses has consumed its draw all the same)
        counts[live] += 1
        miss = hits["hit"] == 0
        total[live[miss]] = total[live[miss]] + thr[live[miss]] * bg
        live, r, c, hits = live[~miss], r[~miss], c[~miss], hits[~miss]
        if live.size == 0:
            break
        st = {}
        rec, c = world.scatter_rays(r, hits, c, p.seed, stats=st, allow_degenerate=True)
        scatter_words += st["rng_words"]
        total[live] = total[live] + thr[live] * rec["emitted"]
        out_cur[live] = c
        go = rec["scatter"] == 1
        thr[live[go]] = thr[live[go]] * rec["attenuation"][go]
        live, r, c = live[go], np.ascontiguousarray(rec["scattered"][go]), c[go]
    return total, out_cur, counts, hit_words, scatter_words


_WORLDS = {}


def _world(rl, name):
    """(world, camera params at a 48-wide frame, max_depth <= 20), built once."""
    if name not in _WORLDS:
        if name == "smoke_room":
            w, p = rl.World.build(_smoke_room), _room_params(rl, 20)
        else:
            w = rl.World.example_scene(name, rgb8=_synthetic_image()) if name == "final_scene" else rl.World.example_scene(name)
            p = w.params
            p.image_width, p.samples_per_pixel = 48, 1
            p.max_depth = min(p.max_depth, 20)
        _WORLDS[name] = (w, p)
    return _WORLDS[name]


# ---------------------------------------------------------------------------------------------- 1: composition
@pytest.mark.parametrize("name", SCENES)
def test_composition_of_hit_rays_seeded_and_scatter_rays_equals_ray_color_rays(rl, name):
    """1: on scenes with ConstantMedium objects, colours, final cursors and per-path ray counts byte-equal to ray_color_rays, with cursors at
    word 0 (counting seeded hits) and at word 7 (counter-free ones); seeded-hit words + scatter words = the rng_words of a counting
    ray_color_rays; the same with the fast traversal switched off."""
    api = rl.api
    world, p = _world(rl, name)
    assert world.counts()["media"] > 0
    cam = rl.Camera(p)
    got7 = rays7 = cur7 = None
    for pos in (0, 7):
        _, rays, cur = _frame(rl, cam, pos)
        st = {}
        w_rgb, w_cur, w_counts = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays, stats=st, allow_degenerate=True)
        rgb, o_cur, counts, hit_words, scatter_words = got = _compose(world, p, rays, cur, counting=(pos == 0))
        print(name, "word_pos", pos, "paths", rgb.shape[0], "rays", int(counts.sum()), "seeded-hit words", hit_words, "scatter words", scatter_words)
        assert rgb.tobytes() == w_rgb.tobytes(), (name, pos, np.abs(rgb - w_rgb).max())
        assert o_cur.tobytes() == w_cur.tobytes(), (name, pos)
        assert counts.tobytes() == w_counts.tobytes(), (name, pos)
        assert hit_words + scatter_words == st["rng_words"], (name, pos, hit_words, scatter_words, st["rng_words"])
        assert hit_words > 0, name  # some ray of the frame does reach a medium
        if pos == 7:
            got7, rays7, cur7 = got, rays, cur
    # the counter-free ray_color_rays: the fast walk with media where the scene has a fast tree, and, with the switch off, the
    # counter-free reference-order kernel; the loop is held against both, and against itself with the switch off
    fast = world.ray_color_rays(None, None, None, cur7, p.seed, p.max_depth, p.background, rays=rays7, allow_degenerate=True)
    served = api.last_query()["kernel"]
    api.set_fast_traversal(False)
    try:
        off = _compose(world, p, rays7, cur7, counting=False)
        slow = world.ray_color_rays(None, None, None, cur7, p.seed, p.max_depth, p.background, rays=rays7, allow_degenerate=True)
        assert api.last_query()["kernel"] == "reference"
    finally:
        api.set_fast_traversal(True)
    print(name, "counter-free ray_color_rays served by", served)
    for a, b, c, d in zip(off[:3], got7[:3], fast, slow):
        assert a.tobytes() == b.tobytes() and c.tobytes() == b.tobytes() and d.tobytes() == b.tobytes(), name


# ---------------------------------------------------------------------------------------------- 2: oracle counters
def test_counting_seeded_hit_reports_the_oracles_counters(rl, oracle):
    """2: the depth-1, one-sample frame of the miniature smoke room: the counting seeded hit of its camera rays reports rays = n and the
    oracle render's traversal counters (a depth-1 path is one Hittable::hit); get_rays words + seeded-hit words + scatter_rays words are the
    oracle's rng_words; the counter-free call gives the same bytes."""
    world = rl.World.build(_smoke_room)
    p = _room_params(rl, 1)
    cam = rl.Camera(p)
    cur0, rays, cur = _frame(rl, cam, 0)
    n = rays.shape[0]
    cs = {}
    oracle.rtiow_render(world.desc, cam.c, stats=cs)
    st = {}
    hits, cur2 = world.hit_rays_seeded(rays, cur, p.seed, stats=st)
    print("oracle", {k: cs[k] for k in COUNTERS + ("rays", "rng_words")}, "seeded hit", {k: st[k] for k in COUNTERS + ("rays", "rng_words")})
    assert st["rays"] == n == cs["rays"] and st["flagged"] == 0
    for k in COUNTERS:
        assert st[k] == cs[k], (k, st[k], cs[k])
    assert st["instance_enters"] > 0 and st["planar_tests"] > 0 and st["sphere_tests"] > 0
    get_words = int((cur["word_pos"] - cur0["word_pos"]).sum(dtype=np.uint64))
    assert st["rng_words"] == int((cur2["word_pos"] - cur["word_pos"]).sum(dtype=np.uint64)) and st["rng_words"] > 0
    hit = hits["hit"] == 1
    ss = {}
    world.scatter_rays(rays[hit], hits[hit], cur2[hit], p.seed, stats=ss)
    assert get_words + st["rng_words"] + ss["rng_words"] == cs["rng_words"], (get_words, st["rng_words"], ss["rng_words"], cs["rng_words"])
    free, free_cur = world.hit_rays_seeded(rays, cur, p.seed)
    assert rl.api.last_query()["kernel"] == "reference"
    assert free.tobytes() == hits.tobytes() and free_cur.tobytes() == cur2.tobytes()


# ---------------------------------------------------------------------------------------------- 3: known answers
DENSITY = 0.4
SEED = 2024


def _slab(rl, opaque=None):
    """The unit-sphere slab at (0, 0, -5), density 0.4; opaque: "before" / "after" lists a Lambertian sphere of radius 0.5 at z = -2 in the
    world's list before / after the medium."""
    def scene(b):
        medium = b.constant_medium(b.sphere((0, 0, -5), 1.0, b.flat()), DENSITY, b.isotropic(b.solid((1.0, 1.0, 1.0))))
        if opaque is None:
            return b.list([medium])
        ball = b.sphere((0, 0, -2), 0.5, b.lambertian(b.solid((0.5, 0.5, 0.5))))
        return b.list([ball, medium] if opaque == "before" else [medium, ball])
    world = rl.World.build(scene)
    kinds = world.materials()["kind"]
    return world, {k: int(np.flatnonzero(kinds == v)[0]) for k, v in (("phase", rl.api.MAT_ISOTROPIC), ("lambertian", rl.api.MAT_LAMBERTIAN))
                   if (kinds == v).any()}


def _first_f64(oracle, seed, stream, pos):
    """gen::<f64>() of ChaCha8Rng::seed_from_u64(seed) after set_stream(stream) at word `pos`: from chacha_script where the position is
    even (its draws are whole u64s), from the raw block words where it is odd (rand_core BlockRng::next_u64: words pos, pos + 1)."""
    if pos % 2 == 0:
        return float(oracle.chacha_script(seed, [("set_stream", stream)] + [("u64",)] * (pos // 2) + [("f64",)])[0][-1])
    w = np.concatenate([oracle.chacha_block(seed, c, stream) for c in range((pos + 1) // 16 + 1)])
    return float(((int(w[pos]) | (int(w[pos + 1]) << 32)) >> 11) * 2.0 ** -53)


def _free_path(u):
    """constant_medium.rs:55: neg_inv_density * ln(u)."""
    return (-1.0 / DENSITY) * math.log(u)


def _check_medium_hits(rl, hits, out_cur, cur, rays, t1, chord, ray_length, us, phase, label):
    """hit iff free path <= chord (none within 1e-12 of equality); t = t1 + free path / ray_length and p = r.at(t) at 1e-14 (the device
    log is <= 2 ulp from glibc's, DESIGN.md §10: ln(u) in [-37, 0) moves t by <= 2 ulp of the free path, a tenfold margin and more);
    the reference's arbitrary fields; two words per evaluated medium."""
    n_hit = 0
    for i, u in enumerate(us):
        hd = _free_path(u)
        assert abs(hd - chord) > 1e-12 * chord, (label, i, "the draw sits on the decision: pick another stream")
        want = hd <= chord
        assert bool(hits["hit"][i]) == want, (label, i, hd, chord)
        assert out_cur["stream"][i] == cur["stream"][i] and out_cur["word_pos"][i] == cur["word_pos"][i] + np.uint64(2), (label, i)
        if not want:
            assert math.isinf(hits["t"][i]) and not hits[i:i + 1].view(np.uint8)[8:].any(), (label, i)
            continue
        n_hit += 1
        t = t1 + hd / ray_length
        assert abs(hits["t"][i] - t) <= 1e-14 * abs(t), (label, i, hits["t"][i], t)
        p = rays["origin"][i] + rays["dir"][i] * t
        assert np.all(np.abs(hits["p"][i] - p) <= 1e-14 * np.abs(p) + 1e-300), (label, i, hits["p"][i], p)
        assert np.array_equal(hits["normal"][i], (1.0, 0.0, 0.0)) and hits["u"][i] == 0.0 and hits["v"][i] == 0.0, (label, i)
        assert hits["front_face"][i] == 1 and hits["material"][i] == phase and hits["_pad"][i] == 0, (label, i)
    return n_hit


def test_known_answers_by_hand(rl, oracle):
    """3: axial rays from the origin through the unit-sphere slab at (0, 0, -5): dir (0, 0, -1) enters at t = 4 and leaves at 6, the
    unnormalised (0, 0, -2.5) at 1.6 and 2.4 (ray_length 2.5: the same 2-unit chord); streams 0..31 at word 0 and at word 3."""
    api = rl.api
    world, idx = _slab(rl)
    streams = np.arange(32, dtype=np.uint64)
    assert _first_f64(oracle, SEED, 5, 0) == float(((int(oracle.chacha_block(SEED, 0, 5)[0]) | (int(oracle.chacha_block(SEED, 0, 5)[1]) << 32)) >> 11) * 2.0 ** -53)
    outcomes = {True: 0, False: 0}
    for d, t1, length in (((0.0, 0.0, -1.0), 4.0, 1.0), ((0.0, 0.0, -2.5), 1.6, 2.5)):
        for pos in (0, 3):
            cur = api.pack_cursors(streams, pos)
            rays = api.pack_rays(np.zeros((32, 3)), np.tile(d, (32, 1)))
            st = {}
            hits, out_cur = world.hit_rays_seeded(rays, cur, SEED, stats=st)
            us = [_first_f64(oracle, SEED, int(s), pos) for s in streams]
            chord = (6.0 - 4.0) if length == 1.0 else (2.4 - 1.6) * 2.5
            k = _check_medium_hits(rl, hits, out_cur, cur, rays, t1, chord, length, us, idx["phase"], (d, pos))
            print("dir", d, "word", pos, "hits", k, "of 32")
            outcomes[True] += k
            outcomes[False] += 32 - k
            assert st["rays"] == 32 and st["rng_words"] == 64 and st["sphere_tests"] == 64  # boundary.hit twice per ray
            free, free_cur = world.hit_rays_seeded(rays, cur, SEED)
            assert free.tobytes() == hits.tobytes() and free_cur.tobytes() == out_cur.tobytes()
    assert outcomes[True] >= 8 and outcomes[False] >= 8, outcomes


def test_known_answers_across_a_block_boundary(rl, oracle):
    """3, beside the issue's positions: cursors at words 15 and 31, where the draw's two words lie in two ChaCha8 blocks (the ring's first
    block is the cursor's, its refill the next one), and at word 13 with two media in a row, so that the second draw is the straddling one."""
    api = rl.api
    world, idx = _slab(rl)
    streams = np.arange(32, dtype=np.uint64)
    rays = api.pack_rays(np.zeros((32, 3)), np.tile((0.0, 0.0, -1.0), (32, 1)))
    for pos in (15, 31):
        cur = api.pack_cursors(streams, pos)
        hits, out_cur = world.hit_rays_seeded(rays, cur, SEED)
        us = [_first_f64(oracle, SEED, int(s), pos) for s in streams]
        k = _check_medium_hits(rl, hits, out_cur, cur, rays, 4.0, 2.0, 1.0, us, idx["phase"], ("straddle", pos))
        assert 0 < k < 32, pos

    def two(b):  # the second slab lies behind the first: a ray that leaves the first unscattered draws again, from words 15 | 16
        fog = b.isotropic(b.solid((1.0, 1.0, 1.0)))
        return b.list([b.constant_medium(b.sphere((0, 0, -5), 1.0, b.flat()), DENSITY, fog), b.constant_medium(b.sphere((0, 0, -9), 1.0, b.flat()), DENSITY, fog)])
    world2 = rl.World.build(two)
    cur = api.pack_cursors(streams, 13)
    hits, out_cur = world2.hit_rays_seeded(rays, cur, SEED)
    n_second = 0
    for i, s in enumerate(streams):
        hd1, hd2 = _free_path(_first_f64(oracle, SEED, int(s), 13)), _free_path(_first_f64(oracle, SEED, int(s), 15))
        assert abs(hd1 - 2.0) > 2e-12 and abs(hd2 - 2.0) > 2e-12
        if hd1 <= 2.0:  # scattered in the first slab: the second one's chord [8, min(10, t)] is empty, no second draw
            want_t, words = 4.0 + hd1, 2
        else:
            want_t, words = (8.0 + hd2 if hd2 <= 2.0 else INF), 4
            n_second += hd2 <= 2.0
        assert out_cur["word_pos"][i] == 13 + words, (i, out_cur[i], words)
        assert (math.isinf(want_t) and hits["hit"][i] == 0) or abs(hits["t"][i] - want_t) <= 1e-14 * want_t, (i, hits["t"][i], want_t)
    assert n_second > 0


def test_scatter_and_ray_color_draws_across_a_block_boundary(rl, oracle):
    """The other two consumers of a cursor at word 15, where a draw takes its low half from the last word of one ChaCha8 block and its
    high half from the first word of the next: scatter_rays' Isotropic direction by hand on the oracle's block words (rand 0.8.5
    Uniform(-1, 1) and rand_distr UnitSphere), and ray_color_rays on perlin_spheres against the loop of hit_rays_seeded + scatter_rays.
    The Noise colour depends on the hit point continuously, so a draw with a wrong low word shows in it (a solid colour hides it)."""
    import struct
    api = rl.api
    world, idx = _slab(rl)
    n = 32
    streams = np.arange(n, dtype=np.uint64)

    def uniform(w, pos):  # ((u64 >> 12) | exponent of 1.0 as f64, in [1, 2)) - 1) * 2 - 1
        v = struct.unpack("<d", struct.pack("<Q", ((int(w[pos]) | (int(w[pos + 1]) << 32)) >> 12) | 0x3FF0000000000000))[0]
        return (v - 1.0) * 2.0 + (-1.0)
    hits = np.zeros(n, dtype=api.RTIOW_HIT)
    hits["t"], hits["hit"], hits["front_face"], hits["material"], hits["normal"], hits["p"] = 1.0, 1, 1, idx["phase"], (1.0, 0.0, 0.0), (0.0, 0.0, -5.0)
    rays = api.pack_rays(np.zeros((n, 3)), np.tile((0.0, 0.0, -1.0), (n, 1)))
    cur = api.pack_cursors(streams, 15)
    rec, out_cur = world.scatter_rays(rays, hits, cur, SEED)
    for i, s in enumerate(streams):
        w = np.concatenate([oracle.chacha_block(SEED, c, int(s)) for c in range(4)])
        pos = 15
        while True:
            x1, x2 = uniform(w, pos), uniform(w, pos + 2)
            pos += 4
            q = x1 * x1 + x2 * x2
            if q < 1.0:
                break
        f = 2.0 * math.sqrt(1.0 - q)
        assert out_cur["word_pos"][i] == pos and np.array_equal(rec["scattered"]["dir"][i], (x1 * f, x2 * f, 1.0 - 2.0 * q)), (i, rec["scattered"]["dir"][i])

    # perlin_spheres: Lambertian only, so every bounce takes a multiple of 4 words and a path that starts at word 15 (camera cursors at
    # word 9 + get_rays' 6) shades at word 15 of a block again and again
    pw = rl.World.perlin_spheres()
    p = pw.params
    p.image_width, p.samples_per_pixel = 48, 1
    p.max_depth = min(p.max_depth, 20)
    _, r, c = _frame(rl, rl.Camera(p), 9)
    assert (c["word_pos"] == 15).all()
    want = pw.ray_color_rays(None, None, None, c, p.seed, p.max_depth, p.background, rays=r, stats={}, allow_degenerate=True)
    free = pw.ray_color_rays(None, None, None, c, p.seed, p.max_depth, p.background, rays=r, allow_degenerate=True)
    got = _compose(pw, p, r, c, counting=False)
    for g, w, f in zip(got[:3], want, free):
        assert g.tobytes() == w.tobytes() and g.tobytes() == f.tobytes()
    assert got[3] == 0


def test_known_answers_interval_cases(rl, oracle):
    """3, the interval: tmax = 5 cuts the chord to 1; tmin = 4.5 moves t1; an origin at the sphere's centre has rec1.t = -1, clamped to
    tmin and then to 0 (rec1.t.max(0.0)); an interval that ends before the boundary reaches no draw."""
    api = rl.api
    world, idx = _slab(rl)
    streams = np.arange(32, dtype=np.uint64)
    cur = api.pack_cursors(streams, 0)
    us = [_first_f64(oracle, SEED, int(s), 0) for s in streams]
    front = api.pack_rays(np.zeros((32, 3)), np.tile((0.0, 0.0, -1.0), (32, 1)))
    centre = api.pack_rays(np.tile((0.0, 0.0, -5.0), (32, 1)), np.tile((0.0, 0.0, -1.0), (32, 1)))
    for label, rays, tmin, tmax, t1, chord in (("tmax 5", front, 1e-10, 5.0, 4.0, 1.0), ("tmin 4.5", front, 4.5, INF, 4.5, 1.5),
                                               ("centre", centre, 1e-10, INF, 1e-10, 1.0 - 1e-10), ("centre, tmin -10", centre, -10.0, INF, 0.0, 1.0)):
        hits, out_cur = world.hit_rays_seeded(rays, cur, SEED, tmin=tmin, tmax=tmax)
        k = _check_medium_hits(rl, hits, out_cur, cur, rays, t1, chord, 1.0, us, idx["phase"], label)
        print(label, "hits", k, "of 32")
        assert 0 < k < 32, label
    st = {}
    hits, out_cur = world.hit_rays_seeded(front, cur, SEED, tmax=3.5, stats=st)  # t2 = min(6, 3.5) <= t1 = 4: not evaluated
    assert not hits["hit"].any() and out_cur.tobytes() == cur.tobytes() and st["rng_words"] == 0


def test_known_answers_fold_order_and_misses(rl, oracle):
    """3, the fold's order: an opaque sphere at z = -2 (hit at t = 1.5) listed BEFORE the medium cuts the medium's chord to nothing — no
    draw, 0 words; listed AFTER it the medium is evaluated first and draws, 2 words; the opaque hit is returned in both orders.  A ray that
    misses the boundary leaves its cursor unchanged."""
    api = rl.api
    streams = np.arange(32, dtype=np.uint64)
    cur = api.pack_cursors(streams, 3)
    rays = api.pack_rays(np.zeros((32, 3)), np.tile((0.0, 0.0, -1.0), (32, 1)))
    records = {}
    for order, words in (("before", 0), ("after", 2)):
        world, idx = _slab(rl, order)
        st = {}
        hits, out_cur = world.hit_rays_seeded(rays, cur, SEED, stats=st)
        assert hits["hit"].all() and (hits["t"] == 1.5).all() and (hits["material"] == idx["lambertian"]).all(), order
        assert np.array_equal(hits["normal"], np.tile((0.0, 0.0, 1.0), (32, 1))) and (hits["front_face"] == 1).all(), order
        assert np.array_equal(out_cur["word_pos"], cur["word_pos"] + np.uint64(words)) and st["rng_words"] == 32 * words, (order, st)
        records[order] = hits
    assert records["before"]["t"].tobytes() == records["after"]["t"].tobytes() and records["before"]["p"].tobytes() == records["after"]["p"].tobytes()
    world, _ = _slab(rl)
    away = api.pack_rays(np.zeros((32, 3)), np.tile((0.0, 1.0, 0.0), (32, 1)))
    st = {}
    hits, out_cur = world.hit_rays_seeded(away, cur, SEED, stats=st)
    assert not hits["hit"].any() and out_cur.tobytes() == cur.tobytes() and st["rng_words"] == 0 and st["rays"] == 32


# ---------------------------------------------------------------------------------------------- 4: media-free scenes
def test_media_free_scene_gives_hit_rays_records_and_unchanged_cursors(rl):
    """4: bouncing_spheres at 64 wide: records byte-equal to hit_rays, cursors unchanged, rng_words == 0, and the fast walk serves the
    counter-free call."""
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel = 64, 1
    cam = rl.Camera(p)
    _, rays, cur = _frame(rl, cam, 7)
    want = world.hit_rays(rays["origin"], rays["dir"], rays["time"])
    assert api.last_query()["kernel"] == "fast"
    st = {}
    world.hit_rays(rays["origin"], rays["dir"], rays["time"], stats=st)
    assert api.last_query()["kernel"] == "reference"
    hits, out_cur = world.hit_rays_seeded(rays, cur, p.seed)
    assert api.last_query()["kernel"] == "fast"
    assert hits.tobytes() == want.tobytes() and out_cur.tobytes() == cur.tobytes()
    ss = {}
    hits, out_cur = world.hit_rays_seeded(rays, cur, p.seed, stats=ss)
    assert api.last_query()["kernel"] == "reference"
    assert hits.tobytes() == want.tobytes() and out_cur.tobytes() == cur.tobytes()
    assert ss["rng_words"] == 0 and ss["rays"] == rays.shape[0] and all(ss[k] == st[k] for k in COUNTERS)
    # an output buffer of its own receives a copy of the input
    lib = api.render_lib()
    out = np.zeros(rays.shape[0], dtype=api.RTIOW_HIT)
    other = np.full(rays.shape[0], 0x55, dtype=np.uint8).repeat(16).view(api.RNG_CURSOR)
    assert lib.rl_rtiow_hit_rays_seeded(world.device(), rays.ctypes.data, cur.ctypes.data, rays.shape[0], p.seed, 1e-10, INF, out.ctypes.data,
                                        other.ctypes.data, None) == api.RL_OK
    assert out.tobytes() == want.tobytes() and other.tobytes() == cur.tobytes()


# ---------------------------------------------------------------------------------------------- 5: placement
def test_results_do_not_depend_on_placement(rl):
    """5: on the miniature room the per-element bytes are the same for batch sizes 1, 63, 65 and 1000, in shuffled order, for a batch
    split in two, and for a batch larger than a launch has lanes (a lane then serves several rays on different streams: a stale ring or a
    stale position would show)."""
    world = rl.World.build(_smoke_room)
    p = _room_params(rl, 1)
    _, rays, cur = _frame(rl, rl.Camera(p), 7)
    pick = np.linspace(0, rays.shape[0] - 1, 1000).astype(np.int64)
    r, c = rays[pick], cur[pick]
    full, full_cur = world.hit_rays_seeded(r, c, p.seed)
    moved = full_cur["word_pos"] != c["word_pos"]
    assert 0 < int(moved.sum()) < 1000  # both kinds of ray are in the batch
    for k in (1, 63, 65, 1000):
        h, cc = world.hit_rays_seeded(r[:k], c[:k], p.seed)
        assert h.tobytes() == full[:k].tobytes() and cc.tobytes() == full_cur[:k].tobytes(), k
    perm = np.random.default_rng(29).permutation(1000)
    h, cc = world.hit_rays_seeded(r[perm], c[perm], p.seed)
    assert h.tobytes() == full[perm].tobytes() and cc.tobytes() == full_cur[perm].tobytes()
    h1, c1 = world.hit_rays_seeded(r[:400], c[:400], p.seed)
    h2, c2 = world.hit_rays_seeded(r[400:], c[400:], p.seed)
    assert h1.tobytes() + h2.tobytes() == full.tobytes() and c1.tobytes() + c2.tobytes() == full_cur.tobytes()
    # 256 CUs x 2048 lanes is the most any launch can have resident; 1000 does not divide it, so lane-mates are different base elements
    idx = np.arange(256 * 2048 + 1000) % 1000
    st = {}
    h, cc = world.hit_rays_seeded(r[idx], c[idx], p.seed, stats=st)
    assert h.tobytes() == full[idx].tobytes() and cc.tobytes() == full_cur[idx].tobytes() and st["rays"] == idx.shape[0]


# ---------------------------------------------------------------------------------------------- 6: edges
def test_edges(rl):
    """6: n = 0 touches no buffer; NULL buffers, NaN bounds, word_pos = 2^31 and an RTC scene are RL_E_INVALID; opt_out_cursors may alias
    the input; hit_rays on a media scene is still RL_E_UNSUPPORTED."""
    api = rl.api
    lib = api.render_lib()
    world, _ = _slab(rl)
    n = 8
    rays = api.pack_rays(np.zeros((n, 3)), np.tile((0.0, 0.0, -1.0), (n, 1)))
    cur = api.pack_cursors(np.arange(n, dtype=np.uint64), 3)
    out = np.zeros(n, dtype=api.RTIOW_HIT)

    def call(sc=None, r=rays, c=cur, k=n, tmin=1e-10, tmax=INF, o=out, oc=None, st=None):
        ptr = lambda a: a.ctypes.data if a is not None else None  # noqa: E731
        return lib.rl_rtiow_hit_rays_seeded(sc or world.device(), ptr(r), ptr(c), k, SEED, tmin, tmax, ptr(o), ptr(oc), st)

    st = api.Stats()
    st.rays = 77
    assert call(r=None, c=None, k=0, o=None, st=C.byref(st)) == api.RL_OK and st.rays == 0
    h0, c0 = world.hit_rays_seeded(rays[:0], cur[:0], SEED)
    assert h0.shape == (0,) and c0.shape == (0,)
    for kw in ({"r": None}, {"c": None}, {"o": None}):
        assert call(**kw) == api.RL_E_INVALID, kw
    for kw in ({"tmin": float("nan")}, {"tmax": float("nan")}):
        assert call(**kw) == api.RL_E_INVALID, kw
    rw = rl.RtcWorld.test_mirror_scene(30, 20)
    assert call(sc=rw.device()) == api.RL_E_INVALID
    for bad in (2 ** 31, 2 ** 40):
        with pytest.raises(rl.RLError) as e:
            world.hit_rays_seeded(rays, api.pack_cursors(np.arange(n, dtype=np.uint64), [0] * (n - 1) + [bad]), SEED)
        assert e.value.code == api.RL_E_INVALID
    ok, ok_cur = world.hit_rays_seeded(rays, api.pack_cursors(np.arange(n, dtype=np.uint64), 2 ** 31 - 9), SEED)
    assert (ok_cur["word_pos"] == np.uint64(2 ** 31 - 7)).all()
    # the NULL-buffer rules hold for the device form too
    assert lib.rl_rtiow_hit_rays_seeded_device(world.device(), None, cur.ctypes.data, n, SEED, 1e-10, INF, out.ctypes.data, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_hit_rays_seeded_device(world.device(), None, None, 0, SEED, 1e-10, INF, None, None, None, None) == api.RL_OK
    # aliasing: the output cursors written over the input, and into a buffer of their own
    want, want_cur = world.hit_rays_seeded(rays, cur, SEED)
    alias = cur.copy()
    assert call(c=alias, oc=alias) == api.RL_OK
    assert out.tobytes() == want.tobytes() and alias.tobytes() == want_cur.tobytes()
    keep, other = cur.copy(), np.zeros(n, dtype=api.RNG_CURSOR)
    assert call(c=keep, oc=other) == api.RL_OK and keep.tobytes() == cur.tobytes() and other.tobytes() == want_cur.tobytes()
    assert call(c=keep, oc=None) == api.RL_OK and keep.tobytes() == cur.tobytes()
    # the bare-ray call keeps refusing media scenes
    with pytest.raises(rl.RLError) as e:
        world.hit_rays(rays["origin"], rays["dir"])
    assert e.value.code == api.RL_E_UNSUPPORTED


# ---------------------------------------------------------------------------------------------- 7: device form
def test_device_form_status_and_a_query_between_two_renders(rl):
    """7: hit_rays_seeded_device on a side stream gives the host form's bytes; rl_render_status counts the query once, with its rays; a
    query between two asynchronous renders of the same scene changes neither frame."""
    import torch
    api = rl.api
    world, p = _world(rl, "smoke_room")
    _, rays, cur = _frame(rl, rl.Camera(p), 7)
    n = rays.shape[0]
    want, want_cur = world.hit_rays_seeded(rays, cur, p.seed)
    dev = "cuda:0"
    up = lambda a, w: torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], w).copy()).to(dev)  # noqa: E731
    d_r, d_c = up(rays, 56), up(cur, 16)
    d_o = torch.zeros((n, 88), dtype=torch.uint8, device=dev)
    d_oc = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    world.hit_rays_seeded_device(d_r.data_ptr(), d_c.data_ptr(), n, p.seed, d_o.data_ptr(), d_oc.data_ptr(), stream=s2.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == n and st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert api.render_status(world)["rays"] == 0  # counted once
    assert d_o.cpu().numpy().tobytes() == want.tobytes() and d_oc.cpu().numpy().tobytes() == want_cur.tobytes()
    assert d_c.cpu().numpy().tobytes() == cur.tobytes()  # the input cursors are read only
    # synchronous with stats, the cursors written in place
    d_c2 = d_c.clone()
    d_o.zero_()
    torch.cuda.synchronize()
    ss = {}
    world.hit_rays_seeded_device(d_r.data_ptr(), d_c2.data_ptr(), n, p.seed, d_o.data_ptr(), d_c2.data_ptr(), stream=s2.cuda_stream, stats=ss)
    assert ss["rays"] == n and ss["rng_words"] == int((want_cur["word_pos"] - cur["word_pos"]).sum(dtype=np.uint64))
    assert d_o.cpu().numpy().tobytes() == want.tobytes() and d_c2.cpu().numpy().tobytes() == want_cur.tobytes()
    # between two asynchronous renders
    pr = _room_params(rl, 8)
    pr.image_width, pr.samples_per_pixel = 64, 2
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
    world.hit_rays_seeded_device(d_r.data_ptr(), d_c.data_ptr(), n, p.seed, d_o.data_ptr(), d_oc.data_ptr(), stream=s2.cuda_stream)
    cam.render_device(world, b.data_ptr(), stream=s1.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == gs["rays"] and st["flagged"] == 0  # rays: of the most recently enqueued one, the second render
    assert np.array_equal(a.cpu().numpy(), frame) and np.array_equal(b.cpu().numpy(), frame)
    assert d_o.cpu().numpy().tobytes() == want.tobytes() and d_oc.cpu().numpy().tobytes() == want_cur.tobytes()
    assert api.render_status(world)["rays"] == 0


@pytest.mark.skipif(bool(os.environ.get("RL_RENDER_LIB")), reason="the C++ host mirror links librl_render.so (the product library)")
def test_cpp_mirror_probe_agrees_with_the_python_path(rl):
    api = rl.api
    Hh = api.host_lib()
    Hh.rlh_seeded_hit_query_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_void_p]
    world, p = _world(rl, "cornell_smoke")
    assert p.seed == rl.World.example_scene("cornell_smoke").params.seed
    _, rays, cur = _frame(rl, rl.Camera(p), 7)
    rays, cur = np.ascontiguousarray(rays[::4]), cur[::4].copy()
    n = rays.shape[0]
    want, want_cur = world.hit_rays_seeded(rays, cur, p.seed, tmax=900.0)
    assert (want_cur["word_pos"] != cur["word_pos"]).any()
    out = np.zeros(n, dtype=api.RTIOW_HIT)
    assert Hh.rlh_seeded_hit_query_probe(rays.ctypes.data, cur.ctypes.data, n, 1e-10, 900.0, out.ctypes.data) == 0, Hh.rlh_last_error()
    assert out.tobytes() == want.tobytes() and cur.tobytes() == want_cur.tobytes()
