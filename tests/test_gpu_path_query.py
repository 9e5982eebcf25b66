"""GPU tier: the seeded path queries (Camera.get_rays = Camera::get_ray, World.ray_color_rays = Camera::ray_color for ray buffers with
per-ray RNG cursors; include/rl_render.h).

The yardstick is the library's own renders, whose kernels this feature does not touch: a host that rebuilds the reference's _render loop
from the two queries must get the render's frame back bit for bit — cursors (s*W*H + x*W + y, 0) for every sample give
render_independent, carrying each pixel's word position from sample to sample gives render — and, through them, the oracle."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
SCENES = ["golden_test_scene", "bouncing_spheres", "cornell_smoke", "cow_scene", "flat_world"]


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_query_pass_cap(0)
    rl.api.set_fast_traversal(True)


def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


def _scene(rl, golden, name, width=None):
    """(world, camera params) at a reduced frame."""
    if name == "golden_test_scene":
        w = rl.World.golden_test_scene()
    elif name == "bouncing_spheres":
        w = rl.World.bouncing_spheres(1)
    elif name == "cow_scene":
        w = rl.World.cow_scene(golden("spot_triangulated.obj.gz"), _spot_texture())
    else:
        w = rl.World.example_scene(name)
    p = w.params
    p.image_width = width or (48 if name == "cornell_smoke" else 64)
    p.max_depth = min(p.max_depth, 20)
    return w, p


def _cam(rl, p, spp):
    return rl.Camera(dataclasses.replace(p, samples_per_pixel=spp))


def _pixels(cam):
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), W)
    return x, y


def _compose(rl, world, cam, px, py, F, S, chained, counting=False):
    """The reference's _render loop (camera.rs:145-199) from the two queries, for the pixels (px, py) and samples F .. F+S-1: colour sums
    added left to right from 0.0, the summed per-path ray counts, the final cursors, and (counting) the summed counters with rng_words =
    the paths' words + the words get_rays consumed."""
    api = rl.api
    W, H = cam.c.image_width, cam.c.image_height
    p = cam.params
    acc = np.zeros((px.shape[0], 3))
    rays_total = 0
    pos = np.zeros(px.shape[0], dtype=np.uint64)
    tot = dict.fromkeys(COUNTERS, 0)
    cur = None
    for s in range(F, F + S):
        if not chained:
            pos = np.zeros(px.shape[0], dtype=np.uint64)
        cur = api.pack_cursors(np.uint64(s) * np.uint64(W * H) + px * np.uint64(W) + py, pos)
        rays, cur1 = cam.get_rays(px, py, cur)
        st = {} if counting else None
        rgb, cur, counts = world.ray_color_rays(None, None, None, cur1, p.seed, p.max_depth, p.background, rays=rays, stats=st, allow_degenerate=True)
        assert np.array_equal(cur["stream"], cur1["stream"])
        acc = acc + rgb
        rays_total += int(counts.sum(dtype=np.uint64))
        if counting:
            assert st["rays"] == int(counts.sum(dtype=np.uint64))
            for k in COUNTERS:
                tot[k] += st[k]
            tot["rng_words"] += int((cur1["word_pos"] - pos).sum(dtype=np.uint64))
        pos = cur["word_pos"].copy()
    return acc, rays_total, cur, tot


@pytest.mark.parametrize("name", SCENES)
def test_sample_parallel_and_chained_frames_from_queries_bit_for_bit(rl, golden, name):
    """1 + 2: the composition equals render_independent (first_sample F in {0, 3}) and render (S chained samples) as bytes; the summed
    ray counts equal the renders' stats.rays and the summed final word positions the counting render's rng_words.  (Every emitting
    material of the reference ends its path — material.rs DiffuseLight::scatter returns None — so the render's in-place accumulation and
    the per-sample fold add the same terms in the same order for every scene here.)"""
    world, p = _scene(rl, golden, name)
    S = 3
    cam = _cam(rl, p, S)
    W, H = cam.c.image_width, cam.c.image_height
    px, py = _pixels(cam)
    for F in (0, 3):
        gs = {}
        want = cam.render_independent_rows(world, 0, 1, first_sample=F, stats=gs, allow_degenerate=True)
        got, nrays, _, _ = _compose(rl, world, cam, px, py, F, S, chained=False)
        assert got.reshape(H, W, 3).tobytes() == want.tobytes(), (name, F, np.abs(got.reshape(H, W, 3) - want).max())
        assert nrays == gs["rays"], (name, F, nrays, gs["rays"])
    gs = {}
    want = cam.render(world, stats=gs, allow_degenerate=True).data
    got, nrays, cur, _ = _compose(rl, world, cam, px, py, 0, S, chained=True)
    assert got.reshape(H, W, 3).tobytes() == np.ascontiguousarray(want).tobytes(), (name, np.abs(got.reshape(H, W, 3) - want).max())
    assert nrays == gs["rays"] and int(cur["word_pos"].sum(dtype=np.uint64)) == gs["rng_words"], (name, nrays, gs)


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_smoke"])
def test_chained_composition_against_the_oracle(rl, oracle, golden, name):
    """3: 300 pixels chosen with a fixed seed; the chained composition against oracle.rtiow_render_pixels with the bars of
    tests/test_gpu_parity.py:19-25 (1e-4 per channel on the means, 1e-9 relative on the sums), all seven counters exact."""
    world, p = _scene(rl, golden, name, width=96)
    S = 4
    cam = _cam(rl, p, S)
    W, H = cam.c.image_width, cam.c.image_height
    pick = np.random.default_rng(17).choice(W * H, 300, replace=False).astype(np.uint64)
    py, px = np.divmod(pick, np.uint64(W))
    got, _, _, tot = _compose(rl, world, cam, px, py, 0, S, chained=True, counting=True)
    cs = {}
    cpu = oracle.rtiow_render_pixels(world.desc, cam.c, px, py, stats=cs)
    for k in COUNTERS:
        assert tot[k] == cs[k], (name, k, tot[k], cs[k])
    assert np.abs(got - cpu).max() / S <= 1e-4
    assert np.abs(got - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max()), np.abs(got - cpu).max()


def _big_batch(rl, world, p, seed):
    """>= 1 M rays: the camera rays of a 1280-wide frame (get_rays); 120 k rays started inside the scene, on and between its surfaces
    (frame rays advanced to a random parameter along themselves, random direction; hit records are not available for media scenes);
    and far origins, 1 % of the frame at 10 x and 1 % at 1000 x the scene radius (taken as the camera's distance to its target), aimed
    at the target.  A far origin widens every box of the fast walk and may exhaust its step budget, which re-traces the ray: with a 2 %
    share even all of them re-traced leave the 1-in-20 cap room for the order-sensitive ones."""
    api = rl.api
    cam = _cam(rl, dataclasses.replace(p, image_width=1280), 1)
    W, H = cam.c.image_width, cam.c.image_height
    px, py = _pixels(cam)
    rays, _ = cam.get_rays(px, py, api.pack_cursors(px * np.uint64(W) + py))
    rng = np.random.default_rng(seed)
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    radius = float(np.linalg.norm(target - eye))
    n_in = 120_000
    k = rng.choice(rays.shape[0], n_in, replace=False)
    unit = rays["dir"][k] / np.linalg.norm(rays["dir"][k], axis=1, keepdims=True)
    o_in = rays["origin"][k] + unit * rng.uniform(0.2, 2.0, (n_in, 1)) * radius
    d_in = rng.normal(size=(n_in, 3))
    n_far = rays.shape[0] // 100
    u = rng.normal(size=(2 * n_far, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o_far = target + u * radius * np.repeat([10.0, 1000.0], n_far)[:, None]
    d_far = (target + rng.uniform(-0.3, 0.3, (2 * n_far, 3)) * radius) - o_far
    o = np.concatenate([rays["origin"], o_in, o_far])
    d = np.concatenate([rays["dir"], d_in, d_far])
    t = np.concatenate([rays["time"], rng.uniform(0, 1, n_in + 2 * n_far)])
    cur = api.pack_cursors(rng.integers(0, 2 ** 62, o.shape[0], dtype=np.uint64), rng.integers(0, 4096, o.shape[0], dtype=np.uint64) * 2)
    return o, d, t, cur, 2 * n_far


@pytest.mark.parametrize("name", ["bouncing_spheres", "cow_scene", "cornell_smoke"])
def test_fast_path_equals_reference_order_path(rl, golden, name):
    """4: counter-free call (fast kernel) against the counting call and against the counter-free call with the fast traversal switched
    off: colours, cursors and ray counts byte-equal on >= 1 M rays; the fast kernel served with at most 1 ray in 20 re-traced (the cap of
    tests/test_gpu_ray_query.py)."""
    api = rl.api
    world, p = _scene(rl, golden, name)
    o, d, t, cur, n_far = _big_batch(rl, world, p, 5)
    assert o.shape[0] >= 1_000_000
    fast = world.ray_color_rays(o, d, t, cur, p.seed, p.max_depth, p.background, allow_degenerate=True)
    q = api.last_query()
    print(name, "rays", o.shape[0], "far", n_far, "re-traced", q["retraced"], "traced", int(fast[2].sum(dtype=np.uint64)))
    assert q["kernel"] == "fast", q
    assert q["retraced"] * 20 <= int(fast[2].sum(dtype=np.uint64)), q
    st = {}
    ref = world.ray_color_rays(o, d, t, cur, p.seed, p.max_depth, p.background, stats=st, allow_degenerate=True)
    assert api.last_query()["kernel"] == "reference"
    assert st["rays"] == int(ref[2].sum(dtype=np.uint64))
    assert st["rng_words"] == int((ref[1]["word_pos"] - cur["word_pos"]).sum(dtype=np.uint64))
    for a, b in zip(fast, ref):
        assert a.tobytes() == b.tobytes(), name
    api.set_fast_traversal(False)
    try:
        off = world.ray_color_rays(o, d, t, cur, p.seed, p.max_depth, p.background, allow_degenerate=True)
        assert api.last_query()["kernel"] == "reference"
    finally:
        api.set_fast_traversal(True)
    for a, b in zip(fast, off):
        assert a.tobytes() == b.tobytes(), name


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_smoke"])
def test_results_do_not_depend_on_placement(rl, golden, name):
    """5: a seeded permutation of the batch permutes the outputs; two calls give the bytes of one; several passes (debug cap) too."""
    api = rl.api
    world, p = _scene(rl, golden, name, width=160)
    cam = _cam(rl, p, 1)
    px, py = _pixels(cam)
    W = cam.c.image_width
    rays, cur = cam.get_rays(px, py, api.pack_cursors(np.uint64(7) * np.uint64(W * cam.c.image_height) + px * np.uint64(W) + py))
    args = (p.seed, p.max_depth, p.background)
    want = world.ray_color_rays(None, None, None, cur, *args, rays=rays)
    perm = np.random.default_rng(23).permutation(rays.shape[0])
    got = world.ray_color_rays(None, None, None, cur[perm], *args, rays=rays[perm])
    for a, b in zip(got, want):
        assert a.tobytes() == b[perm].tobytes()
    h = rays.shape[0] // 3
    a1 = world.ray_color_rays(None, None, None, cur[:h], *args, rays=rays[:h])
    a2 = world.ray_color_rays(None, None, None, cur[h:], *args, rays=rays[h:])
    for x1, x2, b in zip(a1, a2, want):
        assert np.concatenate([x1, x2]).tobytes() == b.tobytes()
    for counting in (False, True):
        api.set_query_pass_cap(1000)
        try:
            st = {} if counting else None
            got = world.ray_color_rays(None, None, None, cur, *args, rays=rays, stats=st)
        finally:
            api.set_query_pass_cap(0)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
        if counting:
            assert st["rays"] == int(want[2].sum(dtype=np.uint64))


def test_custom_rays_are_used_as_given(rl, golden):
    """6: the pinhole rays of a second camera position handed over as the caller's own origin / direction / time arrays, with the
    cursors that camera's get_rays returned, give the bytes of ray_color_rays on get_rays' records; an orthographic grid over
    bouncing_spheres: no flag, every ray that hits nothing returns the background exactly, every colour finite."""
    api = rl.api
    world, p = _scene(rl, golden, "bouncing_spheres", width=96)
    p2 = dataclasses.replace(p, lookfrom=(-9.0, 4.0, 6.0), defocus_angle=0.0)
    cam = _cam(rl, p2, 1)
    px, py = _pixels(cam)
    W = cam.c.image_width
    rays, cur = cam.get_rays(px, py, api.pack_cursors(px * np.uint64(W) + py))
    assert np.array_equal(rays["origin"], np.tile(np.array(list(cam.c.lookfrom)), (rays.shape[0], 1)))
    # the same rays as plain arrays of the caller's own making (a copy through Python floats and fresh buffers)
    o = np.array(rays["origin"].tolist())
    d = np.array(rays["dir"].tolist())
    t = np.array(rays["time"].tolist())
    args = (p2.seed, p2.max_depth, p2.background)
    want = world.ray_color_rays(None, None, None, cur, *args, rays=rays)
    got = world.ray_color_rays(o, d, t, cur, *args)
    for a, b in zip(got, want):
        assert a.tobytes() == b.tobytes()
    gx, gz = np.meshgrid(np.linspace(-12, 12, 120), np.linspace(-12, 12, 120))
    n = gx.size
    oo = np.stack([gx.reshape(-1), np.full(n, 30.0), gz.reshape(-1)], axis=1)
    dd = np.tile((0.0, -1.0, 0.0), (n, 1))
    up = np.tile((0.0, 1.0, 0.0), (n, 1))
    bg = (0.25, 0.5, 0.75)
    st = {}
    rgb, _, counts = world.ray_color_rays(np.concatenate([oo, oo]), np.concatenate([dd, up]), None, api.pack_cursors(np.arange(2 * n, dtype=np.uint64)),
                                          3, 10, bg, stats=st)
    assert st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert np.isfinite(rgb).all()
    assert (counts[n:] == 1).all() and np.array_equal(rgb[n:], np.tile(bg, (n, 1)))  # straight up: one ray, the background exactly
    assert (counts[:n] >= 1).all() and (counts[:n] <= 10).all()


def test_edges(rl, golden):
    """7: max_depth 0, n = 0, word_pos 2^31, cursors starting mid-block (odd positions and word 15 included) and ending a block, a zero
    direction, a NaN origin."""
    api = rl.api
    lib = api.render_lib()
    world, p = _scene(rl, golden, "golden_test_scene")
    cam = _cam(rl, p, 1)
    px, py = _pixels(cam)
    W = cam.c.image_width
    cur0 = api.pack_cursors(px * np.uint64(W) + py)
    rays, cur = cam.get_rays(px, py, cur0)
    n = rays.shape[0]
    bg = p.background
    # max_depth = 0: black, no ray, cursor unchanged
    st = {}
    rgb, c2, counts = world.ray_color_rays(None, None, None, cur, p.seed, 0, bg, rays=rays, stats=st)
    assert not rgb.any() and not counts.any() and c2.tobytes() == cur.tobytes() and st["rays"] == 0 and st["rng_words"] == 0
    rgb, c2, counts = world.ray_color_rays(None, None, None, cur, p.seed, 0, bg, rays=rays)
    assert not rgb.any() and not counts.any() and c2.tobytes() == cur.tobytes()
    # n = 0
    rgb, c2, counts = world.ray_color_rays(np.zeros((0, 3)), np.zeros((0, 3)), None, api.pack_cursors(np.zeros(0, dtype=np.uint64)), p.seed, 5, bg)
    assert rgb.shape == (0, 3) and c2.shape == (0,) and counts.shape == (0,)
    assert cam.get_rays([], [], api.pack_cursors(np.zeros(0, dtype=np.uint64)))[0].shape == (0,)
    bgc = (C.c_double * 3)(*bg)
    assert lib.rl_rtiow_ray_color_rays(world.device(), None, None, 0, 0, 5, bgc, None, None, None, None) == api.RL_OK
    # NULL buffers, the other scene family, word_pos = 2^31, a pixel outside the image
    one = np.zeros((1, 3))
    assert lib.rl_rtiow_ray_color_rays(world.device(), None, cur.ctypes.data, 1, 0, 5, bgc, one.ctypes.data, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_ray_color_rays(world.device(), rays.ctypes.data, cur.ctypes.data, 1, 0, 5, bgc, None, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_ray_color_rays(world.device(), rays.ctypes.data, cur.ctypes.data, 1, 0, 5, None, one.ctypes.data, None, None, None) == api.RL_E_INVALID
    rw = rl.RtcWorld.test_mirror_scene(30, 20)
    assert lib.rl_rtiow_ray_color_rays(rw.device(), rays.ctypes.data, cur.ctypes.data, 1, 0, 5, bgc, one.ctypes.data, None, None, None) == api.RL_E_INVALID
    for bad in (api.pack_cursors([1], 2 ** 31), api.pack_cursors([1], 2 ** 40)):
        with pytest.raises(rl.RLError) as e:
            world.ray_color_rays(None, None, None, bad, p.seed, 5, bg, rays=rays[:1])
        assert e.value.code == api.RL_E_INVALID
        with pytest.raises(rl.RLError) as e:
            cam.get_rays([0], [0], bad)
        assert e.value.code == api.RL_E_INVALID
    for x, y in ((W, 0), (0, cam.c.image_height)):
        with pytest.raises(rl.RLError) as e:
            cam.get_rays([x], [y], api.pack_cursors([0]))
        assert e.value.code == api.RL_E_INVALID
    # cursors anywhere in a block: a draw is words pos, pos + 1 of the stream, so the stream read from word w in one go equals the
    # stream read word by word — get_rays at word w consumes 6 words (pinhole camera: three draws), and its three draws are the u64s
    # at words w, w + 2, w + 4.  Checked against the draws of neighbouring starts: the ray drawn at w + 2 shares two of its three draws
    # (shifted) with the ray drawn at w, for even and odd w, across the block boundary (w = 11 .. 15) and at a block's last words.
    pin = _cam(rl, dataclasses.replace(p, defocus_angle=0.0), 1)  # (the golden scene's own camera has a defocus disc: UnitDisc draws in between)
    c = pin.c
    # an odd position reads the stream's words as rand_core's BlockRng::next_u64 does: lo = word pos, hi = word pos + 1.  `time` is the
    # third draw, exact in the ray: v(w) = u64 at words (w + 4, w + 5) >> 11.  The odd draw's halves against the even draws around it
    # (which the renders pin): e = 10 and 26 put the odd draw on words 15 | 16 and 31 | 32, across a block boundary.
    for e in (0, 6, 8, 10, 12, 26, 1018):
        tr, _ = pin.get_rays([3, 3, 3], [2, 2, 2], api.pack_cursors([99, 99, 99], [e, e + 1, e + 2]))
        ve, vo, ve2 = (int(t * 2.0 ** 53) for t in tr["time"])
        assert vo & (2 ** 21 - 1) == (ve >> 21) >> 11, e   # word e + 5 >> 11
        assert (vo >> 21) >> 11 == ve2 & (2 ** 21 - 1), e  # word e + 6 >> 11
    p00, du, dv = (np.array(list(v)) for v in (c.pixel_00, c.pixel_du, c.pixel_dv))
    for w in list(range(0, 36)) + [1023, 1024, 1025, 2 ** 31 - 8]:
        r0, c0 = pin.get_rays([3, 3], [2, 2], api.pack_cursors([99, 99], [w, w + 2]))
        assert c0["word_pos"].tolist() == [w + 6, w + 8] and c0["stream"].tolist() == [99, 99]
        centre = (p00 + du * 3.0) + dv * 2.0
        # invert pixel_sample = centre + (du*sx + dv*sy) for the second draw sy of the first ray = the first draw sx' of the second ray
        A = np.stack([du, dv], axis=1)
        s0 = np.linalg.lstsq(A, (r0["dir"][0] + r0["origin"][0]) - centre, rcond=None)[0]
        s1 = np.linalg.lstsq(A, (r0["dir"][1] + r0["origin"][1]) - centre, rcond=None)[0]
        assert abs(s0[1] - s1[0]) < 1e-9, (w, s0, s1)
        assert -0.5 <= s0[0] < 0.5 and -0.5 <= s0[1] < 0.5 and 0.0 <= r0["time"][0] < 1.0
        # ray_color from a cursor at w: fast and reference-order kernels agree, whatever the parity
        cw = api.pack_cursors(np.full(64, 5, dtype=np.uint64), np.full(64, w, dtype=np.uint64))
        f = world.ray_color_rays(None, None, None, cw, p.seed, p.max_depth, bg, rays=rays[:64])
        st = {}
        r = world.ray_color_rays(None, None, None, cw, p.seed, p.max_depth, bg, rays=rays[:64], stats=st)
        for a, b in zip(f, r):
            assert a.tobytes() == b.tobytes(), w
        used = r[1]["word_pos"] - np.uint64(w)
        assert (used % np.uint64(2) == 0).all() and st["rng_words"] == int(used.sum(dtype=np.uint64))
    # a zero direction and a NaN origin: defined results, no flag unless the reference would panic
    o = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 1.0, 0.0]])
    d = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [np.nan, 0.0, -1.0]])
    cz = api.pack_cursors([1, 2, 3])
    st = {}
    rz = world.ray_color_rays(o, d, None, cz, p.seed, 5, bg, stats=st, allow_degenerate=True)
    fz = world.ray_color_rays(o, d, None, cz, p.seed, 5, bg, allow_degenerate=True)
    for a, b in zip(fz, rz):
        assert a.tobytes() == b.tobytes()
    assert (rz[2] == 1).all() and st["flagged"] == 0  # NaN comparisons are false everywhere: no hit, the background, no panic site
    assert np.array_equal(rz[0], np.tile(bg, (3, 1)))


def test_device_forms_status_and_a_query_between_two_renders(rl, golden):
    """7 (device forms): get_rays_device + ray_color_rays_device on a side stream give the host forms' bytes; rl_render_status reports
    the query's rays; a flagged query reports RL_E_DEGENERATE through rl_render_status with every output written; a query between two
    asynchronous renders leaves their frames and accounting unchanged."""
    import torch
    api = rl.api
    world, p = _scene(rl, golden, "golden_test_scene", width=96)
    p.samples_per_pixel = 4
    cam = rl.Camera(p)
    H, W = cam.c.image_height, cam.c.image_width
    px, py = _pixels(cam)
    cur0 = api.pack_cursors(px * np.uint64(W) + py)
    rays, cur = cam.get_rays(px, py, cur0)
    want = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays)
    n = rays.shape[0]
    dev = "cuda:0"
    d_px = torch.from_numpy(px.astype(np.uint32)).to(dev)
    d_py = torch.from_numpy(py.astype(np.uint32)).to(dev)
    d_cur = torch.from_numpy(cur0.view(np.uint8).reshape(n, 16).copy()).to(dev)
    d_rays = torch.zeros((n, 56), dtype=torch.uint8, device=dev)
    d_rgb = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    cam.get_rays_device(d_px.data_ptr(), d_py.data_ptr(), d_cur.data_ptr(), d_rays.data_ptr(), d_cur.data_ptr(), n, stream=s2.cuda_stream)
    world.ray_color_rays_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, p.max_depth, p.background, d_rgb.data_ptr(), d_cur.data_ptr(),
                                d_cnt.data_ptr(), stream=s2.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == int(want[2].sum()) and st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert d_rays.cpu().numpy().tobytes() == rays.tobytes()
    assert d_rgb.cpu().numpy().tobytes() == want[0].tobytes() and d_cur.cpu().numpy().tobytes() == want[1].tobytes()
    assert d_cnt.cpu().numpy().astype(np.uint32).tobytes() == want[2].tobytes()
    # between two asynchronous renders
    gs = {}
    frame = cam.render(world, stats=gs).data
    a = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    b = torch.zeros((H, W, 3), dtype=torch.float64, device=dev)
    d_cur.copy_(torch.from_numpy(cur.view(np.uint8).reshape(n, 16).copy()))
    d_rgb.zero_()
    torch.cuda.synchronize()
    cam.render_device(world, a.data_ptr(), stream=s1.cuda_stream)
    world.ray_color_rays_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, p.max_depth, p.background, d_rgb.data_ptr(), stream=s2.cuda_stream)
    cam.render_device(world, b.data_ptr(), stream=s1.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == gs["rays"] and st["flagged"] == 0  # rays: of the most recently enqueued one, the second render
    assert np.array_equal(a.cpu().numpy(), frame) and np.array_equal(b.cpu().numpy(), frame)
    assert d_rgb.cpu().numpy().tobytes() == want[0].tobytes()
    assert api.render_status(world)["rays"] == 0
    # a flagged query: a sphere of radius 0 (test_gpu_edge_cases.py) reaches vec3.rs:219 on every hit
    tex = np.zeros(1, dtype=api.TEXTURE)
    tex[0]["kind"], tex[0]["color"] = api.TEX_SOLID, (0.5, 0.4, 0.3)
    mats = np.zeros(1, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 0
    sph = np.zeros(2, dtype=api.SPHERE)
    sph["center0"], sph["radius"], sph["material"] = [(0, 0, -1), (0.6, 0, -1)], [0.5, 0.0], [0, 0]
    bad = rl.World.from_spheres(sph, mats, tex, False)
    o = np.tile((0.6, 0.0, 1.0), (8, 1))
    d = np.tile((0.0, 0.0, -1.0), (8, 1))
    cz = api.pack_cursors(np.arange(8, dtype=np.uint64))
    st = {}
    ref = bad.ray_color_rays(o, d, None, cz, 1, 4, (1, 1, 1), stats=st, allow_degenerate=True)
    assert st["flagged"] > 0 and st["rc"] == api.RL_E_DEGENERATE
    with pytest.raises(rl.RLError) as e:
        bad.ray_color_rays(o, d, None, cz, 1, 4, (1, 1, 1))
    assert e.value.code == api.RL_E_DEGENERATE
    rz = api.pack_rays(o, d)
    d_r = torch.from_numpy(rz.view(np.uint8).reshape(8, 56).copy()).to(dev)
    d_c = torch.from_numpy(cz.view(np.uint8).reshape(8, 16).copy()).to(dev)
    d_o = torch.full((8, 3), -1.0, dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    bad.ray_color_rays_device(d_r.data_ptr(), d_c.data_ptr(), 8, 1, 4, (1, 1, 1), d_o.data_ptr(), stream=s2.cuda_stream)
    stt = api.render_status(bad, allow_degenerate=True)
    assert stt["rc"] == api.RL_E_DEGENERATE and stt["flagged"] == st["flagged"]
    assert d_o.cpu().numpy().tobytes() == ref[0].tobytes()


@pytest.mark.skipif(bool(os.environ.get("RL_RENDER_LIB")), reason="the C++ host mirror links librl_render.so (the product library)")
def test_cpp_mirror_probe_agrees_with_the_python_path(rl):
    api = rl.api
    Hh = api.host_lib()
    Hh.rlh_path_query_probe.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    world = rl.World.golden_test_scene()
    p = world.params
    cam = rl.Camera(p)
    n = 200
    px = np.arange(n, dtype=np.uint64) % np.uint64(p.image_width)
    cur = api.pack_cursors(np.arange(n, dtype=np.uint64) + np.uint64(11))
    rays = np.zeros(n, dtype=api.RAY)
    c1 = cur.copy()
    assert Hh.rlh_path_query_probe(0, None, c1.ctypes.data, n, rays.ctypes.data) == 0, Hh.rlh_last_error()
    want_rays, want_cur = cam.get_rays(px, np.zeros(n, dtype=np.uint64), cur)
    assert rays.tobytes() == want_rays.tobytes() and c1.tobytes() == want_cur.tobytes()
    rgb = np.zeros((n, 3))
    assert Hh.rlh_path_query_probe(1, rays.ctypes.data, c1.ctypes.data, n, rgb.ctypes.data) == 0, Hh.rlh_last_error()
    want = world.ray_color_rays(None, None, None, want_cur, p.seed, p.max_depth, p.background, rays=want_rays)
    assert rgb.tobytes() == want[0].tobytes() and c1.tobytes() == want[1].tobytes()
