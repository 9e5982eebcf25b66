"""GPU tier: the occlusion queries (occluded_rays / occluded_rays_device; include/rl_render.h rl_rtiow_occluded_rays*).

occluded[i] is Hittable::hit(&rays[i], &Interval{tmin, tmax}).is_some() on the scene root, so every byte is checked against the CPU
oracle's rtiow_hit and against the `hit` field of World.hit_rays for the same ray and interval:
  * random rays (camera-like, from inside the scene, axis-parallel, far origins) against the oracle, counting and counter-free;
  * a frame's pixel-centre rays and the shadow segments from their hit points towards one point above the scene against hit_rays, with
    the kernel that served each call (api.last_query()) and a cap on the rays the any-hit walk hands to the reference's fold;
  * the two ends of the closed interval, rays that start on a surface, tails and bounds of the device form, errors, status accounting,
    a degenerate ray, the C++ mirror."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INF = float("inf")
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")


def _rays(cases):
    return np.array([c[0] for c in cases], dtype=np.float64), np.array([c[1] for c in cases], dtype=np.float64)


def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


def _scene(rl, golden, name):
    if name == "golden_test_scene":
        return rl.World.golden_test_scene()
    if name == "bouncing_spheres":
        return rl.World.bouncing_spheres(1)
    if name == "stress60":
        return rl.World.stress_scene(60, 1, golden("spot_triangulated.obj.gz"), _spot_texture())
    return rl.World.example_scene(name)


def _random_rays(rng, eye, target, extent, n_cam, n_inside, n_axis, n_far):
    """Camera-like rays from `eye` towards a disc around `target`, rays starting inside the scene's extent, axis-parallel rays, and a
    handful of rays from ~1e6 scene sizes away aimed at the scene (the mix of tests/test_gpu_ray_query.py)."""
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


def _scene_rays(world, seed, n_cam, n_inside, n_axis, n_far):
    p = world.params
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    rng = np.random.default_rng(seed)
    o, d = _random_rays(rng, eye, target, float(np.linalg.norm(target - eye)), n_cam, n_inside, n_axis, n_far)
    return o, d, rng.uniform(0.0, 1.0, o.shape[0])


def _frame_rays(rl, world, width, aspect):
    """The pixel-centre rays of a width x (width / aspect) frame of the world's own camera (camera.rs:232-262 without the sample offset)."""
    p = world.params
    p.image_width, p.aspect_ratio = width, aspect
    c = rl.Camera(p).c
    W, H = c.image_width, c.image_height
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    p00, du, dv, eye = (np.array(list(v)) for v in (c.pixel_00, c.pixel_du, c.pixel_dv, c.lookfrom))
    centre = (p00 + x.reshape(-1, 1) * du) + y.reshape(-1, 1) * dv
    return np.tile(eye, (W * H, 1)), centre - eye


def _device_rays(rays):
    import torch
    n = rays.shape[0]
    return torch.from_numpy(rays.view(np.uint8).reshape(n, 56).copy()).to("cuda:0")


# ----------------------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("name", ["golden_test_scene", "bouncing_spheres", "cornell_box", "quads", "flat_world", "stress60"])
def test_occluded_rays_equal_the_oracle_ray_by_ray(rl, oracle, golden, name):
    rl.init(0)
    api = rl.api
    world = _scene(rl, golden, name)
    o, d, times = _scene_rays(world, 4100 + len(name), 1200, 500, 300, 16)  # bouncing_spheres: moving centres (sphere.rs:36), random time
    n = o.shape[0]
    for tmin, tmax in ((1e-10, INF), (0.0, 1.0)):  # directions are not normalised: the camera-like rays reach their target at t = 1
        want = np.array([oracle.rtiow_hit(world.desc, o[i], d[i], times[i], tmin, tmax) is not None for i in range(n)])
        if tmax == INF:  # the rays do meet the scene, and do miss it
            assert want.sum() > 100 and (~want).sum() > 100, (name, int(want.sum()))
        # the far-origin rays may reach Sphere::hit's from_normalized check (vec3.rs:219-222, a counted panic site): the answer stands all the same
        free = rl.occluded_rays(world, o, d, times=times, tmin=tmin, tmax=tmax, allow_degenerate=True)
        assert api.last_query()["kernel"] == ("occlusion_fast" if tmin == 1e-10 else "occlusion_reference"), (name, tmin)
        st, hs = {}, {}
        counting = rl.occluded_rays(world, o, d, times=times, tmin=tmin, tmax=tmax, stats=st, allow_degenerate=True)
        assert api.last_query()["kernel"] == "occlusion_reference"
        assert free.dtype == np.bool_ and free.shape == (n,)
        bad = np.nonzero(free != want)[0]
        assert bad.size == 0, (name, tmax, "counter-free", bad[:8], o[bad[:8]], d[bad[:8]])
        bad = np.nonzero(counting != want)[0]
        assert bad.size == 0, (name, tmax, "counting", bad[:8])
        # a counting call's counters are hit_rays' on the same batch, flagged included
        world.hit_rays(o, d, times=times, tmin=tmin, tmax=tmax, stats=hs, allow_degenerate=True)
        assert {k: st[k] for k in COUNTERS} == {k: hs[k] for k in COUNTERS} and st["rays"] == n and st["rc"] == hs["rc"], (name, st, hs)


# ----------------------------------------------------------------------------- 2. against hit_rays, and the routes
@pytest.mark.parametrize("name", ["bouncing_spheres", "stress60", "flat_world"])
def test_frame_rays_and_shadow_segments_equal_hit_rays_on_both_routes(rl, golden, name):
    """(a) the 480 x 270 pixel-centre rays (129,600: more rays than lanes resident at 64 KB of LDS per workgroup, so the grid-stride loop
    takes a second trip); (b) the shadow segments from the hit points of (a) to one fixed point above the scene, dir = L - p, tmax = 1.
    Counter-free calls are served by the any-hit walk, counting ones by the reference-order fold; both give hit_rays' `hit` byte for byte.
    The walk may hand at most 1 ray in 20 of a batch to the fold — the bar test_fast_path_equals_reference_order_bit_for_bit_and_did_run
    holds hit_rays to on these scenes, and hit_rays is held to it on batch (b) here too: with the fold doing all the work the test
    would show nothing."""
    rl.init(0)
    api = rl.api
    world = _scene(rl, golden, name)
    o, d = _frame_rays(rl, world, 480, 16.0 / 9.0)
    assert o.shape[0] == 129_600
    times = np.random.default_rng(6).uniform(0.0, 1.0, o.shape[0])
    p = world.params
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    extent = float(np.linalg.norm(target - eye))
    L = target + extent * np.array([0.3, 1.5, 0.2])  # above the scene, off every axis and plane of symmetry
    first = world.hit_rays(o, d, times=times)
    assert api.last_query()["kernel"] == "fast"
    hit = first["hit"] == 1
    assert hit.sum() > 20_000, (name, int(hit.sum()))
    batches = {"frame": (o, d, times, INF), "shadow": (first["p"][hit], L - first["p"][hit], times[hit], 1.0)}
    for label, (bo, bd, bt, tmax) in batches.items():
        n = bo.shape[0]
        want = world.hit_rays(bo, bd, times=bt, tmax=tmax)
        hq = api.last_query()
        assert hq["kernel"] == "fast"
        free = rl.occluded_rays(world, bo, bd, times=bt, tmax=tmax)
        q = api.last_query()
        print(name, label, "rays", n, "occluded", int(free.sum()), "re-traced: occlusion", q["retraced"], "hit_rays", hq["retraced"])
        assert q["kernel"] == "occlusion_fast", q
        assert hq["retraced"] * 20 <= n, (name, label, hq)  # the yardstick itself stays within the cap on this batch
        assert q["retraced"] * 20 <= n, (name, label, q)
        assert free.astype(np.uint8).tobytes() == want["hit"].astype(np.uint8).tobytes(), (name, label, np.nonzero(free != (want["hit"] == 1))[0][:8])
        st, hs = {}, {}
        counting = rl.occluded_rays(world, bo, bd, times=bt, tmax=tmax, stats=st)
        assert api.last_query() == {"kernel": "occlusion_reference", "retraced": 0}
        assert counting.astype(np.uint8).tobytes() == want["hit"].astype(np.uint8).tobytes(), (name, label)
        ref = world.hit_rays(bo, bd, times=bt, tmax=tmax, stats=hs)
        assert ref.tobytes() == want.tobytes()
        assert {k: st[k] for k in COUNTERS} == {k: hs[k] for k in COUNTERS} and st["rays"] == n, (name, label, st, hs)
        if label == "shadow":  # the segments do both: reach the point and end in the scene
            assert 1000 < free.sum() < n - 1000, (name, int(free.sum()), n)


# ----------------------------------------------------------------------------- 3. the ends of the interval
@pytest.mark.parametrize("name", ["bouncing_spheres", "quads"])
def test_both_ends_of_the_closed_interval(rl, golden, name):
    rl.init(0)
    api = rl.api
    world = _scene(rl, golden, name)
    o, d, times = _scene_rays(world, 91, 1300, 450, 250, 0)
    assert o.shape[0] == 2000
    full = world.hit_rays(o, d, times=times)
    hitting = np.nonzero(full["hit"] == 1)[0]
    picks = hitting[np.linspace(0, hitting.size - 1, 8).astype(int)]
    assert np.unique(picks).size == 8
    for i in picks:
        t = float(full["t"][i])
        for tmax, own in ((t, True), (float(np.nextafter(t, 0.0)), None)):
            want = world.hit_rays(o, d, times=times, tmax=tmax)["hit"] == 1
            free = rl.occluded_rays(world, o, d, times=times, tmax=tmax)
            assert api.last_query()["kernel"] == "occlusion_fast"
            counting = rl.occluded_rays(world, o, d, times=times, tmax=tmax, stats={})
            assert np.array_equal(free, want) and np.array_equal(counting, want), (name, i, tmax, np.nonzero(free != want)[0][:8])
            if own:
                assert free[i], (name, i, t)  # the closed end: the ray's own closest root is inside [1e-10, t]
            else:
                assert not free[i], (name, i, t)  # nothing lies before the closest hit
    zero = rl.occluded_rays(world, o, d, times=times, tmin=0.0)
    assert api.last_query()["kernel"] == "occlusion_reference"  # not the interval the walk's filters are derived for
    assert np.array_equal(zero, world.hit_rays(o, d, times=times, tmin=0.0)["hit"] == 1)


def test_rays_that_start_on_a_sphere_surface(rl, oracle):
    """Origins on the three large spheres of bouncing_spheres (radius 1, centres (0,1,0), (-4,1,0), (4,1,0)), pointing straight out,
    straight in, and anywhere: the root at the origin itself is ~0, on one side or the other of tmin = 1e-10 by rounding alone."""
    rl.init(0)
    world = rl.World.bouncing_spheres(1)
    rng = np.random.default_rng(17)
    u = rng.normal(size=(600, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    centres = np.array([(0.0, 1.0, 0.0), (-4.0, 1.0, 0.0), (4.0, 1.0, 0.0)])[rng.integers(0, 3, 600)]
    o = centres + u
    d = np.concatenate([u[:200], -u[200:400], rng.normal(size=(200, 3))])
    times = rng.uniform(0.0, 1.0, 600)
    for tmax in (INF, 1.0, 2.5):
        want = np.array([oracle.rtiow_hit(world.desc, o[i], d[i], times[i], 1e-10, tmax) is not None for i in range(600)])
        free = rl.occluded_rays(world, o, d, times=times, tmax=tmax)
        counting = rl.occluded_rays(world, o, d, times=times, tmax=tmax, stats={})
        assert np.array_equal(free, want) and np.array_equal(counting, want), (tmax, np.nonzero(free != want)[0][:8])
        assert np.array_equal(free, world.hit_rays(o, d, times=times, tmax=tmax)["hit"] == 1)
    inward = rl.occluded_rays(world, o[200:400], d[200:400], times=times[200:400])
    assert inward.all()  # straight through the sphere the ray starts on: the far side, t = 2


# ----------------------------------------------------------------------------- 4. tails and bounds
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_device_form_writes_n_bytes_and_no_more(rl, n):
    import torch
    rl.init(0)
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    o, d, times = _scene_rays(world, 23, 200, 40, 17, 0)
    want = rl.occluded_rays(world, o, d, times=times)
    assert want.any() and not want.all()
    d_rays = _device_rays(api.pack_rays(o[:n], d[:n], times[:n]))
    for stats in (None, {}):  # the any-hit walk (asynchronous), the reference-order fold (synchronous)
        d_out = torch.full((n + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rl.occluded_rays_device(world, d_rays.data_ptr(), d_out.data_ptr(), n, stream=torch.cuda.current_stream().cuda_stream, stats=stats)
        assert api.last_query()["kernel"] == ("occlusion_fast" if stats is None else "occlusion_reference")
        if stats is None:
            assert api.render_status(world)["rays"] == n
        else:
            assert stats["rays"] == n
        got = d_out.cpu().numpy()
        assert (got[n:] == 0xA5).all(), (n, got[n:n + 8])  # the canary behind element n - 1
        assert np.array_equal(got[:n], want[:n].astype(np.uint8)), n


# ----------------------------------------------------------------------------- 5. errors
def _media_world(rl):
    def build(b):
        fog = b.isotropic(b.solid((1, 1, 1)))
        return b.list([b.constant_medium(b.sphere((0, 0, 0), 1.0, b.lambertian(b.solid((1, 1, 1)))), 0.5, fog)])
    return rl.World.build(build)


def test_errors_and_empty_batches(rl):
    rl.init(0)
    api = rl.api
    lib = api.render_lib()
    o, d = _rays([((0, 0, 5), (0, 0, -1))])
    media = _media_world(rl)
    for call in (lambda: rl.occluded_rays(media, o, d), lambda: rl.occluded_rays(media, o, d, stats={}), lambda: rl.occluded_rays_device(media, 0x1000, 0x2000, 1)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_UNSUPPORTED
        with pytest.raises(rl.RLError) as h:
            media.hit_rays(o, d)
        assert str(e.value) == str(h.value)  # the message of hit_rays
    world = rl.World.golden_test_scene()
    rw = rl.RtcWorld.test_csg_scene(30, 20)
    assert rl.occluded_rays(world, np.zeros((0, 3)), np.zeros((0, 3))).shape == (0,)  # n = 0
    st = {}
    assert rl.occluded_rays(world, np.zeros((0, 3)), np.zeros((0, 3)), stats=st).shape == (0,) and all(st[k] == 0 for k in COUNTERS)
    dirty = api.Stats()
    dirty.rays, dirty.flagged = 99, 99
    assert lib.rl_rtiow_occluded_rays(world.device(), None, 0, 1e-10, INF, None, C.byref(dirty)) == api.RL_OK and dirty.rays == 0 and dirty.flagged == 0
    assert lib.rl_rtiow_occluded_rays(world.device(), None, 0, 1e-10, INF, None, None) == api.RL_OK  # no buffer is touched
    assert lib.rl_rtiow_occluded_rays_device(world.device(), None, 0, 1e-10, INF, None, None, None) == api.RL_OK
    rays = api.pack_rays(o, d)
    out = np.full(1, 7, dtype=np.uint8)
    H, R, P = world.device(), rays.ctypes.data, out.ctypes.data
    NAN = float("nan")
    assert lib.rl_rtiow_occluded_rays(H, None, 1, 1e-10, INF, P, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays(H, R, 1, 1e-10, INF, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays_device(H, None, 1, 1e-10, INF, P, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays_device(H, R, 1, 1e-10, INF, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays(H, R, 1, NAN, INF, P, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays(H, R, 1, 1e-10, NAN, P, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays_device(H, R, 1, 1e-10, NAN, P, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays(H, R, (1 << 40) + 1, 1e-10, INF, P, None) == api.RL_E_INVALID  # refused before anything is read
    assert lib.rl_rtiow_occluded_rays_device(H, R, (1 << 40) + 1, 1e-10, INF, P, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays(rw.device(), R, 1, 1e-10, INF, P, None) == api.RL_E_INVALID  # RTC handle
    assert lib.rl_rtiow_occluded_rays_device(rw.device(), R, 1, 1e-10, INF, P, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_occluded_rays(None, R, 1, 1e-10, INF, P, None) == api.RL_E_INVALID
    assert out[0] == 7  # no refused call wrote anything
    assert lib.rl_rtiow_occluded_rays(H, R, 1, 1e-10, INF, P, None) == api.RL_OK and out[0] in (0, 1)


# ----------------------------------------------------------------------------- 6. device form and status
def test_device_form_on_a_side_stream_then_render_status(rl):
    import torch
    rl.init(0)
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    o, d, times = _scene_rays(world, 3, 3000, 500, 100, 0)
    n = o.shape[0]
    d_rays = _device_rays(api.pack_rays(o, d, times))
    stream = torch.cuda.Stream()
    for tmax in (INF, 1.0):
        want = rl.occluded_rays(world, o, d, times=times, tmax=tmax)
        d_out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        rl.occluded_rays_device(world, d_rays.data_ptr(), d_out.data_ptr(), n, tmax=tmax, stream=stream.cuda_stream)
        st = api.render_status(world)
        assert st["rays"] == n and st["flagged"] == 0 and st["rc"] == api.RL_OK
        assert api.last_query()["kernel"] == "occlusion_fast"
        assert np.array_equal(d_out.cpu().numpy(), want.astype(np.uint8))
        assert api.render_status(world)["rays"] == 0  # each query counts once
    d_out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    cs = {}
    rl.occluded_rays_device(world, d_rays.data_ptr(), d_out.data_ptr(), n, tmax=1.0, stream=stream.cuda_stream, stats=cs)  # synchronous
    assert cs["rays"] == n and cs["node_tests"] > 0 and np.array_equal(d_out.cpu().numpy(), want.astype(np.uint8))


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
    o, d, _ = _scene_rays(world, 4, 2000, 0, 0, 0)
    n = o.shape[0]
    d_rays = _device_rays(api.pack_rays(o, d))
    d_out = torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda:0")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    cam.render_device(world, a.data_ptr(), stream=s1.cuda_stream)
    rl.occluded_rays_device(world, d_rays.data_ptr(), d_out.data_ptr(), n, stream=s2.cuda_stream)
    cam.render_device(world, b.data_ptr(), stream=s1.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == gs["rays"] and st["flagged"] == 0  # rays: of the most recently enqueued one, the second render
    assert np.array_equal(a.cpu().numpy(), want) and np.array_equal(b.cpu().numpy(), want)
    assert np.array_equal(d_out.cpu().numpy(), rl.occluded_rays(world, o, d).astype(np.uint8))
    assert api.render_status(world)["rays"] == 0


def test_a_degenerate_ray_in_a_batch_changes_no_other_ray(rl):
    """The 1e13-radii ray of test_a_degenerate_ray_in_a_batch_flags_that_ray_only (tests/test_gpu_ray_query.py): a unit sphere seen from
    so far away that the outward normal is the zero vector and from_normalized's check fails (vec3.rs:219-222).  The counting form
    reports it as hit_rays does; the byte is hit_rays' either way."""
    rl.init(0)
    api = rl.api
    tex, mats, sph = np.zeros(1, dtype=api.TEXTURE), np.zeros(1, dtype=api.MATERIAL), np.zeros(1, dtype=api.SPHERE)
    sph["center0"], sph["radius"] = (0, 0, 0), 1.0
    w = rl.World.from_spheres(sph, mats, tex, False)
    o, d = _rays([((0, 0, 5), (0, 0, -1)), ((0, 2, 5), (0, 0, -1)), ((0, 0, 1e13), (0, 0, -1)), ((0.5, 0, 5), (0, 0, -1)), ((0, 0, 0), (0, 0, 0))])
    keep = np.arange(5) != 2
    cst = {}
    clean = rl.occluded_rays(w, o[keep], d[keep], stats=cst)  # the zero direction among them: no hit, no flag
    assert cst["flagged"] == 0 and cst["rc"] == api.RL_OK and list(clean) == [True, False, True, False]
    want = w.hit_rays(o, d, allow_degenerate=True)["hit"] == 1
    assert want[2]
    st = {}
    counting = rl.occluded_rays(w, o, d, stats=st, allow_degenerate=True)
    assert st["flagged"] == 1 and st["rc"] == api.RL_E_DEGENERATE and st["rays"] == 5
    with pytest.raises(rl.RLError) as e:
        rl.occluded_rays(w, o, d, stats={})
    assert e.value.code == api.RL_E_DEGENERATE
    free = rl.occluded_rays(w, o, d, allow_degenerate=True)
    for got in (counting, free):
        assert np.array_equal(got, want) and np.array_equal(got[keep], clean)


# ----------------------------------------------------------------------------- 7. the C++ mirror
@pytest.mark.skipif(bool(os.environ.get("RL_RENDER_LIB")), reason="the C++ host mirror links librl_render.so (the product library)")
def test_cpp_mirror_probe_agrees_with_the_python_path(rl):
    rl.init(0)
    api = rl.api
    H = api.host_lib()
    H.rlh_occlusion_probe.argtypes = [C.c_void_p, C.c_uint64, C.c_double, C.c_double, C.c_void_p]
    world = rl.World.golden_test_scene()
    o, d, _ = _scene_rays(world, 11, 500, 100, 50, 0)
    rays = api.pack_rays(o, d)
    for tmin, tmax in ((1e-10, INF), (1e-10, 1.0), (0.0, 2.0)):
        out = np.full(rays.shape[0], 7, dtype=np.uint8)
        assert H.rlh_occlusion_probe(rays.ctypes.data, rays.shape[0], tmin, tmax, out.ctypes.data) == 0, H.rlh_last_error()
        want = rl.occluded_rays(world, o, d, tmin=tmin, tmax=tmax)
        assert np.array_equal(out, want.astype(np.uint8)) and 0 < want.sum() < want.size
