"""GPU tier: the end of a walk in the fast wave kernels (csrc/rl_rtiow_wave_body.inc).  A walk that hits nothing leaves a marker
(FAST_MISSED) and goes to GEN, which adds the background and counts the sample before anything else it does there; SHADE writes the next
ray over the old one whether the path goes on or not.  What can go wrong: a marker consumed late or twice (the stored pixel, the resumed
launch, the hand-over to a stealing wave, the per-sample store, the adaptive stop all read sum and n in GEN), a marker left behind by a
lane that waits in GEN without a pixel, and a sample that starts from a ray SHADE has overwritten.

Tiny frames, 61 x 34 (61 is no multiple of 8: slots outside the image).  Every fast form must give the bits, the ray count and the panic-site
count of its reference-order form (the counting render with stats=), the counting frame must be the CPU oracle's within the bar
test_gpu_fast_traversal.py uses, and the number of rays re-traced in the reference's order (slow_traces) must be what the commit before
this change counted for the same frame: PARENT_SLOW, recorded from one run of that commit's library."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H = 61, 34
MIN, EVERY = 4, 4  # adaptive: checkpoints at 4, 8, 12, ...
COUNTERS = ("rays", "node_tests", "sphere_tests", "rng_words", "flagged")

# slow_traces of the plain fast render, by (world, spp, max_depth): one run of the parent commit's library
PARENT_SLOW = {
    ("built", 1, 50): 10, ("built", 2, 50): 17, ("built", 8, 50): 59, ("built", 9, 50): 66, ("built", 72, 50): 480,
    ("built", 9, 0): 0, ("built", 9, 1): 46, ("built", 9, 2): 62,
    ("sky", 9, 50): 0, ("sky", 72, 50): 0,
    ("tiny", 9, 50): 18666, ("tiny", 9, 1): 18666, ("tiny", 72, 50): 149328,
}


def _materials(api):
    tex = np.zeros(5, dtype=api.TEXTURE)
    tex["kind"] = api.TEX_SOLID
    tex["color"] = [(0.2, 0.3, 0.1), (0.9, 0.9, 0.9), (0.7, 0.3, 0.3), (4.0, 4.0, 4.0), (0.0, 0.0, 0.0)]
    tex[4]["kind"], tex[4]["even"], tex[4]["odd"], tex[4]["inv_scale"] = api.TEX_CHECKER, 0, 1, 1.0 / 0.32
    mats = np.zeros(6, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 4  # checker ground
    mats[1]["kind"], mats[1]["texture"] = api.MAT_LAMBERTIAN, 2
    mats[2]["kind"], mats[2]["albedo"], mats[2]["fuzz"] = api.MAT_METAL, (0.8, 0.8, 0.8), 1.0  # rough: part of its rays are absorbed
    mats[3]["kind"], mats[3]["albedo"], mats[3]["fuzz"] = api.MAT_METAL, (0.7, 0.6, 0.5), 0.0  # polished: always reflected
    mats[4]["kind"], mats[4]["ior"] = api.MAT_DIELECTRIC, 1.5
    mats[5]["kind"], mats[5]["texture"] = api.MAT_DIFFUSE_LIGHT, 3
    return mats, tex


def _world(rl, centers, radii, material):
    api = rl.api
    mats, tex = _materials(api)
    sph = np.zeros(len(centers), dtype=api.SPHERE)
    sph["center0"], sph["center1"], sph["radius"], sph["material"], sph["moving"] = centers, centers, radii, material, 0
    return rl.World.from_spheres(sph, mats, tex, True)


def _built_world(rl):
    """The camera sits at the origin and looks down -z.  A ground sphere, three spheres of each material in a row across the view, and up
    against the sky a coincident pair (equal roots: those rays are re-traced in the reference's order, with a hit as the answer).  The
    upper rows see sky only."""
    centers, radii, material = [(0.0, -1001.6, -7.0)], [1000.0], [0]
    for i in range(15):
        centers.append((-3.5 + 0.5 * i, -1.35 + 0.1 * (i % 3), -6.0 - 0.4 * (i % 4))), radii.append(0.25), material.append(1 + i % 5)
    for m in (1, 3):
        centers.append((0.9, 0.4, -8.5)), radii.append(0.3), material.append(m)
    return _world(rl, centers, radii, material)


def _matte_world(rl):
    """Ground, five Lambertian spheres and a light, the camera at the origin: what the pinhole camera with the viewport 1e-31 away looks at
    (Metal and Dielectric normalise the incoming direction, and the reference asserts that its squared length is not about zero)."""
    centers, radii, material = [(0.0, -1001.6, -7.0)], [1000.0], [0]
    for i in range(6):
        centers.append((-2.5 + i, -1.2 + 0.1 * (i % 3), -6.0 - 0.4 * (i % 4))), radii.append(0.4), material.append(5 if i == 3 else 1)
    return _world(rl, centers, radii, material)


def _camera(rl, spp, depth, focus=7.0, defocus=0.3):
    p = rl.CameraParams(aspect_ratio=16.0 / 9.0, image_width=W, samples_per_pixel=spp, max_depth=depth, vfov=50.0, lookfrom=(0.0, 0.0, 0.0), lookat=(0.0, 0.0, -1.0),
                        defocus_angle=defocus, focus_dist=focus, background=(0.6, 0.7, 0.9), seed=11)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (W, H)
    return cam


_cache = {}


def _scene(rl, oracle, name, spp, depth):
    """(world, camera, counting frame, its counters): the reference-order render, pinned to the CPU oracle once and then only read.
    "built": the world above.  "sky": one sphere behind the camera, every sample ends inside GEN's own start_ray.  "tiny": the matte
    world through a pinhole camera whose viewport is 1e-31 away, so every camera ray's direction is outside the binary32 filter's range:
    each is re-traced in the reference's order from the start, with a miss as the answer on the sky pixels and a hit on the others."""
    if "world_" + name not in _cache:
        _cache["world_" + name] = {"sky": lambda: _world(rl, [(0.0, 0.0, 5.0)], [1.0], [1]), "built": lambda: _built_world(rl), "tiny": lambda: _matte_world(rl)}[name]()
    world = _cache["world_" + name]
    key = (name, spp, depth)
    if key not in _cache:
        cam = _camera(rl, spp, depth, *((1e-31, 0.0) if name == "tiny" else ()))
        gs, cs = {}, {}
        counting = cam.render(world, stats=gs).data
        cpu = oracle.rtiow_render(world.desc, cam.c, stats=cs)
        for k in COUNTERS:
            assert gs[k] == cs[k], (key, k, gs[k], cs[k])
        assert gs["flagged"] == 0
        assert np.abs(counting - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())
        counting.setflags(write=False)
        _cache[key] = (cam, counting, gs)
    return (world,) + _cache[key]


def _bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _timed(rl, cam, world, row_first=0, row_step=1):
    """Counter-free render (the kernels bench.py times) -> (frame, status)."""
    import torch
    dev = torch.device("cuda", 0)
    nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    buf = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, row_first=row_first, row_step=row_step)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


@pytest.fixture
def wave_kernels(rl):
    """Small frames through the wave-scheduled kernels (not the cooperative one), no stealing; every switch back to its default afterwards."""
    api = rl.api
    rl.init(0)
    api.set_coop(False), api.set_steal(0.0)
    yield api
    api.set_coop(True), api.set_fast_traversal(True), api.set_steal(3.0), api.set_pixel_entry(3), api.set_indep_k(1), api.set_lpt(True)


def _check_plain(rl, oracle, name, spp, depth):
    world, cam, counting, gs = _scene(rl, oracle, name, spp, depth)
    plain, st = _timed(rl, cam, world)
    print(f"walk_end slow_traces {(name, spp, depth)}: {st['slow_traces']}  rays {st['rays']}  flagged {st['flagged']}")
    assert _bits(plain, counting)
    assert st["rays"] == gs["rays"] and st["flagged"] == gs["flagged"]
    assert st["slow_traces"] == PARENT_SLOW[name, spp, depth]
    return world, cam, counting, gs, st


@pytest.mark.parametrize("spp", [1, 2, 8, 9, 72])
def test_sample_counts(rl, oracle, wave_kernels, spp):
    """1: the deferred miss is the only event before the pixel is stored.  8, 9: around the probe launch's length.  72: the probe launch's
    last sample may end in a deferred miss; the tile sort runs and the resumed launch continues from the stored sum and word position."""
    world, cam, counting, gs, st = _check_plain(rl, oracle, "built", spp, 50)
    assert st["slow_traces"] > 0  # the coincident pair
    assert gs["rays"] > spp * W * H  # scattered rays
    if spp == 1:
        assert (counting[0] == np.array([0.6, 0.7, 0.9])).all()  # a sky row: the background itself
    wave_kernels.set_lpt(False)  # one launch: no resume
    single, st1 = _timed(rl, cam, world)
    wave_kernels.set_lpt(True)
    assert _bits(single, counting) and st1["rays"] == gs["rays"] and st1["slow_traces"] == st["slow_traces"]


@pytest.mark.parametrize("depth", [0, 1, 2, 50])
def test_depths(rl, oracle, wave_kernels, depth):
    """Depth 1: every hit ends in SHADE, which has overwritten o and d by then; the next sample must still be right.  Depth 0: no ray at all."""
    world, cam, counting, gs, st = _check_plain(rl, oracle, "built", 9, depth)
    if depth == 0:
        assert gs["rays"] == 0 and not counting.any()
    if depth == 1:
        assert gs["rays"] == 9 * W * H  # camera rays only


@pytest.mark.parametrize("spp", [9, 72])
def test_all_sky_frame(rl, oracle, wave_kernels, spp):
    """Every sample ends inside GEN's own start_ray: the marker is consumed at the lane's next GEN visit, the last one before the store."""
    world, cam, counting, gs, st = _check_plain(rl, oracle, "sky", spp, 50)
    assert gs["rays"] == spp * W * H and st["slow_traces"] == 0
    for root in (0, 3):  # with the entry table the walk has no step at all; without it, it starts at the root
        wave_kernels.set_pixel_entry(root)
        frame, st_r = _timed(rl, cam, world)
        wave_kernels.set_pixel_entry(3)
        assert _bits(frame, counting) and st_r["rays"] == gs["rays"]


@pytest.mark.parametrize("spp,depth", [(9, 50), (9, 1), (72, 50)])
def test_retraced_camera_rays_hit_and_miss(rl, oracle, wave_kernels, spp, depth):
    """FAST_SLOW with a miss as the re-trace's answer (SHADE closes the sample: p == o, nd == d) and with a hit."""
    world, cam, counting, gs, st = _check_plain(rl, oracle, "tiny", spp, depth)
    assert st["slow_traces"] >= spp * W * H  # every camera ray
    assert (counting[0] == counting[0, 0]).all() and counting[0].all()  # a sky row: the re-trace's answer is a miss
    assert counting[-1].std() > 0 if depth > 1 else not counting[-1].any()  # a ground row: a hit (at depth 1 the path ends there, black)


def test_other_instantiations(rl, oracle, wave_kernels):
    """The 72-sample frame through every other kernel that includes the body."""
    import torch
    api = wave_kernels
    world, cam, counting, gs = _scene(rl, oracle, "built", 72, 50)
    dev = torch.device("cuda", 0)

    # RL_PIXEL_ENTRY=0: camera rays start at the root
    api.set_pixel_entry(0)
    root, st_root = _timed(rl, cam, world)
    api.set_pixel_entry(3)
    assert _bits(root, counting) and st_root["rays"] == gs["rays"] and st_root["slow_traces"] == PARENT_SLOW["built", 72, 50]

    # the work-stealing instantiation: the resumed launch of a row shard (hand-over at a sample boundary, right after a deferred miss too)
    api.set_steal(3.0)
    shard, st_shard = _timed(rl, cam, world, 1, 2)
    api.set_steal(0.0)
    gs_shard = {}
    assert _bits(shard, cam.render_rows(world, 1, 2, stats=gs_shard)) and st_shard["rays"] == gs_shard["rays"] and st_shard["flagged"] == gs_shard["flagged"]
    assert _bits(shard, counting[1::2])

    # the sample-parallel kernel, k = 1 and k = 4, against its own counting form
    frames = []
    for k in (1, 4):
        api.set_indep_k(k)
        buf = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev)
        cam.render_independent_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        st_k = api.render_status(world)
        gs_k = {}
        counted = cam.render_independent_rows(world, 0, 1, stats=gs_k)
        assert _bits(buf.cpu().numpy(), counted) and st_k["rays"] == gs_k["rays"] and st_k["flagged"] == gs_k["flagged"] == 0, k
        frames.append((counted, gs_k["rays"]))
    api.set_indep_k(1)
    assert _bits(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]

    # the moments kernel: its sums are the plain frame, its squares those of the reference-order layout
    ms = {}
    mom = cam.render_moments(world, stats=ms)
    api.set_fast_traversal(False)
    mom_ref = cam.render_moments(world)
    api.set_fast_traversal(True)
    assert _bits(mom.sums, counting) and _bits(mom.sq, mom_ref.sq) and _bits(mom_ref.sums, counting) and ms["rays"] == gs["rays"]

    # an adaptive render with checkpoints at 4, 8, 12, ...: sky pixels stop at the first one, each of their samples a deferred miss
    bound = 1e-6
    ad = cam.render_adaptive(world, MIN, EVERY, abs_variance=bound)
    api.set_fast_traversal(False)
    ad_ref = cam.render_adaptive(world, MIN, EVERY, abs_variance=bound)
    api.set_fast_traversal(True)
    assert np.array_equal(ad.counts, ad_ref.counts) and _bits(ad.sums, ad_ref.sums) and _bits(ad.sq, ad_ref.sq)
    assert (ad.counts[0] == MIN).all()
    full = ad.counts == 72
    assert full.any() and _bits(ad.sums[full], counting[full]) and _bits(ad.sq[full], mom.sq[full])

    # a pixel-list render of a scattered subset (sky, spheres, ground, the last column and row; unsorted, one duplicate)
    rng = np.random.default_rng(5)
    xs = np.concatenate([rng.integers(0, W, 40), [W - 1, 0, W - 1, 7, 7]]).astype(np.uint32)
    ys = np.concatenate([rng.integers(0, H, 40), [H - 1, H - 1, 0, 20, 20]]).astype(np.uint32)
    out = cam.render_pixels(world, xs, ys)
    assert _bits(out, np.ascontiguousarray(counting[ys, xs]))
