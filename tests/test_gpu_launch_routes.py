"""GPU tier: every route of the RTIOW launch tables (csrc/rl_rtiow_launch.h).

The four launchers (frame / moments / adaptive, sample-parallel, pixel lists, path query) pick their kernel instantiation from one table per
kernel family, by the scene's flags: a sphere-only world with the fast structure, and general worlds with and without transcendental
texture code (`trans`: a Noise texture) and with and without a ConstantMedium (`media`).  Five tiny worlds cover the four (trans, media)
flavours and the sphere kernels; on each, every entry point runs counter-free and counting, and the identities the project states
elsewhere (tests/test_gpu_wave_block_paths.py, test_gpu_render_pixels.py, test_gpu_render_moments.py, test_gpu_render_adaptive.py,
test_gpu_independent_samples.py, test_gpu_path_query.py) must hold bit for bit.  A wrong table row that still renders the right bits (TRANS
set on a scene without Noise) is not visible here: that is what the launch trace of profiles/rtiow_launch_tables.txt is for.

24 x 16 pixels at 64 spp (>= 64: the probe launch, the tile sort and the resumed launch run), depth 6."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 24, 16, 64, 6
MIN, EVERY = 4, 4
WORLDS = ["spheres", "quads", "quads_noise", "media", "media_noise"]


def _restore(api):
    api.set_coop(True), api.set_fast_traversal(True), api.set_steal(3.0), api.set_indep_k(1), api.set_fastg_one_wave(-1), api.set_lpt(True)


@pytest.fixture(autouse=True)
def _switches(rl, request):
    rl.init(0)
    request.addfinalizer(lambda: _restore(rl.api))


def _sphere_world(rl):
    """12 spheres: ground, a 3 x 3 field of every material (two moving), a glass ball and a light."""
    api = rl.api
    tex = np.zeros(3, dtype=api.TEXTURE)
    tex["kind"] = api.TEX_SOLID
    tex["color"] = [(0.5, 0.5, 0.5), (0.7, 0.3, 0.3), (4.0, 4.0, 4.0)]
    mats = np.zeros(5, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 0
    mats[1]["kind"], mats[1]["texture"] = api.MAT_LAMBERTIAN, 1
    mats[2]["kind"], mats[2]["albedo"], mats[2]["fuzz"] = api.MAT_METAL, (0.8, 0.8, 0.8), 0.3
    mats[3]["kind"], mats[3]["ior"] = api.MAT_DIELECTRIC, 1.5
    mats[4]["kind"], mats[4]["texture"] = api.MAT_DIFFUSE_LIGHT, 2
    centers, center1, radii, material, moving = [(0.0, -100.0, 0.0)], [(0.0, -100.0, 0.0)], [100.0], [0], [0]
    for i in range(9):
        x, z = -1.6 + 1.6 * (i % 3), -1.2 + 1.2 * (i // 3)
        centers.append((x, 0.3, z)), radii.append(0.3), material.append(1 + i % 3), moving.append(int(i % 4 == 0))
        center1.append((x, 0.3 + (0.3 if i % 4 == 0 else 0.0), z))
    for c, r, m in [((0.0, 1.3, 0.0), 0.5, 3), ((1.8, 1.6, -0.8), 0.3, 4)]:
        centers.append(c), center1.append(c), radii.append(r), material.append(m), moving.append(0)
    sph = np.zeros(len(centers), dtype=api.SPHERE)
    sph["center0"], sph["center1"], sph["radius"], sph["material"], sph["moving"] = centers, center1, radii, material, moving
    assert len(sph) == 12
    return rl.World.from_spheres(sph, mats, tex, True)


def _general_world(rl, noise, media):
    def scene(b):
        grey = b.lambertian(b.solid((0.6, 0.6, 0.6)))
        wall = b.lambertian(b.noise(4.0, 7)) if noise else b.lambertian(b.solid((0.7, 0.3, 0.3)))
        objs = [b.quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), grey), b.quad((-3, 0, -3), (6, 0, 0), (0, 4, 0), wall),
                b.quad((-1, 3.5, -1), (2, 0, 0), (0, 0, 2), b.diffuse_light(b.solid((4.0, 4.0, 4.0)))),
                b.triangle((-2.2, 0, 0.5), (1.5, 0, 0), (0, 1.8, 0), b.metal((0.8, 0.8, 0.8), 0.1))]
        if media:
            flat, (x0, y0, z0), (dx, dy, dz) = b.flat(), (0.2, 0.0, -1.0), (1.6, 1.6, 1.6)
            box = [b.quad((x0, y0, z0), (dx, 0, 0), (0, dy, 0), flat), b.quad((x0, y0, z0 + dz), (dx, 0, 0), (0, dy, 0), flat),
                   b.quad((x0, y0, z0), (0, dy, 0), (0, 0, dz), flat), b.quad((x0 + dx, y0, z0), (0, dy, 0), (0, 0, dz), flat),
                   b.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), flat), b.quad((x0, y0 + dy, z0), (dx, 0, 0), (0, 0, dz), flat)]
            return b.list([b.bvh(objs), b.constant_medium(b.list(box), 0.8, b.isotropic(b.solid((0.9, 0.9, 0.9))))])
        return b.bvh(objs)
    return rl.World.build(scene)


_cache = {}


def _scene(rl, name):
    """World, camera, the 40 listed pixels, and the yardstick: the counting frame and the counting moments (reference-order kernel, whatever
    the switches say).  Built once, with the switches at their defaults, and never written to afterwards."""
    if name not in _cache:
        _restore(rl.api)
        world = _sphere_world(rl) if name == "spheres" else _general_world(rl, "noise" in name, "media" in name)
        cam = rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=W, samples_per_pixel=SPP, max_depth=DEPTH, vfov=50.0, lookfrom=(0.0, 1.8, 6.0),
                                        lookat=(0.0, 1.0, 0.0), defocus_angle=0.3, focus_dist=6.0, background=(0.6, 0.7, 0.9), seed=5))
        assert (cam.c.image_width, cam.c.image_height) == (W, H)
        pick = np.random.default_rng(3).choice(np.setdiff1d(np.arange(W * H), [0, W - 1, W * (H - 1), W * H - 1]), 36, replace=False)
        pick = np.concatenate([[0, W - 1, W * (H - 1), W * H - 1], pick]).astype(np.uint32)
        ys, xs = np.divmod(pick, np.uint32(W))
        gs, ms = {}, {}
        frame = cam.render(world, stats=gs).data
        mom = cam.render_moments(world, stats=ms)
        for a in (frame, mom.sums, mom.sq):
            a.setflags(write=False)
        assert gs["flagged"] == 0 and ms["rays"] == gs["rays"] and _bits(mom.sums, frame)
        if name == "spheres":
            assert rl.api.fast_tree(world) is not None
        # the adaptive bound, from the yardstick alone: an eighth of the mean per-sample variance (largest channel).  A pixel stops at
        # checkpoint n when its variance of the mean, about its per-sample variance / n, is below it: from n = 8 on that is every pixel
        # of below-average variance, and the pixels of a constant colour (sky, light) stop at the first checkpoint.
        var = np.maximum((mom.sq - mom.sums * mom.sums / SPP) / (SPP - 1), 0.0).max(axis=-1)
        bound = float(var.mean()) / 8.0
        assert bound > 0.0 and np.isfinite(bound)
        _cache[name] = dict(world=world, cam=cam, xs=xs, ys=ys, frame=frame, rays=gs["rays"], mom=mom, bound=bound)
    return _cache[name]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _device_call(rl, world, shapes, call):
    """A counter-free `_device` call into NaN- / 0xFF-filled buffers -> (host arrays, status)."""
    import torch
    dev = torch.device("cuda", 0)
    bufs = [torch.full(s, float("nan"), dtype=torch.float64, device=dev) if dt is np.float64 else torch.full(s, -1, dtype=torch.int32, device=dev) for s, dt in shapes]
    call(torch.cuda.current_stream(dev).cuda_stream, *[b.data_ptr() for b in bufs])
    st = rl.api.render_status(world)
    return [b.cpu().numpy() if dt is np.float64 else b.cpu().numpy().view(np.uint32) for b, (_, dt) in zip(bufs, shapes)], st


def _frame(rl, S, row_first=0, row_step=1):
    cam, world = S["cam"], S["world"]
    nrows = rl.api.rows_for(H, row_first, row_step)
    (out,), st = _device_call(rl, world, [((nrows, W, 3), np.float64)], lambda stream, d: cam.render_device(world, d, stream=stream, row_first=row_first, row_step=row_step))
    return out, st


def _indep(rl, S):
    cam, world = S["cam"], S["world"]
    (out,), st = _device_call(rl, world, [((H, W, 3), np.float64)], lambda stream, d: cam.render_independent_device(world, d, stream=stream))
    return out, st


def _moments(rl, S):
    cam, world = S["cam"], S["world"]
    (sums, sq), st = _device_call(rl, world, [((H, W, 3), np.float64)] * 2, lambda stream, d0, d1: cam.render_moments_device(world, d0, d1, stream=stream))
    return sums, sq, st


def _adaptive(rl, S):
    cam, world = S["cam"], S["world"]
    (sums, sq, counts), _ = _device_call(rl, world, [((H, W, 3), np.float64)] * 2 + [((H, W), np.uint32)],
                                         lambda stream, d0, d1, d2: cam.render_adaptive_device(world, MIN, EVERY, d0, d1, d2, abs_variance=S["bound"], stream=stream))
    return sums, sq, counts


def _check_frame_and_list(rl, S, what):
    """The counter-free frame and list (with indep the calls that have a one-wave-per-SIMD form; on sphere worlds a cooperative form)."""
    cam, world, xs, ys, frame = S["cam"], S["world"], S["xs"], S["ys"], S["frame"]
    out, st = _frame(rl, S)
    assert _bits(out, frame) and st["rays"] == S["rays"] and st["flagged"] == 0, (what, "frame")
    px = cam.render_pixels(world, xs, ys)
    assert _bits(px, frame[ys, xs]), (what, "pixels")
    return out, px


@pytest.mark.parametrize("name", WORLDS)
def test_every_entry_point_reaches_a_kernel_that_renders_the_reference_bits(rl, name):
    api = rl.api
    S = _scene(rl, name)
    cam, world, xs, ys, frame, mom = S["cam"], S["world"], S["xs"], S["ys"], S["frame"], S["mom"]

    # 1, 2: the frame, counter-free == counting; 5: listed pixels == the frame's pixels (counter-free and counting)
    _check_frame_and_list(rl, S, name)
    ps = {}
    assert _bits(cam.render_pixels(world, xs, ys, stats=ps), frame[ys, xs]) and ps["flagged"] == 0

    # 3, 4: sample-parallel, k = 1 == k = 3 == its own counting form
    frames = []
    for k in (1, 3):
        api.set_indep_k(k)
        fast, st = _indep(rl, S)
        gs = {}
        counted = cam.render_independent_rows(world, 0, 1, stats=gs)
        assert _bits(fast, counted) and st["rays"] == gs["rays"] and gs["flagged"] == 0, (name, k)
        frames.append((fast, gs["rays"]))
    api.set_indep_k(1)
    assert _bits(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]

    # 6: moments sums == the frame, squares == their reference-order form; 7: the list's moments == the frame's at the listed pixels
    sums, sq, st = _moments(rl, S)
    assert _bits(sums, frame) and _bits(sq, mom.sq) and st["rays"] == S["rays"]
    psums, psq = cam.render_pixels_moments(world, xs, ys)
    assert _bits(psums, frame[ys, xs]) and _bits(psq, mom.sq[ys, xs])
    api.set_fast_traversal(False)
    sums_ref, sq_ref, _ = _moments(rl, S)
    psums_ref, psq_ref = cam.render_pixels_moments(world, xs, ys)
    api.set_fast_traversal(True)
    assert _bits(sums_ref, frame) and _bits(sq_ref, sq) and _bits(psums_ref, psums) and _bits(psq_ref, psq)

    # 8: adaptive counts, sums and squares == their reference-order form; the bound stops some pixels
    a_sums, a_sq, a_counts = _adaptive(rl, S)
    api.set_fast_traversal(False)
    r_sums, r_sq, r_counts = _adaptive(rl, S)
    api.set_fast_traversal(True)
    assert _bits(a_counts, r_counts) and _bits(a_sums, r_sums) and _bits(a_sq, r_sq)
    print(name, "adaptive counts", dict(zip(*[v.tolist() for v in np.unique(a_counts, return_counts=True)])))
    assert (a_counts < SPP).any() and (a_counts >= MIN).all() and (a_counts <= SPP).all()
    full = a_counts == SPP
    assert _bits(a_sums[full], frame[full]) and _bits(a_sq[full], mom.sq[full])

    # 9: path-query colours of the 40 camera rays == their counting form, with the same out-cursors
    p = cam.params
    rays, cur = cam.get_rays(xs, ys, api.pack_cursors(xs.astype(np.uint64) * np.uint64(W) + ys.astype(np.uint64)))
    rgb, out_cur, counts = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays)
    assert api.last_query()["kernel"] == "fast"
    qs = {}
    rgb_c, out_cur_c, counts_c = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays, stats=qs)
    assert api.last_query()["kernel"] == "reference"
    assert _bits(rgb, rgb_c) and _bits(out_cur, out_cur_c) and np.array_equal(counts, counts_c) and qs["rays"] == int(counts.sum()) and qs["flagged"] == 0


@pytest.mark.parametrize("one_wave", [1, 0])
def test_both_forms_of_the_media_and_noise_flavour(rl, one_wave):
    """The flavour with both the media and the transcendental code: forced into / out of its one-wave-per-SIMD form (frame, indep, pixels)."""
    S = _scene(rl, "media_noise")
    rl.api.set_fastg_one_wave(one_wave)
    _check_frame_and_list(rl, S, one_wave)
    fast, st = _indep(rl, S)
    gs = {}
    assert _bits(fast, S["cam"].render_independent_rows(S["world"], 0, 1, stats=gs)) and st["rays"] == gs["rays"]


@pytest.mark.parametrize("coop", [False, True])
def test_sphere_world_through_the_cooperative_and_the_wave_kernel(rl, coop):
    """Frame and list with and without the cooperative kernel; and the stealing instantiation: the resumed launch of a row shard."""
    S = _scene(rl, "spheres")
    rl.api.set_coop(coop)
    _check_frame_and_list(rl, S, coop)
    rl.api.set_steal(3.0)
    shard, st = _frame(rl, S, 1, 2)
    gs = {}
    assert _bits(shard, S["cam"].render_rows(S["world"], 1, 2, stats=gs)) and st["rays"] == gs["rays"]
    assert _bits(shard, S["frame"][1::2])
