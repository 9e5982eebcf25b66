"""GPU tier: every way into and out of the wave scheduler's blocks (csrc/rl_rtiow_wave_body.inc), through every kernel that includes
the body.  The blocks are separate uniform `if`s around divergent code; what can go wrong in such a body are its
entries and exits — a lane that leaves TRAV for LEAF, SHADE or GEN, a miss that ends a sample inside the walk, a sky sample that ends
inside GEN, a FAST_SLOW re-trace, a path that dies by depth, a pixel that stops at a checkpoint, a resumed pixel, a stolen pixel.

One small frame that takes all of them, 64 x 36 at 72 spp (>= 64: the probe launch, the device-side tile sort and the resumed launch
run), is rendered by the plain fast kernel, without the per-pixel entry table, by the work-stealing instantiation on a row shard, by the
sample-parallel kernel with k = 1 and k = 4, by the moments kernel, and by an adaptive render that stops some pixels at its first
checkpoint.  No tolerance between GPU forms: each must give the bits of its reference-order form (the counting render with stats=,
the LDS_SCENE = 3 layout), and the counting frame must be the CPU oracle's within the tight bar test_gpu_fast_traversal.py uses.

Equal bits do not tell which kernel rendered them, so every step also asserts, from the library's launch log (api.rtiow_launches), the
instantiation its comment names.  (That is how the moments and adaptive steps were found to have compared the counting reference-order
kernel with itself: Camera.render_moments and render_adaptive always count.  Their counter-free device forms now run beside them.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, SPP = 64, 72
MIN, EVERY = 4, 4  # adaptive: checkpoints at 4, 8 (inside the probe launch's samples [0, 8)), 12, ...
COUNTERS = ("rays", "node_tests", "sphere_tests", "rng_words", "flagged")


def _built_world(rl):
    """40 spheres: a checker ground, a field of small spheres of every material (some moving), and set apart against the sky a lone
    Lambertian sphere (pixels whose only entry is that leaf), a glass ball (both orientations), a light, a rough and a polished
    metal ball, and a coincident pair (equal roots: FAST_SLOW re-traces).  The upper rows of the frame see sky only."""
    api = rl.api
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
    rng = np.random.default_rng(7)
    centers, radii, material, moving, center1 = [(0.0, -1000.0, 0.0)], [1000.0], [0], [0], [(0.0, -1000.0, 0.0)]
    for i in range(32):  # the field: a 8 x 4 grid, jittered
        x, z = -3.5 + (i % 8) + 0.6 * rng.random(), -2.0 + 1.2 * (i // 8) + 0.5 * rng.random()
        centers.append((x, 0.2, z)), radii.append(0.2), material.append(1 + i % 5), moving.append(int(i % 3 == 0))
        center1.append((x, 0.2 + (0.4 * rng.random() if i % 3 == 0 else 0.0), z))
    for c, r, m in [((-2.5, 1.6, -1.0), 0.35, 1), ((0.0, 1.0, 0.0), 0.7, 4), ((2.4, 1.5, -1.0), 0.4, 5), ((-1.4, 0.9, 1.0), 0.45, 2), ((1.5, 0.8, 1.2), 0.45, 3),
                    ((0.9, 2.0, -1.5), 0.3, 1), ((0.9, 2.0, -1.5), 0.3, 3)]:  # the last two coincide
        centers.append(c), radii.append(r), material.append(m), moving.append(0), center1.append(c)
    sph = np.zeros(len(centers), dtype=api.SPHERE)
    sph["center0"], sph["center1"], sph["radius"], sph["material"], sph["moving"] = centers, center1, radii, material, moving
    assert len(sph) == 40
    world = rl.World.from_spheres(sph, mats, tex, True)
    p = rl.CameraParams(aspect_ratio=16.0 / 9.0, image_width=W, samples_per_pixel=SPP, max_depth=50, vfov=50.0, lookfrom=(0.0, 1.6, 7.0), lookat=(0.0, 1.6, 0.0),
                        defocus_angle=0.3, focus_dist=7.0, background=(0.6, 0.7, 0.9), seed=11)
    return world, p


_worlds = {}


def _scene(rl, name, depth):
    if name not in _worlds:
        if name == "bouncing_spheres":
            world = rl.World.bouncing_spheres(1)
            p = world.params
            p.image_width, p.samples_per_pixel = W, SPP
            _worlds[name] = (world, p)
        else:
            _worlds[name] = _built_world(rl)
    world, p = _worlds[name]
    p.max_depth = depth
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (64, 36)
    return world, cam


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


def _indep(rl, cam, world, k):
    """The sample-parallel mode with k samples per claim: (counter-free frame, its status, counting frame, its counters)."""
    import torch
    dev = torch.device("cuda", 0)
    rl.api.set_indep_k(k)
    buf = torch.full((cam.c.image_height, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_independent_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    st = rl.api.render_status(world)
    gs = {}
    counted = cam.render_independent_rows(world, 0, 1, stats=gs)
    return buf.cpu().numpy(), st, counted, gs


def _device(rl, world, shapes, call):
    """A counter-free `_device` call into NaN- / 0xFF-filled buffers -> (host arrays, status)."""
    import torch
    dev = torch.device("cuda", 0)
    bufs = [torch.full(s, float("nan"), dtype=torch.float64, device=dev) if dt is np.float64 else torch.full(s, -1, dtype=torch.int32, device=dev) for s, dt in shapes]
    call(torch.cuda.current_stream(dev).cuda_stream, *[b.data_ptr() for b in bufs])
    st = rl.api.render_status(world)
    return [b.cpu().numpy() if dt is np.float64 else b.cpu().numpy().view(np.uint32) for b, (_, dt) in zip(bufs, shapes)], st


# the instantiations the steps below name (1024 lanes, sphere layouts 4 = fast tree, 3 = guarded compact ops; the reference-order kernel)
FAST, STEALING, COUNTING = "rtiow_wave_kernel<1024, 4, false, false>", "rtiow_wave_kernel<1024, 4, false, true>", "rtiow_wave_kernel<1024, 3, true, false>"
INDEP, INDEP_COUNTING = "rtiow_wave_indep_kernel<1024, 4, false>", "rtiow_wave_general_indep_kernel<512, false, true, false>"
MOMENTS_FAST, MOMENTS_GUARD, MOMENTS_COUNTING = "rtiow_wave_moments_kernel<1024, 4>", "rtiow_wave_moments_kernel<1024, 3>", "rtiow_wave_general_moments_kernel<512, false, true, false>"
TWO = [(0, 8, 0, False), (8, SPP, 1, True)]  # the probe launch and the resumed launch in the sorted tile order
ONE = [(0, SPP, 0, False)]


class _Log:
    def __init__(self, api):
        self.api, self.total = api, api.rtiow_launch_total()

    def ran(self, kernels, flow, what):
        """The launches since the last call: these kernels, in this flow (sample range, resume, tile order)."""
        recs = self.api.rtiow_launches(self.total)
        self.total += len(recs)
        assert [r["kernel"] for r in recs] == kernels, (what, [r["kernel"] for r in recs])
        assert [(r["sample_begin"], r["sample_end"], r["resume"], r["tile_order"]) for r in recs] == flow, (what, recs)
        assert [r["steal_state"] for r in recs] == [k == STEALING for k in kernels], what
        return recs


@pytest.fixture
def wave_kernels(rl):
    """Small frames through the wave-scheduled kernels (not the cooperative one); every switch back to its default afterwards."""
    api = rl.api
    rl.init(0)
    api.set_coop(False)
    yield api
    api.set_coop(True), api.set_fast_traversal(True), api.set_steal(3.0), api.set_pixel_entry(3), api.set_indep_k(1), api.set_lpt(True)


@pytest.mark.parametrize("depth", [50, 3, 0])
@pytest.mark.parametrize("name", ["bouncing_spheres", "built"])
def test_every_instantiation_renders_the_reference_order_bits(rl, oracle, wave_kernels, name, depth):
    api = wave_kernels
    world, cam = _scene(rl, name, depth)
    # the yardstick: the reference-order counting render, pinned to the CPU oracle
    gs, cs = {}, {}
    log = _Log(api)
    counting = cam.render(world, stats=gs).data
    log.ran([COUNTING] * 2, TWO, "counting")
    cpu = oracle.rtiow_render(world.desc, cam.c, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    assert gs["flagged"] == 0
    assert np.abs(counting - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())
    if depth == 0:
        assert gs["rays"] == 0 and not counting.any()

    # plain fast kernel (probe launch + resumed launch, no stealing), with and without the per-pixel entry table
    api.set_steal(0.0)
    plain, st = _timed(rl, cam, world)
    log.ran([FAST] * 2, TWO, "plain")
    assert _bits(plain, counting) and st["rays"] == gs["rays"] and st["flagged"] == 0
    if name == "built" and depth:
        assert st["slow_traces"] > 0  # the coincident pair
        assert np.unique(api.pixel_entry_table(world, 64 * 36)).size > 3  # sky pixels, leaf-only pixels, pixels that enter at inner nodes
    api.set_pixel_entry(0)
    root, st_root = _timed(rl, cam, world)
    log.ran([FAST] * 2, TWO, "root walk")
    api.set_pixel_entry(3)
    assert _bits(root, counting) and st_root["rays"] == gs["rays"] and st_root["slow_traces"] == st["slow_traces"]
    api.set_lpt(False)  # one launch: no resume
    single, st_single = _timed(rl, cam, world)
    log.ran([FAST], ONE, "single launch")
    api.set_lpt(True)
    assert _bits(single, counting) and st_single["rays"] == gs["rays"] and st_single["slow_traces"] == st["slow_traces"]

    # the work-stealing instantiation: the resumed launch of a row shard
    api.set_steal(3.0)
    shard, st_shard = _timed(rl, cam, world, 1, 2)
    log.ran([FAST, STEALING], TWO, "stealing shard")
    state, n = api.steal_record(world, 18 * W)
    handed = n != api.NEVER_OFFERED
    print(name, depth, "pixels handed over on the shard:", int(handed.sum()), "of", 18 * W)
    assert (state == 3).all() and ((n[handed] >= 8) & (n[handed] < SPP)).all()
    if depth:  # (without a ray a sample is a few instructions: a wave that asks may find every pixel finished)
        assert handed.any()
    gs_shard = {}
    assert _bits(shard, cam.render_rows(world, 1, 2, stats=gs_shard)) and st_shard["rays"] == gs_shard["rays"]
    log.ran([COUNTING] * 2, TWO, "counting shard")
    assert _bits(shard, counting[1::2])
    api.set_steal(0.0)

    # the sample-parallel kernel, k = 1 and k = 4, against its own counting form
    frames = []
    for k in (1, 4):
        fast, st_k, counted, gs_k = _indep(rl, cam, world, k)
        log.ran([INDEP, INDEP_COUNTING], ONE * 2, ("indep", k))
        assert _bits(fast, counted) and st_k["rays"] == gs_k["rays"] and gs_k["flagged"] == 0, k
        frames.append((fast, gs_k["rays"]))
    api.set_indep_k(1)
    assert _bits(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]

    # the moments kernel: its sums are the plain frame, its squares those of the reference-order layout
    ms = {}
    mom = cam.render_moments(world, stats=ms)
    api.set_fast_traversal(False)
    mom_ref = cam.render_moments(world)
    api.set_fast_traversal(True)
    log.ran([MOMENTS_COUNTING] * 4, TWO * 2, "counting moments")  # (Camera.render_moments always counts: both are the reference-order kernel)
    assert _bits(mom.sums, counting) and _bits(mom.sq, mom_ref.sq) and _bits(mom_ref.sums, counting) and ms["rays"] == gs["rays"]
    frame_shape = [((36, W, 3), np.float64)] * 2
    (f_sums, f_sq), st_m = _device(rl, world, frame_shape, lambda stream, d0, d1: cam.render_moments_device(world, d0, d1, stream=stream))
    log.ran([MOMENTS_FAST] * 2, TWO, "moments, fast layout")
    api.set_fast_traversal(False)
    (g_sums, g_sq), st_g = _device(rl, world, frame_shape, lambda stream, d0, d1: cam.render_moments_device(world, d0, d1, stream=stream))
    api.set_fast_traversal(True)
    log.ran([MOMENTS_GUARD] * 2, TWO, "moments, guarded layout")
    assert _bits(f_sums, counting) and _bits(f_sq, mom.sq) and _bits(g_sums, counting) and _bits(g_sq, mom.sq)
    assert st_m["rays"] == gs["rays"] == st_g["rays"] and st_m["flagged"] == 0

    # an adaptive render: some pixels stop at the first checkpoint (inside the probe launch: they must not be resumed), others never
    bound = 1e-6
    ad = cam.render_adaptive(world, MIN, EVERY, abs_variance=bound)
    api.set_fast_traversal(False)
    ad_ref = cam.render_adaptive(world, MIN, EVERY, abs_variance=bound)
    api.set_fast_traversal(True)
    log.ran([MOMENTS_COUNTING] * 4, TWO * 2, "counting adaptive")  # (Camera.render_adaptive always counts)
    assert np.array_equal(ad.counts, ad_ref.counts) and _bits(ad.sums, ad_ref.sums) and _bits(ad.sq, ad_ref.sq)
    shapes = frame_shape + [((36, W), np.uint32)]
    for fast, kernel in ((True, MOMENTS_FAST), (False, MOMENTS_GUARD)):  # the stopping rule in the wave kernel's two layouts
        api.set_fast_traversal(fast)
        (d_sums, d_sq, d_counts), _ = _device(rl, world, shapes, lambda stream, d0, d1, d2: cam.render_adaptive_device(world, MIN, EVERY, d0, d1, d2, abs_variance=bound, stream=stream))
        api.set_fast_traversal(True)
        log.ran([kernel] * 2, TWO, ("adaptive", kernel))
        assert np.array_equal(d_counts, ad.counts) and _bits(d_sums, ad.sums) and _bits(d_sq, ad.sq), kernel
    assert (ad.counts == MIN).any()
    full = ad.counts == SPP
    if depth:
        assert full.any()
        assert _bits(ad.sums[full], counting[full]) and _bits(ad.sq[full], mom.sq[full])
    else:
        assert (ad.counts == MIN).all()
