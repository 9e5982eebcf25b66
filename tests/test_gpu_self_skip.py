"""GPU tier: the self-test skip of the fast sphere traversal (csrc/rl_rtiow_wave.h fast_self_miss).  A scattered ray skips its test of
the sphere it has just left when SHADE has proven that test accepts no root >= 1e-10.  Frames of the timed kernel must still equal the
counting kernel's bit for bit, with the same ray and panic-site counts, in the worlds where self-hits ("acne") and grazing exits happen:
a huge ground sphere under a low camera, moving spheres, glass spheres that rays leave from the inside, fuzzy metal, tiny spheres on a
big one — through the plain launch, the cost-sorted resumed launch (spp >= 64) and the work-stealing instantiation on a row shard."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _fast_tree(rl, world):
    L = rl.api.render_lib()
    out = (C.c_uint64 * 16)()
    assert L.rl_debug_host_structures(world.desc, out) == 0, L.rl_last_error().decode()
    return bool(out[0] & 1)


def _timed(rl, cam, world, row_first=0, row_step=1):
    import torch
    dev = torch.device("cuda", 0)
    nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    buf = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, row_first=row_first, row_step=row_step)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _check(rl, world, p):
    """The timed fast kernel (wave-scheduled, not the cooperative small-frame kernel) against the counting kernel."""
    assert _fast_tree(rl, world)  # the world is one the fast traversal takes
    cam = rl.Camera(p)
    try:
        rl.api.set_coop(False)
        rl.api.set_rtiow_variant(1029)
        timed, st = _timed(rl, cam, world)
    finally:
        rl.api.set_rtiow_variant(0)
        rl.api.set_coop(True)
    gs = {}
    counting = cam.render(world, stats=gs).data
    assert _same_bits(timed, counting)
    assert st["rays"] == gs["rays"] and st["flagged"] == gs["flagged"] == 0
    assert gs["rays"] * 10 > 13 * cam.c.image_width * cam.c.image_height * p.samples_per_pixel  # many secondary rays: the skip is exercised
    return gs


@pytest.mark.parametrize("radius", [1e3, 1e4, 1e5])
def test_huge_ground_sphere_under_a_grazing_camera(rl, radius):
    """Rays that leave a huge sphere at grazing angles: the rounded hit point's error is as large as the self-intersection root, so
    some of them do hit the ground again at t >= 1e-10 and must not skip."""
    k = max(1.0, radius / 1e3)  # the small spheres scale with the ground so that the scene keeps its fast structure (normals_safe)

    def build(b):
        ground = b.lambertian(b.solid((0.5, 0.5, 0.5))) if radius < 1e4 else b.metal((0.7, 0.7, 0.7), 0.4)
        items = [b.sphere((0, -radius, 0), radius, ground)]
        for i in range(-3, 4):
            m = [b.lambertian(b.solid((0.8, 0.3, 0.2))), b.metal((0.8, 0.8, 0.9), 0.0), b.dielectric(1.5)][(i + 3) % 3]
            items.append(b.sphere((1.3 * k * i, 0.5 * k, -3.0 * k - abs(i) * k), 0.5 * k, m))
        return b.bvh(items)

    world = rl.World.build(build)
    p = rl.CameraParams(aspect_ratio=2.0, image_width=128, samples_per_pixel=6, max_depth=50, vfov=40.0, lookfrom=(0, 0.05 * k, 4.0 * k),
                        lookat=(0, 0.02 * k, -20.0 * k), background=(0.7, 0.8, 1.0), seed=11)
    _check(rl, world, p)


def _mixed_world(rl, seed):
    """A big sphere with tiny ones on its top, moving spheres, glass spheres (thick and thin), fuzzy metal of every fuzz."""
    rng = np.random.default_rng(seed)

    def build(b):
        items = [b.sphere((0, -50, 0), 50.0, b.lambertian(b.solid((0.4, 0.5, 0.4))))]
        for _ in range(40):  # tiny spheres resting on the big one
            x, z = rng.uniform(-3, 3, 2)
            r = rng.uniform(0.01, 0.05)
            y = np.sqrt(50.0 ** 2 - x * x - z * z) - 50.0 + r
            m = [b.lambertian(b.solid(tuple(rng.uniform(0.1, 0.9, 3)))), b.metal((0.9, 0.9, 0.9), float(rng.uniform(0, 1))), b.dielectric(1.5)][rng.integers(0, 3)]
            items.append(b.sphere((x, y, z), r, m))
        for _ in range(12):  # glass: rays leave these from the inside
            c = (rng.uniform(-3, 3), rng.uniform(0.3, 1.2), rng.uniform(-3, 1))
            items.append(b.sphere(c, float(rng.uniform(0.2, 0.8)), b.dielectric(float(rng.uniform(1.1, 2.4)))))
        for _ in range(12):  # moving spheres
            c = np.array([rng.uniform(-3, 3), rng.uniform(0.2, 1.0), rng.uniform(-3, 1)])
            m = b.metal(tuple(rng.uniform(0.5, 1.0, 3)), float(rng.uniform(0, 0.8))) if rng.random() < 0.5 else b.lambertian(b.solid((0.7, 0.2, 0.2)))
            items.append(b.sphere(tuple(c), float(rng.uniform(0.1, 0.4)), m, center2=tuple(c + rng.uniform(-0.3, 0.3, 3))))
        return b.bvh(items)

    return rl.World.build(build)


@pytest.mark.parametrize("seed", [1, 2])
def test_glass_moving_fuzzy_metal_and_tiny_spheres_on_a_big_one(rl, seed):
    world = _mixed_world(rl, seed)
    p = rl.CameraParams(aspect_ratio=1.5, image_width=120, samples_per_pixel=8, max_depth=50, vfov=45.0, lookfrom=(0.5, 0.6, 5.0),
                        lookat=(0, 0.3, -1), defocus_angle=0.5, focus_dist=5.0, background=(0.6, 0.7, 0.9), seed=seed)
    _check(rl, world, p)


def test_resumed_lpt_launch(rl):
    """spp >= 64: the cost-sorted second launch resumes every pixel; the self entry starts cleared with every camera ray."""
    world = _mixed_world(rl, 3)
    p = rl.CameraParams(aspect_ratio=1.5, image_width=48, samples_per_pixel=72, max_depth=50, vfov=45.0, lookfrom=(0.5, 0.4, 5.0),
                        lookat=(0, 0.3, -1), background=(0.6, 0.7, 0.9), seed=4)
    _check(rl, world, p)


def test_stealing_shard(rl):
    """The work-stealing instantiation rtiow_wave_kernel<1024, 4, false, true> on a 1/4 row shard, against the counting kernel's rows.
    The shard lies between the cooperative kernel's small-frame limit and the stealing rule's ceiling (3 x the lanes of 256 CUs), so the
    automatic choice is the wave-scheduled fast kernel with stealing in its resume launch; stealing off must render the same bits."""
    world = _mixed_world(rl, 5)
    assert _fast_tree(rl, world)
    p = rl.CameraParams(aspect_ratio=1.5, image_width=960, samples_per_pixel=64, max_depth=50, vfov=45.0, lookfrom=(0.5, 0.6, 5.0),
                        lookat=(0, 0.3, -1), background=(0.6, 0.7, 0.9), seed=5)
    cam = rl.Camera(p)
    shard = 4
    npix = rl.api.rows_for(cam.c.image_height, 1, shard) * cam.c.image_width
    assert 40960 < npix <= 3 * 256 * 1024  # above the cooperative kernel's small-frame limit, within the stealing rule
    frames = []
    try:
        for fill in (3.0, 0.0):  # stealing on / off
            rl.api.set_steal(fill)
            frames.append(_timed(rl, cam, world, 1, shard))
    finally:
        rl.api.set_steal(3.0)
    (img, st), (img_off, st_off) = frames
    gs = {}
    counting = cam.render_rows(world, 1, shard, stats=gs)
    assert _same_bits(img, counting) and _same_bits(img_off, counting)
    assert gs["rays"] == st["rays"] == st_off["rays"] and st["flagged"] == gs["flagged"] == 0
