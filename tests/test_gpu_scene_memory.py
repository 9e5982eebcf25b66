"""GPU tier (-m gpu): who owns the library's device memory (csrc/rl_devbuf.h).

Every device allocation of the library passes through one owning type, which counts what is alive (api.live_buffers(): count, bytes).
A scene owns its program's buffers and its work buffers (grown on demand by the renders that need them); a host-buffer call owns its
staging for the length of the call.  So: whatever a world was used for, dropping it brings the count back to where it was; a work buffer
that has grown, or is larger than the frame needs, renders the same bits as a fresh one; and the count follows the memory the driver
reports."""
import dataclasses
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_coop(True)
    rl.api.set_indep_cap(0)


def _baseline(rl):
    gc.collect()
    return rl.api.live_buffers()


def _spheres_cam(rl, world, width, spp=64):
    """bouncing_spheres at 16:9 and depth 8: 32x18, 64x36, 96x54."""
    p = dataclasses.replace(world.params, image_width=width, samples_per_pixel=spp, max_depth=8)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (width, width * 9 // 16)
    return cam


def _render_device(rl, cam, world):
    """The asynchronous (counter-free) render into a torch buffer -> the frame's sums."""
    import torch
    buf = torch.zeros((cam.c.image_height, cam.c.image_width, 3), dtype=torch.float64, device="cuda:0")
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    rl.api.render_status(world)
    return buf.cpu().numpy()


def test_every_work_buffer_is_created_and_released(rl, golden):
    api = rl.api
    base = _baseline(rl)
    try:
        world = rl.World.bouncing_spheres(1)
        api.set_coop(False)  # 64x36 through the wave-scheduled fast kernel: cost-sorted (LPT) buffers, sort scratch, stealing, pixel entries
        _render_device(rl, _spheres_cam(rl, world, 64), world)
        after_wave = api.live_buffers()
        assert after_wave > base
        api.set_coop(True)  # the cooperative kernel's pixel list
        _render_device(rl, _spheres_cam(rl, world, 32), world)
        after_coop = api.live_buffers()
        assert after_coop[0] > after_wave[0] and after_coop[1] > after_wave[1]
        _spheres_cam(rl, world, 32).render(world, stats={})  # counting render through the host-buffer entry: its staging is gone again
        assert api.live_buffers() == after_coop
        cam8 = _spheres_cam(rl, world, 32, spp=8)
        api.set_indep_cap(cam8.c.image_height * cam8.c.image_width * 3 * 8 * 3)  # 3 samples per pass: 3 passes
        cam8.render_independent(world)
        api.set_indep_cap(0)
        after_indep = api.live_buffers()
        assert after_indep[0] > after_coop[0] and after_indep[1] > after_coop[1]
        api.render_progress(world)  # the work counters move to pinned host memory (not device memory: the count stays)
        _render_device(rl, _spheres_cam(rl, world, 32), world)
        assert api.live_buffers() == after_indep
        # ray queries: 256 camera rays, their hits and their colours
        cam = _spheres_cam(rl, world, 32)
        px, py = np.arange(256, dtype=np.uint64) % 32, np.arange(256, dtype=np.uint64) // 32
        rays, cur = cam.get_rays(px, py, api.pack_cursors(px * np.uint64(32) + py))
        hits = world.hit_rays(rays["origin"], rays["dir"], rays["time"])
        assert hits.shape == (256,) and api.live_buffers() == after_indep  # the staging of rays and hits is gone again
        rgb, _, counts = world.ray_color_rays(None, None, None, cur, cam.c.seed, 8, world.params.background, rays=rays)
        assert rgb.shape == (256, 3) and counts.min() >= 1
        after_paths = api.live_buffers()  # (the scene may now hold the device copy of the parameter block the path kernel reads)
        assert after_paths >= after_indep
        world.ray_color_rays(None, None, None, cur, cam.c.seed, 8, world.params.background, rays=rays)
        assert api.live_buffers() == after_paths

        # a general scene: the fast general tree, and the device copy of the parameter block its kernel reads
        quads = rl.World.example_scene("quads")
        qcam = rl.Camera(dataclasses.replace(quads.params, aspect_ratio=1.0, image_width=48, samples_per_pixel=64))
        assert (qcam.c.image_width, qcam.c.image_height) == (48, 48)
        before = api.live_buffers()
        quads.device()
        created = api.live_buffers()
        assert created[0] > before[0]
        _render_device(rl, qcam, quads)
        assert api.live_buffers()[0] > created[0]
        qcam.render(quads, stats={})

        rw = rl.RtcWorld.test_obj_scene(golden("teapot-low.obj"), 60, 40)
        before = api.live_buffers()
        assert rw.render(1).shape == (40, 60, 3)
        assert api.live_buffers()[0] > before[0]
        assert rw.render_rgb8(1).shape == (40, 60, 3)
        o = np.tile(np.array([0.0, 1.0, -8.0]), (64, 1))
        d = np.stack([np.linspace(-0.3, 0.3, 64), np.zeros(64), np.ones(64)], axis=1)
        rw.intersect_rays(o, d, k=4)
        assert rw.color_at_rays(o, d).shape == (64, 3)

        assert api.live_buffers() > after_paths
        del world, quads, rw
    finally:
        api.set_coop(True)
        api.set_indep_cap(0)
    assert _baseline(rl) == base


@pytest.mark.parametrize("coop", [True, False])
def test_growth_keeps_results(rl, coop):
    """32x18, 96x54, 32x18 on ONE world (its work buffers grow, then are larger than the frame) = the same frames on fresh worlds.
    coop: the cooperative kernel's pixel list; not coop: the cost-sorted, stealing and pixel-entry buffers.  Both: the pass buffer."""
    api = rl.api
    base = _baseline(rl)
    try:
        api.set_coop(coop)

        def frames(world, width):
            cam = _spheres_cam(rl, world, width)
            return _render_device(rl, cam, world), cam.render_independent(world).data

        fresh = {width: frames(rl.World.bouncing_spheres(1), width) for width in (32, 96)}
        world = rl.World.bouncing_spheres(1)
        for width in (32, 96, 32):
            chained, indep = frames(world, width)
            assert np.array_equal(chained, fresh[width][0]), (coop, width)
            assert np.array_equal(indep, fresh[width][1]), (coop, width)
        del world
    finally:
        api.set_coop(True)
    assert _baseline(rl) == base


def test_counter_is_tied_to_real_memory(rl):
    """Eight worlds, each with a ~8 MB pass buffer, created and dropped: the driver's free memory after the eighth is the free memory
    after the first to within four pass buffers (eight leaked ones would be twice that).  No torch tensor is allocated in the loop."""
    import torch
    api = rl.api
    torch.cuda.mem_get_info(0)
    base = _baseline(rl)
    pass_bytes = 96 * 54 * 3 * 8 * 64
    free = []
    for cycle in range(8):
        world = rl.World.bouncing_spheres(1)
        _spheres_cam(rl, world, 96).render_independent(world)
        assert api.live_buffers()[1] >= base[1] + pass_bytes
        del world
        gc.collect()
        assert api.live_buffers() == base, cycle
        free.append(torch.cuda.mem_get_info(0)[0])
    print("free bytes after each cycle:", free)
    assert abs(free[0] - free[7]) < 4 * pass_bytes, free
