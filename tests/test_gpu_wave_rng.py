"""GPU tier: the wave-cooperative ChaCha8 block generation of the wave-scheduled sphere kernel (csrc/rl_rtiow_wave.h
Ring::coop_blocks, RL_COOP_GEN).  A GEN block generates the two blocks of every stream reset one block per lane, each into the
requesting lane's ring column (two passes when more than 32 lanes start a sample).  Every ray must still draw the same words: the
timed frames equal the counting kernel's bit for bit, and both equal the oracle (counters, rows)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "rng_words", "flagged")


def _timed(rl, cam, world, row_first=0, row_step=1):
    import torch
    dev = torch.device("cuda", 0)
    nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    buf = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, row_first=row_first, row_step=row_step)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


def _check(rl, oracle, world, p, full_oracle):
    cam = rl.Camera(p)
    try:
        rl.api.set_coop(False)  # small frames: the wave-scheduled kernel, not the cooperative one-wave-per-pixel kernel
        rl.api.set_rtiow_variant(1029)  # the fast traversal rtiow_wave_kernel<1024, 4, false> (what bench.py times)
        timed, st = _timed(rl, cam, world)
    finally:
        rl.api.set_rtiow_variant(0)
        rl.api.set_coop(True)
    gs = {}
    counting = cam.render(world, stats=gs).data
    assert np.array_equal(timed, counting) and st["rays"] == gs["rays"]
    if full_oracle:
        cs = {}
        cpu = oracle.rtiow_render(world.desc, cam.c, stats=cs)
        for k in COUNTERS:
            assert gs[k] == cs[k], (k, gs[k], cs[k])
    else:
        ys = np.arange(0, cam.c.image_height, max(1, cam.c.image_height // 4)).astype(np.uint32)
        gx, gy = np.meshgrid(np.arange(cam.c.image_width, dtype=np.uint32), ys)
        cpu = oracle.rtiow_render_pixels(world.desc, cam.c, gx.ravel(), gy.ravel()).reshape(len(ys), cam.c.image_width, 3)
        timed = timed[ys.astype(int)]
    assert np.abs(timed - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())
    return gs


def test_launch_start_two_passes(rl, oracle):
    """Every lane starts in GEN: 128 blocks per wave, the two-pass path."""
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 128, 6, 50
    _check(rl, oracle, world, p, full_oracle=True)


def test_specular_world_at_depth_50(rl, oracle):
    """Metal and glass everywhere at depth 50: long paths, many FILL top-ups between the stream resets."""

    def build(b):
        items = [b.sphere((0, -1000, 0), 1000, b.metal((0.7, 0.7, 0.75), 0.0))]
        for i in range(-4, 5):
            for k in range(-4, 5):
                m = b.dielectric(1.5) if (i + k) % 2 else b.metal((0.8, 0.6, 0.5), 0.05 * ((i * 7 + k) % 4))
                items.append(b.sphere((1.1 * i, 0.45, 1.1 * k), 0.45, m))
        items.append(b.sphere((0, 2.0, 0), 1.5, b.dielectric(1.33)))
        return b.bvh(items)

    world = rl.World.build(build)
    p = rl.CameraParams(aspect_ratio=1.5, image_width=96, samples_per_pixel=8, max_depth=50, vfov=35.0, lookfrom=(9, 4, 7), lookat=(0, 0.5, 0),
                        background=(0.7, 0.8, 1.0), seed=3)
    gs = _check(rl, oracle, world, p, full_oracle=True)
    assert gs["rays"] > 2 * 96 * 64 * 8  # paths of several bounces: the FILL path is exercised


def test_lpt_resume_launch(rl, oracle):
    """spp >= 64: the cost-sorted second launch resumes every pixel at its saved ChaCha word position."""
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 128, 72, 50
    _check(rl, oracle, world, p, full_oracle=False)


def test_stealing_shard(rl, oracle):
    """The work-stealing instantiation rtiow_wave_kernel<1024, 4, false, true> on a 1/3 shard, against the counting kernel's rows."""
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 960, 64, 50
    cam = rl.Camera(p)
    shard = 3
    try:
        rl.api.set_steal(3.0)
        img, st = _timed(rl, cam, world, 0, shard)
    finally:
        rl.api.set_steal(3.0)
    gs = {}
    counting = cam.render_rows(world, 0, shard, stats=gs)
    assert np.array_equal(img, counting) and gs["rays"] == st["rays"] and st["flagged"] == 0
    ys = np.arange(0, cam.c.image_height, shard)[::40].astype(np.uint32)
    gx, gy = np.meshgrid(np.arange(cam.c.image_width, dtype=np.uint32), ys)
    cpu = oracle.rtiow_render_pixels(world.desc, cam.c, gx.ravel(), gy.ravel()).reshape(len(ys), cam.c.image_width, 3)
    assert np.abs(img[(ys // shard).astype(int)] - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())
