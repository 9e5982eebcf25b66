"""GPU tier: work stealing on small shards (csrc/rl_rtiow_wave.h STEAL instantiation, csrc/rl_rtiow_coop.h rtiow_steal_loop).  A shard
with about as many pixels as the GPU has lanes is bound by its longest per-pixel sample chains; waves whose lanes have run out of pixels
take pixels over from lanes that are still rendering — at a sample boundary, with the pixel's exact sums and ChaCha word position — and
continue them with all 64 lanes.  Which wave renders which sample must not change a single bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _frame(rl, cam, world, row_first=0, row_step=1):
    import torch
    dev = torch.device("cuda", 0)
    nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    buf = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, row_first=row_first, row_step=row_step)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


@pytest.mark.parametrize("width,spp,shard", [(640, 96, 1), (960, 64, 3), (1920, 72, 8)])
def test_work_stealing_renders_the_same_bits(rl, oracle, width, spp, shard):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = width, spp, 50
    cam = rl.Camera(p)
    npix = rl.api.rows_for(cam.c.image_height, 0, shard) * cam.c.image_width
    assert 40960 < npix <= 3 * 256 * 1024  # above the cooperative kernel's small-frame limit, within the stealing rule
    frames = []
    try:
        for fill in (3.0, 0.0, 3.0, 3.0):  # stealing on / off / on / on: the take-overs differ from run to run, the bits must not
            rl.api.set_steal(fill)
            frames.append(_frame(rl, cam, world, 0, shard))
    finally:
        rl.api.set_steal(3.0)
    ref, st_ref = frames[1]
    for img, st in frames:
        assert np.array_equal(img, ref) and st["rays"] == st_ref["rays"] and st["flagged"] == 0
    gs = {}
    counting = cam.render_rows(world, 0, shard, stats=gs)  # the reference-order counting kernel
    assert np.array_equal(ref, counting) and gs["rays"] == st_ref["rays"]
    ys = np.arange(0, cam.c.image_height, shard)[:: max(1, len(range(0, cam.c.image_height, shard)) // 6)].astype(np.uint32)
    gx, gy = np.meshgrid(np.arange(cam.c.image_width, dtype=np.uint32), ys)
    cpu = oracle.rtiow_render_pixels(world.desc, cam.c, gx.ravel(), gy.ravel()).reshape(len(ys), cam.c.image_width, 3)
    rows = (ys // shard).astype(int)
    assert np.abs(ref[rows] - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())


# ----------------------------------------------------------------------------- the protocol at its smallest shapes
# The cases above show that stealing changes no bit at the workload's own sizes; nothing in them shows that a pixel was ever taken over
# (were none, every assertion would still hold).  Here the hand-over itself is read back: the launch log (api.rtiow_launches) names the
# instantiation of each launch, and api.steal_record gives, per pixel, the final steal_state and the sample at which its lane released
# it.  With a few thousand pixels at most against CUs x 1024 lanes nearly every wave starts without work and asks at once, so a frame
# without a single hand-over means the protocol is broken, not that the scene was unlucky.
PLAIN, STEALING = "rtiow_wave_kernel<1024, 4, false, false>", "rtiow_wave_kernel<1024, 4, false, true>"
_small = {}


def _small_world(rl, name):
    """The 12-sphere world of test_gpu_launch_routes.py / the 40-sphere "built" world of test_gpu_wave_block_paths.py (a coincident pair:
    rays the fast walk re-traces in the reference's order, also inside the steal loop), each with its own camera placement."""
    if name not in _small:
        if name == "twelve":
            from test_gpu_launch_routes import _sphere_world
            _small[name] = (_sphere_world(rl), dict(vfov=50.0, lookfrom=(0.0, 1.8, 6.0), lookat=(0.0, 1.0, 0.0), defocus_angle=0.3, focus_dist=6.0, background=(0.6, 0.7, 0.9), seed=5))
        else:
            from test_gpu_wave_block_paths import _built_world
            world, p = _built_world(rl)
            _small[name] = (world, dict(vfov=p.vfov, lookfrom=p.lookfrom, lookat=p.lookat, defocus_angle=p.defocus_angle, focus_dist=p.focus_dist, background=p.background, seed=p.seed))
    return _small[name]


@pytest.fixture
def stealing_on_wave_kernels(rl):
    api = rl.api
    rl.init(0)
    api.set_coop(False), api.set_steal(3.0)
    yield api
    api.set_coop(True), api.set_steal(3.0)


SMALL = [(8, 8, 0, 1, 64, 6),     # one tile
         (13, 11, 0, 1, 65, 6),   # ragged tiles: candidates with x >= W or r >= nrows are passed over
         (24, 16, 1, 3, 64, 6),   # a row shard: virtual_index_pixel
         (64, 36, 0, 1, 72, 6)]


@pytest.mark.parametrize("w,h,row_first,row_step,spp,depth", SMALL + [(64, 36, 0, 1, 72, 50)], ids=lambda v: str(v))
@pytest.mark.parametrize("name", ["twelve", "built"])
def test_pixels_are_handed_over_and_finish_with_the_counting_bits(rl, stealing_on_wave_kernels, name, w, h, row_first, row_step, spp, depth):
    api = stealing_on_wave_kernels
    world, view = _small_world(rl, name)
    cam = rl.Camera(rl.CameraParams(aspect_ratio=w / (h + 0.5), image_width=w, samples_per_pixel=spp, max_depth=depth, **view))
    assert (cam.c.image_width, cam.c.image_height) == (w, h)
    npix = api.rows_for(h, row_first, row_step) * w
    gs = {}
    counting = cam.render_rows(world, row_first, row_step, stats=gs)  # the reference-order counting kernel
    assert gs["flagged"] == 0

    def render(fill):
        api.set_steal(fill)
        t0 = api.rtiow_launch_total()
        img, st = _frame(rl, cam, world, row_first, row_step)
        recs = api.rtiow_launches(t0)
        assert img.tobytes() == counting.tobytes() and st["rays"] == gs["rays"] and st["flagged"] == 0
        assert [(r["sample_begin"], r["sample_end"], r["resume"], r["tile_order"]) for r in recs] == [(0, 8, 0, False), (8, spp, 1, True)]
        return recs, st

    handed_over = []
    for _ in range(3):  # which wave takes which pixel differs from run to run; what is asserted must hold in each
        recs, st = render(3.0)
        assert [r["kernel"] for r in recs] == [PLAIN, STEALING] and [r["steal_state"] for r in recs] == [False, True]
        state, n = api.steal_record(world, npix)
        assert (state == 3).all(), np.unique(state, return_counts=True)  # every pixel of the shard finished, wherever
        handed = n != api.NEVER_OFFERED
        assert ((n[handed] >= 8) & (n[handed] < spp)).all(), n[handed]  # released at a sample boundary of the resumed launch, before the last
        handed_over.append(int(handed.sum()))
        if name == "built" and (w, h) == (64, 36):
            assert st["slow_traces"] > 0  # the coincident pair
    print(f"{name} {w} x {h} rows {row_first}::{row_step} spp {spp} depth {depth}: {npix} pixels, handed over {handed_over}, slow traces {st['slow_traces']}")
    assert min(handed_over) >= 1, handed_over

    # stealing off: the plain instantiation twice, and the record stays as the last stealing launch left it
    recs, _ = render(0.0)
    assert [r["kernel"] for r in recs] == [PLAIN, PLAIN] and not any(r["steal_state"] for r in recs)
    state_after, n_after = api.steal_record(world, npix)
    assert np.array_equal(state_after, state) and np.array_equal(n_after, n)
