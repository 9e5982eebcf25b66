"""GPU tier: the pass plan of the wave kernels' cooperative ChaCha8 block generation (csrc/rl_rtiow_wave.h Ring::coop_blocks): full
passes of 64 jobs with a lane per block, and a remainder of at most 32 jobs in quad passes of 16 jobs with four lanes per block
(csrc/rl_rtiow_kernel.h chacha8_quad_block_to_lds_job); FILL generates through the same plan.  Every block must land, word for word,
in the ring slots the lane-per-block form writes.  The counting kernel shares Ring, so the independent side is the CPU oracle:
the timed frame equals the counting frame bit for bit, the counters equal the oracle's, the pixels are the oracle's within
1e-9 * max(1, |cpu|) (the pattern of tests/test_gpu_wave_rng.py::_check with full_oracle=True).

A wave claims one 8x8 tile, so the frame size sets the number of lanes that start a sample at launch start (two blocks each):
    3x2   6 requesters   J = 12: one quad pass              8x6  48 requesters  J = 96: one full pass, two quad passes
    5x4  20 requesters   J = 40 > 32: one full pass         8x7  56 requesters  J = 112: two full passes
    8x5  40 requesters   J = 80: one full, one quad pass    8x8  64 requesters  J = 128: two full passes
and 24x16 is six waves in one workgroup with every shape mixed.  The specular world's long paths give FILL passes of 1-16, 17-32 and
more lanes at 3x2, 8x3 and 8x6."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ("rays", "node_tests", "sphere_tests", "rng_words", "flagged")


def _sized(p, width, height):
    """The camera parameters for a width x height frame: image_height = floor(image_width / aspect_ratio)."""
    p.image_width, p.aspect_ratio = width, width / (height + 0.5)
    return p


def _timed(rl, cam, world):
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.full((cam.c.image_height, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


def _check(rl, oracle, world, p, size):
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == size
    try:
        rl.api.set_coop(False)  # small frames: the wave-scheduled kernel, not the cooperative one-wave-per-pixel kernel
        rl.api.set_rtiow_variant(1029)  # the fast traversal rtiow_wave_kernel<1024, 4, false> (what bench.py times)
        timed, st = _timed(rl, cam, world)
    finally:
        rl.api.set_rtiow_variant(0)
        rl.api.set_coop(True)
    gs, cs = {}, {}
    counting = cam.render(world, stats=gs).data
    assert np.array_equal(timed, counting) and st["rays"] == gs["rays"]
    cpu = oracle.rtiow_render(world.desc, cam.c, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    assert np.abs(timed - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())
    return gs


def _specular_world(rl):
    """The world of tests/test_gpu_wave_rng.py::test_specular_world_at_depth_50: metal and glass everywhere."""

    def build(b):
        items = [b.sphere((0, -1000, 0), 1000, b.metal((0.7, 0.7, 0.75), 0.0))]
        for i in range(-4, 5):
            for k in range(-4, 5):
                m = b.dielectric(1.5) if (i + k) % 2 else b.metal((0.8, 0.6, 0.5), 0.05 * ((i * 7 + k) % 4))
                items.append(b.sphere((1.1 * i, 0.45, 1.1 * k), 0.45, m))
        items.append(b.sphere((0, 2.0, 0), 1.5, b.dielectric(1.33)))
        return b.bvh(items)

    return rl.World.build(build)


@pytest.mark.parametrize("size", [(3, 2), (5, 4), (8, 5), (8, 6), (8, 7), (8, 8), (24, 16)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_pass_shape_of_the_first_gen(rl, oracle, size):
    world = rl.World.bouncing_spheres(1)
    p = _sized(world.params, *size)
    p.samples_per_pixel, p.max_depth = 8, 10
    _check(rl, oracle, world, p, size)


@pytest.mark.parametrize("size", [(3, 2), (8, 3), (8, 6)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_fill_passes_of_the_specular_world_at_depth_50(rl, oracle, size):
    world = _specular_world(rl)
    p = _sized(rl.CameraParams(image_width=size[0], samples_per_pixel=8, max_depth=50, vfov=35.0, lookfrom=(9, 4, 7), lookat=(0, 0.5, 0),
                               background=(0.7, 0.8, 1.0), seed=3), *size)
    gs = _check(rl, oracle, world, p, size)
    assert gs["rays"] > 2 * size[0] * size[1] * 8  # paths of several bounces: the FILL path is exercised


def test_resume_launch_at_72_spp(rl, oracle):
    """spp >= 64: the cost-sorted second launch resumes every pixel at its saved word position, so the first GEN of that launch has
    non-zero positions: both ring halves, odd blk_lo."""
    world = rl.World.bouncing_spheres(1)
    p = _sized(world.params, 8, 6)
    p.samples_per_pixel, p.max_depth = 72, 10
    _check(rl, oracle, world, p, (8, 6))


def _oracle_samples(rl, oracle, world, p, F, S):
    """The oracle's single-sample frames of samples F .. F + S - 1, and their summed counters."""
    c1 = rl.Camera(dataclasses.replace(p, samples_per_pixel=1)).c
    frames, tot = [], dict.fromkeys(COUNTERS, 0)
    for s in range(F, F + S):
        cs = {}
        frames.append(oracle.rtiow_render(world.desc, c1, first_sample=s, stats=cs))
        for k in COUNTERS:
            tot[k] += cs[k]
    return frames, tot


def test_moments_render(rl, oracle):
    """rtiow_wave_moments_kernel at 8x6: the sums are the counting render's bytes, with the oracle's counters and pixels; the second
    moments are, bit for bit, those of the cooperative one-wave-per-pixel kernel, which generates its blocks itself, without Ring."""
    import torch
    world = rl.World.bouncing_spheres(1)
    p = _sized(world.params, 8, 6)
    p.samples_per_pixel, p.max_depth = 8, 10
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (8, 6)
    dev = torch.device("cuda", 0)

    def moments():
        d_s = torch.full((6, 8, 3), float("nan"), dtype=torch.float64, device=dev)
        d_q = torch.full((6, 8, 3), float("nan"), dtype=torch.float64, device=dev)
        cam.render_moments_device(world, d_s.data_ptr(), d_q.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        st = rl.api.render_status(world)
        return d_s.cpu().numpy(), d_q.cpu().numpy(), st

    try:
        rl.api.set_coop(False)
        sums, sq, st = moments()
    finally:
        rl.api.set_coop(True)
    csums, csq, _ = moments()  # the cooperative kernel
    gs, cs = {}, {}
    counting = cam.render(world, stats=gs).data
    assert sums.tobytes() == counting.tobytes() and st["rays"] == gs["rays"]
    assert not np.isnan(sq).any() and sums.tobytes() == csums.tobytes() and sq.tobytes() == csq.tobytes()
    cpu = oracle.rtiow_render(world.desc, cam.c, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    assert np.abs(sums - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())


def test_independent_sample_render(rl, oracle):
    """rtiow_wave_indep_kernel at 8x6: every sample from word 0 of its own stream.  Counter-free frame = counting frame, counters = the
    oracle's single-sample renders summed, pixels = their left-to-right sum within the tolerance."""
    import torch
    world = rl.World.bouncing_spheres(1)
    F, S = 2, 8
    p = _sized(world.params, 8, 6)
    p.samples_per_pixel, p.max_depth = S, 10
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (8, 6)
    buf = torch.zeros((6, 8, 3), dtype=torch.float64, device="cuda:0")
    try:
        rl.api.set_coop(False)
        cam.render_independent_device(world, buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, first_sample=F)
        st = rl.api.render_status(world)
    finally:
        rl.api.set_coop(True)
    fast = buf.cpu().numpy()
    gs = {}
    counted = cam.render_independent_rows(world, 0, 1, first_sample=F, stats=gs)
    assert np.array_equal(fast, counted) and st["rays"] == gs["rays"]
    frames, tot = _oracle_samples(rl, oracle, world, p, F, S)
    for k in COUNTERS:
        assert gs[k] == tot[k], (k, gs[k], tot[k])
    cpu = np.zeros_like(frames[0])
    for f in frames:
        cpu = cpu + f
    assert np.abs(fast - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())


CHILD = r'''
import importlib, sys
import numpy as np
import torch  # before the product library: one HIP runtime per process
sys.path.insert(0, %(root)r)
rl = importlib.import_module("rendering-learning_amd")
rl.api.init(0)
world = rl.World.bouncing_spheres(1)
p = world.params
p.image_width, p.aspect_ratio, p.samples_per_pixel, p.max_depth = 8, 8 / 6.5, 8, 10
cam = rl.Camera(p)
assert (cam.c.image_width, cam.c.image_height) == (8, 6)
rl.api.set_coop(False)
rl.api.set_rtiow_variant(1029)
buf = torch.full((6, 8, 3), float("nan"), dtype=torch.float64, device="cuda:0")
cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
st = rl.api.render_status(world)
sys.stdout.write("FRAME %%d %%s\n" %% (st["rays"], buf.cpu().numpy().tobytes().hex()))
'''


def test_switch_restores_lane_per_block_passes(rl):
    """RL_COOP_QUAD=0 in a fresh process (the switch is read once, at initialisation): the same frame bytes and ray count."""
    world = rl.World.bouncing_spheres(1)
    p = _sized(world.params, 8, 6)
    p.samples_per_pixel, p.max_depth = 8, 10
    cam = rl.Camera(p)
    try:
        rl.api.set_coop(False)
        rl.api.set_rtiow_variant(1029)
        here, st = _timed(rl, cam, world)
    finally:
        rl.api.set_rtiow_variant(0)
        rl.api.set_coop(True)
    env = dict(os.environ, RL_COOP_QUAD="0")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout
    line = next(ln for ln in r.stdout.splitlines() if ln.startswith("FRAME "))
    _, rays, hexbytes = line.split()
    assert int(rays) == st["rays"] and bytes.fromhex(hexbytes) == here.tobytes()
