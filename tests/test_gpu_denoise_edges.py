"""GPU tier: the a-trous denoiser (include/rl_render.h "Denoising") where tests/test_gpu_denoise.py does not reach: a
workgroup that takes a second and later tile (forced by api.set_denoise_blocks, and in the shipped launch on an image with more tiles than
the grid's cap), odd steps and steps beyond the image, the largest step and the host form's twelve iterations, magnitudes far from 1,
containment of non-finite inputs, the smallest variance_floor, and denoise_render of an adaptive render.  The yardstick is
tests/atrous_model.py (held to the exact operation by tests/test_atrous_model_exact.py); outputs are compared as bytes, no tolerance."""
import dataclasses

import numpy as np
import pytest

import atrous_model as M
import test_gpu_denoise as T

pytestmark = pytest.mark.gpu
FORCED = (0, 1)  # images, LDS
DBL_MIN = float(np.finfo(np.float64).tiny)


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    rl.api.set_denoise_blocks(0)
    yield
    rl.api.set_denoise_route(-1)
    rl.api.set_denoise_blocks(0)


def _tiles(W, H, step, lds):
    """The tiling as the design states it: 32 x 8 tiles of adjacent pixels (images), or of each non-empty lattice of the step (LDS)."""
    s = step if lds else 1
    return min(s, W) * min(s, H) * (-(-(-(-W // s)) // 32)) * (-(-(-(-H // s)) // 8))


def _params(rl, G, floor=1e-8, seed=5):
    inv = list(np.random.default_rng(seed).uniform(0.25, 4.0, G))
    return rl.api.atrous_params(G, color_sigma=2.0, guide_inv_sigma=inv, variance_floor=floor)


def _check_routes(rl, frame, p, step, want, max_blocks=(0,), routes=FORCED):
    """One pass on each forced route and each workgroup cap against the model's (colour, variance); the launch is what the hooks report."""
    api = rl.api
    H, W = frame[0].shape[:2]
    try:
        for route in routes:
            api.set_denoise_route(route)
            tiles = _tiles(W, H, step, route == 1)
            for mb in max_blocks:
                api.set_denoise_blocks(mb)
                got_c, got_v = T._device_passes(rl, frame, p, [step])
                launch = api.last_denoise_launch()
                assert api.last_denoise_route() == ("images", "lds")[route]
                assert launch["tiles"] == tiles, (route, mb, launch)
                if mb:
                    assert launch["blocks"] == min(mb, tiles) and launch["tiles"] > launch["blocks"], (route, mb, launch)
                assert T._same(got_c, want[0]), (route, mb, int((got_c != want[0]).sum()))
                assert T._same(got_v, want[1]), (route, mb, int((got_v != want[1]).sum()))
    finally:
        api.set_denoise_route(-1)
        api.set_denoise_blocks(0)


@pytest.mark.parametrize("G", [0, 8])
@pytest.mark.parametrize("step", [1, 3, 16])
@pytest.mark.parametrize("shape", [(23, 37), (45, 70)], ids=["37x23", "70x45"])
def test_a_few_workgroups_walk_every_tile(rl, shape, step, G):
    """1, 2 and 5 workgroups for 6 - 256 (37 x 23) and 18 - 256 (70 x 45) tiles: every workgroup takes several tiles in turn, on the LDS
    route staging each over the last one's points.  The outputs start as NaN, so a tile that nobody took shows."""
    frame = T._frame(*shape, G)
    p = _params(rl, G)
    want = M.atrous_pass(*frame, *M.params_of(p), step)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    _check_routes(rl, frame, p, step, want, max_blocks=(1, 2, 5))


def test_the_shipped_launch_with_more_tiles_than_workgroups(rl):
    """No cap set: a 3-wide image of 8 * (8 * CUs + 3) rows has 8 * CUs + 3 tiles at step 1 on either route and twice that at step 2 on the
    LDS route; 8 workgroups per CU is the largest grid any route launches, so the tile loop's later trips run as shipped."""
    import torch
    api = rl.api
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    W, H, G = 3, 8 * (8 * cus + 3), 2
    frame = T._frame(H, W, G, seed=31)
    p = _params(rl, G)
    api.set_denoise_blocks(0)
    try:
        for step, routes in ((1, (0, 1)), (2, (1,))):
            want_c, want_v = M.atrous_pass(*frame, *M.params_of(p), step)
            for route in routes:
                api.set_denoise_route(route)
                got_c, got_v = T._device_passes(rl, frame, p, [step])
                launch = api.last_denoise_launch()
                print(f"{W} x {H} step {step} route {api.last_denoise_route()}: {launch}")
                assert launch["tiles"] == _tiles(W, H, step, route == 1) and 0 < launch["blocks"] < launch["tiles"], launch
                assert launch["blocks"] <= 8 * cus
                assert T._same(got_c, want_c) and T._same(got_v, want_v), (step, route)
    finally:
        api.set_denoise_route(-1)


@pytest.mark.parametrize("G", [0, 3])
@pytest.mark.parametrize("step", [3, 5, 7, 64, 1 << 20])
@pytest.mark.parametrize("shape", [(23, 37), (9, 33)], ids=["37x23", "33x9"])
def test_odd_steps_and_steps_beyond_the_image(rl, shape, step, G):
    """Odd steps: lattices of unequal sizes aligned to nothing.  64 and 1 << 20 reach past both edges of both shapes from every pixel: only
    the centre tap is inside.  33 x 9 leaves one pixel column and one pixel row to a second tile."""
    frame = T._frame(*shape, G)
    p = _params(rl, G)
    want = M.atrous_pass(*frame, *M.params_of(p), step)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    _check_routes(rl, frame, p, step, want)


def test_the_host_form_at_twelve_iterations(rl):
    frame = T._frame(23, 37, 3)
    p = _params(rl, 3)
    want_c, want_v = M.atrous(*frame, *M.params_of(p), 12)
    got_c, got_v = rl.api.denoise_atrous(*frame, iterations=12, params=p)
    assert np.isfinite(want_c).all() and np.isfinite(want_v).all()
    assert T._same(got_c, want_c) and T._same(got_v, want_v)


def _huge_frame():
    """Colours about 1e140 (one region exactly flat, so that d2 = 0 there and the weights are tiny / tiny), variances about 1e-300."""
    _, mean, variance, guides = M.four_region_image(23, 37, 4, 41, n_guides=2)
    rng = np.random.default_rng(43)
    color = np.ascontiguousarray(mean * 1e140)
    color[:, :8] = rng.standard_normal((23, 8, 3)) * 1e140
    return color, np.ascontiguousarray(rng.random((23, 37, 3)) * 1e-300), guides


def _subnormal_frame():
    """Colours O(1) but for the top left 10 x 12 block, whose colours are small multiples of 2^-1074: their differences and squares are
    subnormal or underflow; every variance is subnormal (a block of exact zeros stays), so D is a few DBL_MIN and (h*h) * D is subnormal."""
    _, mean, variance, guides = M.four_region_image(23, 37, 4, 47, n_guides=2)
    rng = np.random.default_rng(53)
    color = mean.copy()
    color[:10, :12] = rng.integers(0, 1 << 20, (10, 12, 3)) * 5e-324
    tiny = rng.integers(0, 1 << 30, (23, 37, 3)) * 5e-324
    tiny[12:16, 20:30] = 0.0
    assert tiny.max() < DBL_MIN
    return np.ascontiguousarray(color), np.ascontiguousarray(tiny), guides


@pytest.mark.parametrize("step", [1, 2])
@pytest.mark.parametrize("which", ["huge", "subnormal"])
def test_magnitudes_far_from_one(rl, which, step):
    """The model's bytes rest on correctly rounded binary64 division and multiplication over the whole range, not only near 1."""
    frame, floor = (_huge_frame(), 1e-305) if which == "huge" else (_subnormal_frame(), DBL_MIN)
    p = _params(rl, 2, floor=floor)
    want = M.atrous_pass(*frame, *M.params_of(p), step)
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    assert not T._same(want[0], frame[0])  # the pass did something at these magnitudes
    _check_routes(rl, frame, p, step, want)


@pytest.mark.parametrize("step", [1, 3])
def test_non_finite_inputs_stay_in_their_footprint(rl, step):
    """A NaN colour in the interior, a +inf variance in a corner and a NaN guide in column 32 (the first of the second tile, a halo point of
    the first): non-finite outputs, in every channel of both images, exactly in the pixels one of whose 25 taps is such a pixel; every other
    pixel has the model's bytes."""
    H, W = 23, 70
    color, variance, guides = T._frame(H, W, 2)
    color[11, 20, 1] = np.nan
    variance[0, 0, 0] = np.inf
    guides[5, 32, 1] = np.nan
    frame = (color, variance, guides)
    expected = np.zeros((H, W), dtype=bool)
    for qy, qx in ((11, 20), (0, 0), (5, 32)):
        for j in range(-2, 3):
            for i in range(-2, 3):
                py, px = qy + j * step, qx + i * step
                if 0 <= py < H and 0 <= px < W:
                    expected[py, px] = True
    assert expected[0, 0] and expected[5, 32 - step] and expected[5, 32] and not expected[20, 60]
    p = _params(rl, 2)
    want_c, want_v = M.atrous_pass(*frame, *M.params_of(p), step)
    api = rl.api
    try:
        for route in FORCED:
            api.set_denoise_route(route)
            got_c, got_v = T._device_passes(rl, frame, p, [step])
            for got, want in ((got_c, want_c), (got_v, want_v)):
                bad = ~np.isfinite(got)
                assert (bad.any(axis=-1) == bad.all(axis=-1)).all()
                assert (bad.all(axis=-1) == expected).all(), route
                assert ((~np.isfinite(want)).all(axis=-1) == expected).all()
                assert got[~expected].tobytes() == want[~expected].tobytes(), route
    finally:
        api.set_denoise_route(-1)


@pytest.mark.parametrize("G", [0, 2])
@pytest.mark.parametrize("step", [1, 16])
def test_the_smallest_variance_floor_on_a_flat_image(rl, step, G):
    """variance_floor = DBL_MIN, the least the library takes, on a flat image without variance: D is the floor in every tap and every
    (h*h) * D is a subnormal.  Finite, and the model's bytes (a subnormal floor would give 0 / 0: tests/test_denoise_abi.py)."""
    H, W = 23, 37
    _, _, guides = T._frame(H, W, G)
    frame = (np.broadcast_to(np.array([0.3, 0.7, 1.1]), (H, W, 3)).copy(), np.zeros((H, W, 3)), guides)
    p = _params(rl, G, floor=DBL_MIN)
    want = M.atrous_pass(*frame, *M.params_of(p), step)
    assert np.isfinite(want[0]).all() and not want[1].any()
    _check_routes(rl, frame, p, step, want)


def test_denoise_render_of_an_adaptive_render(rl):
    """render_adaptive (up to 16 samples, checkpoints at 4, 8, 12, variance of the mean <= 2e-3) and render_features through denoise_render:
    finite, and the bytes of the model on the same inputs.  The error against a 1024-spp render is printed, not asserted: the adaptive
    case has not been measured before."""
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    p = dataclasses.replace(world.params, image_width=64, aspect_ratio=64 / 48.5, samples_per_pixel=16)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (64, 48)
    adaptive, features = cam.render_adaptive(world, 4, 4, abs_variance=2e-3), cam.render_features(world)
    values, counts = np.unique(adaptive.counts, return_counts=True)
    print(f"adaptive counts: {dict(zip(values.tolist(), counts.tolist()))}")
    assert len(values) >= 2 and adaptive.counts.min() >= 2
    color, variance = api.denoise_render(adaptive, features)
    assert np.isfinite(color).all() and np.isfinite(variance).all()
    cin, vin, guides, sigmas, a = api._denoise_render_inputs(adaptive, features, None, api.GUIDE_KINDS)
    prm = api.atrous_params(guides.shape[2], guide_sigma=sigmas)
    want_c, want_v = M.atrous(cin, vin, guides, *M.params_of(prm), 5)
    assert T._same(want_c * a, color) and T._same(want_v * (a * a), variance)
    truth = rl.Camera(dataclasses.replace(p, samples_per_pixel=1024)).render(world).pixel_data()
    before, after = M.mse(adaptive.mean(), truth), M.mse(color, truth)
    print(f"bouncing_spheres 64x48 adaptive, {adaptive.counts.mean():.2f} spp on average: mse noisy {before:.4e}, denoised {after:.4e}, ratio {after / before:.3f}")
