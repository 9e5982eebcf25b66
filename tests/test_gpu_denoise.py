"""GPU tier: the a-trous denoiser (rl_denoise_atrous_pass_device, rl_denoise_atrous; include/rl_render.h "Denoising").
The yardstick is tests/atrous_model.py, the header's statement in numpy.  No tolerance anywhere: outputs are compared as bytes, on both
routes of the kernel (taps from the images / from one lattice's tile and halo staged in LDS)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import atrous_model as M

pytestmark = pytest.mark.gpu
ROUTES = (-1, 0, 1)  # default, images, LDS


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_denoise_route(-1)
    rl.api.set_denoise_blocks(0)


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _frame(H, W, G, seed=11):
    """(color, variance, guides or None): seeded noise on the four-region pattern; one region's variances are exactly 0."""
    _, mean, variance, guides = M.four_region_image(H, W, 4, seed, n_guides=G)
    return mean, variance, guides


def _params(rl, G, seed=5, color_sigma=2.0):
    inv = list(np.random.default_rng(seed).uniform(0.25, 4.0, G))
    return rl.api.atrous_params(G, color_sigma=color_sigma, guide_inv_sigma=inv, variance_floor=1e-8)


def _device_passes(rl, frame, p, steps, stream=None, want_variance=True):
    """The device form's ping-pong loop over torch buffers on `stream` (default: a fresh non-default one) -> (color, variance) on the host."""
    import torch
    color, variance, guides = frame
    H, W = color.shape[:2]
    dev = "cuda:0"
    src = [torch.from_numpy(color).to(dev), torch.from_numpy(variance).to(dev)]
    dg = torch.from_numpy(guides).to(dev) if guides is not None else None
    work = [[torch.full_like(src[0], float("nan")), torch.full_like(src[0], float("nan"))] for _ in range(2)]
    torch.cuda.synchronize()
    s = stream if stream is not None else torch.cuda.Stream()
    for n, step in enumerate(steps):
        dst = work[n & 1]
        last = n + 1 == len(steps)
        rl.api.denoise_atrous_pass_device(W, H, step, p, src[0].data_ptr(), src[1].data_ptr(), dg.data_ptr() if dg is not None else 0, dst[0].data_ptr(),
                                          dst[1].data_ptr() if want_variance or not last else 0, stream=s.cuda_stream)
        src = dst
    s.synchronize()
    return src[0].cpu().numpy(), src[1].cpu().numpy()


@pytest.mark.parametrize("G", [0, 1, 8])
@pytest.mark.parametrize("step", [1, 2, 4, 16])
@pytest.mark.parametrize("shape", [(23, 37), (16, 16), (8, 32)], ids=["37x23", "16x16", "32x8"])
def test_one_pass_gives_the_model_bytes_on_every_route(rl, shape, step, G):
    """37 x 23 is a multiple of neither tile edge and takes several workgroups; 32 x 8 is exactly one tile; step 16 puts most taps outside
    and, on the LDS route, leaves a handful of pixels to each of its 16 x 16 lattices."""
    api = rl.api
    frame = _frame(*shape, G)
    p = _params(rl, G)
    want_c, want_v = M.atrous_pass(*frame, *M.params_of(p), step)
    assert np.isfinite(want_c).all() and np.isfinite(want_v).all()
    try:
        for route in ROUTES:
            api.set_denoise_route(route)
            got_c, got_v = _device_passes(rl, frame, p, [step])
            if route >= 0:
                assert api.last_denoise_route() == ("images", "lds")[route]
            assert _same(got_c, want_c), (route, float(np.abs(got_c - want_c).max()))
            assert _same(got_v, want_v), (route, float(np.abs(got_v - want_v).max()))
    finally:
        api.set_denoise_route(-1)


@pytest.mark.parametrize("shape", [(1, 1), (40, 1), (1, 40), (3, 2)], ids=["1x1", "1x40", "40x1", "2x3"])
@pytest.mark.parametrize("step", [1, 16])
def test_degenerate_shapes(rl, shape, step):
    api = rl.api
    frame = _frame(*shape, 2)
    p = _params(rl, 2)
    want_c, want_v = M.atrous_pass(*frame, *M.params_of(p), step)
    try:
        for route in ROUTES:
            api.set_denoise_route(route)
            got_c, got_v = _device_passes(rl, frame, p, [step])
            assert np.isfinite(got_c).all() and np.isfinite(got_v).all()
            assert _same(got_c, want_c) and _same(got_v, want_v), route
    finally:
        api.set_denoise_route(-1)


@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_host_form_is_the_model_iterated_and_the_device_loop(rl, iterations):
    api = rl.api
    frame = _frame(23, 37, 3)
    p = _params(rl, 3)
    want_c, want_v = M.atrous(*frame, *M.params_of(p), iterations)
    got_c, got_v = api.denoise_atrous(*frame, iterations=iterations, params=p)
    assert _same(got_c, want_c) and _same(got_v, want_v)
    only_c, none = api.denoise_atrous(*frame, iterations=iterations, params=p, out_variance=False)
    assert none is None and _same(only_c, got_c)
    if iterations:
        steps = [1 << it for it in range(iterations)]
        dev_c, dev_v = _device_passes(rl, frame, p, steps)
        assert _same(dev_c, got_c) and _same(dev_v, got_v)
        dev_c, _ = _device_passes(rl, frame, p, steps, want_variance=False)  # the last pass without a variance output
        assert _same(dev_c, got_c)
    # the C++ mirror's wrapper
    Hl = api.host_lib()
    Hl.rlh_denoise_atrous_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(api.AtrousParams)] + [C.c_void_p] * 5
    mc, mv = np.empty_like(got_c), np.empty_like(got_v)
    assert Hl.rlh_denoise_atrous_probe(37, 23, iterations, C.byref(p), *(a.ctypes.data for a in frame), mc.ctypes.data, mv.ctypes.data) == 0
    assert _same(mc, got_c) and _same(mv, got_v)


def test_host_form_releases_its_staging(rl):
    api = rl.api
    before = api.live_buffers()
    api.denoise_atrous(*_frame(23, 37, 2), iterations=3, params=_params(rl, 2))
    assert api.live_buffers() == before


def test_a_guide_switched_off_is_the_call_without_that_channel(rl):
    api = rl.api
    color, variance, guides = _frame(23, 37, 3)
    inv = [1.5, 0.0, 0.75]
    on = api.denoise_atrous(color, variance, guides, iterations=3, guide_inv_sigma=inv)
    off = api.denoise_atrous(color, variance, np.ascontiguousarray(guides[..., [0, 2]]), iterations=3, guide_inv_sigma=[inv[0], inv[2]])
    assert _same(on[0], off[0]) and _same(on[1], off[1])
    other = api.denoise_atrous(color, variance, guides, iterations=3, guide_inv_sigma=[1.5, 0.5, 0.75])
    assert not _same(other[0], on[0])  # the channel does matter when it is on


def test_a_hard_edge_in_a_guide_stops_the_leak(rl):
    """Two flat halves whose colours differ, no noise but a large stated variance, so that the colour term stops nothing; the guide is the
    half's index.  With guide_inv_sigma = 1e6 the pixels beside the edge stay closer to their own half's colour than with the guide off."""
    api = rl.api
    H, W = 12, 40
    right = np.arange(W)[None, :].repeat(H, 0) >= W // 2
    truth = np.where(right[..., None], np.array([0.2, 0.9, 0.4]), np.array([1.0, 0.1, 0.3]))
    variance = np.ones((H, W, 3))
    guides = np.ascontiguousarray(right.astype(np.float64)[..., None])
    on, _ = api.denoise_atrous(truth, variance, guides, iterations=3, color_sigma=2.0, guide_inv_sigma=[1e6])
    off, _ = api.denoise_atrous(truth, variance, guides, iterations=3, color_sigma=2.0, guide_inv_sigma=[0.0])
    band = slice(W // 2 - 3, W // 2 + 3)
    leak_on, leak_off = M.mse(on[:, band], truth[:, band]), M.mse(off[:, band], truth[:, band])
    print(f"leak across the edge: guide on {leak_on:.3e}, guide off {leak_off:.3e}")
    assert leak_on < leak_off


def test_two_frames_on_two_streams_give_their_single_stream_bytes(rl):
    import torch
    api = rl.api
    frames = [_frame(70, 96, 2, seed=21), _frame(45, 130, 2, seed=22)]
    ps = [_params(rl, 2, seed=7), _params(rl, 2, seed=8, color_sigma=1.0)]
    steps = [1, 2, 4]
    alone = [api.denoise_atrous(*f, iterations=len(steps), params=p) for f, p in zip(frames, ps)]
    dev = "cuda:0"
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    bufs = []
    for color, variance, guides in frames:
        src = [torch.from_numpy(color).to(dev), torch.from_numpy(variance).to(dev)]
        bufs.append({"src": src, "g": torch.from_numpy(guides).to(dev), "work": [[torch.empty_like(src[0]), torch.empty_like(src[0])] for _ in range(2)]})
    torch.cuda.synchronize()
    for n, step in enumerate(steps):  # the two frames' passes enqueued alternately, each frame on its own stream
        for b, (color, _, _), p, s in zip(bufs, frames, ps, streams):
            dst = b["work"][n & 1]
            api.denoise_atrous_pass_device(color.shape[1], color.shape[0], step, p, b["src"][0].data_ptr(), b["src"][1].data_ptr(), b["g"].data_ptr(),
                                           dst[0].data_ptr(), dst[1].data_ptr(), stream=s.cuda_stream)
            b["src"] = dst
    for s in streams:
        s.synchronize()
    for b, (want_c, want_v) in zip(bufs, alone):
        assert _same(b["src"][0].cpu().numpy(), want_c) and _same(b["src"][1].cpu().numpy(), want_v)


def test_end_to_end_on_bouncing_spheres(rl):
    """render_moments and render_features at 4 spp through denoise_render against a 1024-spp render of the same camera: the denoised image's
    mean squared error is lower than the noisy one's (no margin: the filter must not make things worse; the ratio this prints is what
    tools/denoise_ab.py records in profiles/denoise.json).  The same buffers through the model give the call's bytes."""
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    p = dataclasses.replace(world.params, image_width=64, aspect_ratio=64 / 48.5, samples_per_pixel=4)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (64, 48)
    moments, features = cam.render_moments(world), cam.render_features(world)
    truth = rl.Camera(dataclasses.replace(p, samples_per_pixel=1024)).render(world).pixel_data()
    noisy = moments.sums * (1.0 / moments.samples)
    color, variance = api.denoise_render(moments, features)
    assert np.isfinite(color).all() and np.isfinite(variance).all()
    before, after = M.mse(noisy, truth), M.mse(color, truth)
    print(f"bouncing_spheres 64x48 at 4 spp: mse noisy {before:.4e}, denoised {after:.4e}, ratio {after / before:.3f}")
    assert after < before
    cin, vin, guides, sigmas, a = api._denoise_render_inputs(moments, features, None, api.GUIDE_KINDS)
    prm = api.atrous_params(guides.shape[2], guide_sigma=sigmas)
    got_c, got_v = api.denoise_atrous(cin, vin, guides, params=prm)
    want_c, want_v = M.atrous(cin, vin, guides, *M.params_of(prm), 5)
    assert _same(got_c, want_c) and _same(got_v, want_v)
    assert _same(got_c * a, color) and _same(got_v * (a * a), variance)
