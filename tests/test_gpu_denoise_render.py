"""GPU tier: denoise_render on the device (rl_denoise_prepare_device, rl_denoise_finish_device, rl_denoise_render_device, rl_denoise_render,
rl_rtiow_render_denoised_rgb8; include/rl_render.h "Denoising").  The yardstick is tests/denoise_render_model.py, the
header's statement in numpy, which tests/test_denoise_render_abi.py pins to the host path.  No tolerance anywhere: outputs are compared as
bytes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import atrous_model as M
import denoise_render_model as DM

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WANTS = {"all": 15, "albedo": 1, "depth+coverage": 12, "normal": 2}
SHAPES = {"1x1": (1, 1, 0), "37x23": (23, 37, 0), "37x23 in 2 workgroups": (23, 37, 2), "256x1": (1, 256, 0)}  # (H, W, set_denoise_blocks)


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_denoise_blocks(0)


def _same(a, b):
    return a.tobytes() == b.tobytes()


def _to_device(rl, m: DM.Inputs):
    """(api.DenoiseInputs of device pointers, the torch tensors that own them)."""
    import torch
    def tensor(a):  # uint32 images travel as their int32 bits
        a = np.ascontiguousarray(a)
        return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to(DEV)
    keep = {k: tensor(getattr(m, k)) for k in ("sums", "sq", "counts", "albedo_sum", "normal_sum", "depth_sum", "hit_count") if getattr(m, k) is not None}
    d = rl.api.denoise_inputs({k: t.data_ptr() for k, t in keep.items()}, want=m.want, samples=m.samples, feature_samples=m.feature_samples)
    return d, keep


def _params(rl, G, seed=5):
    inv = list(np.random.default_rng(seed).uniform(0.25, 4.0, G))
    return rl.api.atrous_params(G, color_sigma=2.0, guide_inv_sigma=inv, variance_floor=1e-8)


@pytest.fixture(scope="module")
def frames():
    """The CPU test's hand-made sums, tiled: {(shape id, with_counts): Inputs with want = all four}.  Read-only."""
    return {(sid, wc): DM.tiled(DM.hand_made(wc), H, W) for sid, (H, W, _) in SHAPES.items() for wc in (False, True)}


def test_device_sqrt_is_the_correctly_rounded_one(rl):
    """The one operation of the definition beyond + - * /: the normal guide of normal_sums whose squared length is not a square, against
    np.sqrt (correctly rounded, as IEEE 754 asks).  An approximate sqrt (v_sqrt_f64 alone is good to about 2^-26 relative) cannot give these
    bytes on 4096 random vectors."""
    import torch
    rng = np.random.default_rng(23)
    H, W = 16, 256
    ns = rng.standard_normal((H, W, 3)) * np.exp2(rng.integers(-40, 40, (H, W, 1)))
    m = DM.Inputs(sums=np.ones((H, W, 3)), sq=np.ones((H, W, 3)), albedo_sum=np.ones((H, W, 3)), feature_samples=1, samples=2, normal_sum=ns, want=DM.GUIDE_NORMAL)
    want = DM.prepare(m)[2]
    length = np.sqrt((ns[..., 0] * ns[..., 0] + ns[..., 1] * ns[..., 1]) + ns[..., 2] * ns[..., 2])
    assert _same(want, ns / length[..., None]) and (length * length != (ns[..., 0] * ns[..., 0] + ns[..., 1] * ns[..., 1]) + ns[..., 2] * ns[..., 2]).any()
    d, keep = _to_device(rl, m)
    out = [torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=DEV) for _ in range(3)]
    rl.api.denoise_prepare_device(W, H, d, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr())
    torch.cuda.synchronize()
    got = out[2].cpu().numpy()
    assert _same(got, want), float(np.abs(got / want - 1.0).max())


@pytest.mark.parametrize("want", WANTS.values(), ids=WANTS.keys())
@pytest.mark.parametrize("with_counts", [False, True], ids=["moments", "adaptive"])
@pytest.mark.parametrize("sid", SHAPES.keys())
def test_prepare_and_finish_give_the_model_bytes(rl, frames, sid, with_counts, want):
    """1 x 1; 37 x 23, a multiple of no block edge, by default and with two workgroups, so that both kernels take later trips of their
    grid-stride loop; 256 x 1, exactly one block."""
    import torch
    api = rl.api
    H, W, blocks = SHAPES[sid]
    m = dataclasses.replace(frames[sid, with_counts], want=want)
    G = DM.n_guides(want)
    want_c, want_v, want_g = DM.prepare(m)
    rng = np.random.default_rng(9)
    cf, vf = want_c * rng.uniform(0.5, 1.5, want_c.shape), want_v * rng.uniform(0.5, 1.5, want_c.shape)  # what the passes might leave
    fin_c, fin_v = DM.finish(cf, vf, m.albedo_sum, m.feature_samples)
    d, keep = _to_device(rl, m)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    color, variance, guides = nan(H, W, 3), nan(H, W, 3), nan(H, W, G + 1)  # one channel more than G: the kernel must stop at H * W * G doubles
    d_cf, d_vf = torch.from_numpy(cf).to(DEV), torch.from_numpy(vf).to(DEV)
    out_c, out_v = nan(H, W, 3), nan(H, W, 3)
    out_u8, only_u8, ref_u8 = (torch.full((H, W, 3), fill, dtype=torch.uint8, device=DEV) for fill in (7, 8, 9))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        api.set_denoise_blocks(blocks)
        api.denoise_prepare_device(W, H, d, color.data_ptr(), variance.data_ptr(), guides.data_ptr(), stream=s.cuda_stream)
        api.denoise_finish_device(W, H, d_cf.data_ptr(), d_vf.data_ptr(), keep["albedo_sum"].data_ptr(), m.feature_samples, out_c.data_ptr(), out_v.data_ptr(),
                                  out_u8.data_ptr(), stream=s.cuda_stream)
        # ... the picture alone, and in place
        api.denoise_finish_device(W, H, d_cf.data_ptr(), 0, keep["albedo_sum"].data_ptr(), m.feature_samples, d_out_rgb8=only_u8.data_ptr(), stream=s.cuda_stream)
        api.denoise_finish_device(W, H, d_cf.data_ptr(), d_vf.data_ptr(), keep["albedo_sum"].data_ptr(), m.feature_samples, d_cf.data_ptr(), d_vf.data_ptr(),
                                  stream=s.cuda_stream)
        api.render_lib().rl_rtiow_encode_rgb8_device(out_c.data_ptr(), H * W, 1, ref_u8.data_ptr(), s.cuda_stream)
        s.synchronize()
    finally:
        api.set_denoise_blocks(0)
    assert _same(color.cpu().numpy(), want_c) and _same(variance.cpu().numpy(), want_v)
    flat = guides.cpu().numpy().reshape(-1)
    assert _same(flat[:H * W * G], want_g.reshape(-1)) and np.isnan(flat[H * W * G:]).all()
    assert _same(out_c.cpu().numpy(), fin_c) and _same(out_v.cpu().numpy(), fin_v)
    assert _same(d_cf.cpu().numpy(), fin_c) and _same(d_vf.cpu().numpy(), fin_v)
    assert torch.equal(out_u8, ref_u8) and torch.equal(only_u8, ref_u8)


def _render_device(rl, m, p, iterations, variance=True, rgb8=True, blocks=0):
    """denoise_render_device on a fresh non-default stream, the work buffer pre-filled with NaN -> (color, variance or None, rgb8 or None) on the host."""
    import torch
    api = rl.api
    H, W = m.sums.shape[:2]
    d, keep = _to_device(rl, m)
    work_bytes = api.denoise_render_work_bytes(W, H, p.n_guides)
    work = torch.full((work_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    out_c = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=DEV)
    out_v = torch.full_like(out_c, float("nan")) if variance else None
    out_u8 = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV) if rgb8 else None
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        api.set_denoise_blocks(blocks)
        api.denoise_render_device(W, H, d, iterations, p, work.data_ptr(), work_bytes, out_c.data_ptr(), out_v.data_ptr() if variance else 0,
                                  out_u8.data_ptr() if rgb8 else 0, stream=s.cuda_stream)
        s.synchronize()
    finally:
        api.set_denoise_blocks(0)
    return out_c.cpu().numpy(), out_v.cpu().numpy() if variance else None, out_u8.cpu().numpy() if rgb8 else None


def _encode(rl, color):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(color)).to(DEV)
    u8 = torch.full(color.shape, 9, dtype=torch.uint8, device=DEV)
    assert rl.api.render_lib().rl_rtiow_encode_rgb8_device(t.data_ptr(), color.shape[0] * color.shape[1], 1, u8.data_ptr(), None) == 0
    torch.cuda.synchronize()
    return u8.cpu().numpy()


@pytest.fixture(scope="module")
def frame_37x23(frames):
    return frames["37x23", True]


@pytest.mark.parametrize("iterations", [0, 1, 5])
def test_render_device_gives_the_model_bytes(rl, frame_37x23, iterations):
    m = frame_37x23
    p = _params(rl, 8)
    want_c, want_v = DM.render(m, M.params_of(p), iterations)
    assert np.isfinite(want_c).all() and np.isfinite(want_v).all()
    got_c, got_v, got_u8 = _render_device(rl, m, p, iterations)
    assert _same(got_c, want_c), float(np.abs(got_c - want_c).max())
    assert _same(got_v, want_v), float(np.abs(got_v - want_v).max())
    assert _same(got_u8, _encode(rl, got_c))
    only_c, none, _ = _render_device(rl, m, p, iterations, variance=False, rgb8=False)  # the last pass without a variance output
    assert none is None and _same(only_c, want_c)
    # the picture alone, every kernel in two workgroups
    import torch
    d, keep = _to_device(rl, m)
    work_bytes = rl.api.denoise_render_work_bytes(37, 23, 8)
    work = torch.full((work_bytes // 8,), float("nan"), dtype=torch.float64, device=DEV)
    u8 = torch.full((23, 37, 3), 7, dtype=torch.uint8, device=DEV)
    try:
        rl.api.set_denoise_blocks(2)
        rl.api.denoise_render_device(37, 23, d, iterations, p, work.data_ptr(), work_bytes, d_out_rgb8=u8.data_ptr())
        torch.cuda.synchronize()
    finally:
        rl.api.set_denoise_blocks(0)
    assert _same(u8.cpu().numpy(), got_u8)


def test_non_finite_inputs_stay_local(rl, frame_37x23):
    """One pixel that took one sample and one that took none: after two passes (steps 1 and 2) the non-finite output pixels are exactly
    the model's, those within 2 + 4 pixels of either in both directions, and the bytes of the others are the model's too."""
    one, zero = (5, 30), (17, 8)
    m = DM.with_short_pixels(frame_37x23, one, zero)
    p = _params(rl, 8)
    want_c, want_v = DM.render(m, M.params_of(p), 2)
    got_c, got_v, _ = _render_device(rl, m, p, 2, rgb8=False)
    bad = lambda a: ~np.isfinite(a).all(axis=-1)
    ys, xs = np.mgrid[0:23, 0:37]
    reach = np.zeros((23, 37), dtype=bool)
    for y, x in (one, zero):
        reach |= (np.abs(ys - y) <= 6) & (np.abs(xs - x) <= 6)
    assert (bad(want_c) <= reach).all() and bad(want_c)[one] and bad(want_c)[zero] and not bad(want_c).all()
    assert (bad(got_c) == bad(want_c)).all() and (bad(got_v) == bad(want_v)).all()
    ok = ~bad(want_c)
    assert _same(got_c[ok], want_c[ok]) and _same(got_v[~bad(want_v)], want_v[~bad(want_v)])


@pytest.fixture(scope="module")
def spheres(rl):
    """bouncing_spheres 64 x 48 at 4 spp: (world, camera, Moments, Adaptive, Features).  Rendered once, read-only."""
    world = rl.World.bouncing_spheres(1)
    p = dataclasses.replace(world.params, image_width=64, aspect_ratio=64 / 48.5, samples_per_pixel=4)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (64, 48)
    return world, cam, cam.render_moments(world), cam.render_adaptive(world, 2, 1, abs_variance=1e-3, rel_variance=1e-2), cam.render_features(world)


@pytest.mark.parametrize("kind", ["moments", "adaptive"])
def test_denoise_render_gpu_gives_the_host_path_bytes(rl, spheres, kind):
    api = rl.api
    world, cam, moments, adaptive, features = spheres
    est = moments if kind == "moments" else adaptive
    if kind == "adaptive":
        assert len(np.unique(adaptive.counts)) > 1 and adaptive.counts.min() >= 2
    want_c, want_v = api.denoise_render(est, features)
    before = api.live_buffers()
    got_c, got_v, got_u8 = api.denoise_render_gpu(est, features, rgb8=True)
    assert api.live_buffers() == before
    assert _same(got_c, want_c) and _same(got_v, want_v)
    assert _same(got_u8, _encode(rl, got_c))
    for want in (("albedo",), ("depth", "coverage")):
        a, b = api.denoise_render(est, features, iterations=2, want=want), api.denoise_render_gpu(est, features, iterations=2, want=want)
        assert _same(a[0], b[0]) and _same(a[1], b[1]), want
    # the C++ mirror's probe
    Hl = api.host_lib()
    Hl.rlh_denoise_render_probe.argtypes = ([C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(api.AtrousParams)] + [C.c_void_p] * 3 + [C.c_uint64] + [C.c_void_p] * 4
                                            + [C.c_uint64, C.c_uint32] + [C.c_void_p] * 2)
    prm = api.atrous_params(8, guide_sigma=api._denoise_render_inputs(est, features, None, api.GUIDE_KINDS)[3])
    mc, mv = np.empty_like(got_c), np.empty_like(got_v)
    counts = adaptive.counts.ctypes.data if kind == "adaptive" else None
    assert Hl.rlh_denoise_render_probe(64, 48, 5, C.byref(prm), est.sums.ctypes.data, est.sq.ctypes.data, counts, 0 if counts else est.samples,
                                       features.albedo_sum.ctypes.data, features.normal_sum.ctypes.data, features.depth_sum.ctypes.data,
                                       features.hit_count.ctypes.data, features.samples, 15, mc.ctypes.data, mv.ctypes.data) == 0, Hl.rlh_last_error()
    assert _same(mc, got_c) and _same(mv, got_v)


@pytest.mark.parametrize("rule", [None, (2, 1, 1e-3, 1e-2)], ids=["moments", "adaptive"])
def test_render_denoised_rgb8_is_the_composition(rl, spheres, rule):
    """Camera.render_denoised_rgb8 against the same composition written here from the device forms on torch buffers."""
    import torch
    api = rl.api
    world, cam, *_ = spheres
    H, W, FS = 48, 64, 2
    got = cam.render_denoised_rgb8(world, FS, rule=rule, iterations=3)
    assert got.shape == (H, W, 3) and got.dtype == np.uint8
    f64 = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)
    sums, sq, albedo, normal, depth = f64(H, W, 3), f64(H, W, 3), f64(H, W, 3), f64(H, W, 3), f64(H, W)
    counts, hits = (torch.zeros((H, W), dtype=torch.int32, device=DEV) for _ in range(2))
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    if rule is None:
        cam.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s.cuda_stream)
    else:
        cam.render_adaptive_device(world, rule[0], rule[1], sums.data_ptr(), sq.data_ptr(), counts.data_ptr(), abs_variance=rule[2], rel_variance=rule[3],
                                   stream=s.cuda_stream)
    fcam = rl.Camera(dataclasses.replace(cam.params, samples_per_pixel=FS))
    fcam.render_features_device(world, stream=s.cuda_stream, d_albedo_sum=albedo.data_ptr(), d_normal_sum=normal.data_ptr(), d_depth_sum=depth.data_ptr(),
                                d_hit_count=hits.data_ptr())
    ptrs = {"sums": sums.data_ptr(), "sq": sq.data_ptr(), "albedo_sum": albedo.data_ptr(), "normal_sum": normal.data_ptr(), "depth_sum": depth.data_ptr(),
            "hit_count": hits.data_ptr(), "counts": counts.data_ptr() if rule is not None else 0}
    d = api.denoise_inputs(ptrs, samples=cam.params.samples_per_pixel, feature_samples=FS)
    D = api.DENOISE_GUIDE_SIGMA
    p = api.atrous_params(8, guide_sigma=[D["albedo"]] * 3 + [D["normal"]] * 3 + [D["depth"], D["coverage"]])
    work_bytes = api.denoise_render_work_bytes(W, H, 8)
    work = torch.empty((work_bytes // 8,), dtype=torch.float64, device=DEV)
    u8 = torch.full((H, W, 3), 7, dtype=torch.uint8, device=DEV)
    api.denoise_render_device(W, H, d, 3, p, work.data_ptr(), work_bytes, d_out_rgb8=u8.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    api.render_status(world)
    assert _same(got, u8.cpu().numpy())
    if rule is not None:
        assert len(torch.unique(counts)) > 1
    assert len(np.unique(got)) > 32  # ... and it is a picture, not one colour
