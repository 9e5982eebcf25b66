"""GPU tier: the pixel-list renders (Camera.render_pixels / RtcWorld.render_pixels and their _device forms; include/rl_render.h "Pixel-list
renders").

The yardstick needs no tolerance: a pixel's stream is sample_index*W*H + x*W + y, its samples chain only within the pixel and every fast
path re-traces its order-sensitive rays, so a pixel rendered from a list is bit for bit the same pixel of the full frame — whatever else
is in the list, in whatever order, through whichever of the list kernels (cooperative, fast general, reference-order general)."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
SPHERE_SCENES = ["golden_test_scene", "bouncing_spheres"]
SCENES = SPHERE_SCENES + ["cornell_smoke", "cow_scene", "flat_world", "final_scene"]
SPP = 3
TOL = 1e-4  # tests/test_gpu_parity.py: per-channel tolerance on pixel RGB (means)


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_coop(True)
    rl.api.set_coop_pixels_max(0)
    rl.api.set_fast_traversal(True)


def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


def _scene(rl, golden, name, width=None):
    """(world, camera params) at a reduced frame."""
    if name == "golden_test_scene":
        w = rl.World.golden_test_scene()
    elif name == "bouncing_spheres":
        w = rl.World.bouncing_spheres(1)
    elif name == "cow_scene":
        w = rl.World.cow_scene(golden("spot_triangulated.obj.gz"), _spot_texture())
    elif name == "final_scene":
        w = rl.World.example_scene(name, rgb8=_spot_texture()[::8, ::8])
    else:
        w = rl.World.example_scene(name)
    p = w.params
    p.image_width = width or (40 if name == "final_scene" else 64 if p.aspect_ratio >= 4.0 / 3.0 else 48)  # at most 64 x 48
    p.max_depth = min(p.max_depth, 20)
    return w, p


_cache = {}


def _setup(rl, golden, name):
    """The scene, its camera at SPP samples and the two frames the lists are compared against (rendered once, with the switches at their
    defaults, and never written to afterwards)."""
    if name not in _cache:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)
        world, p = _scene(rl, golden, name)
        cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=SPP))
        gs = {}
        frame = cam.render(world, stats=gs, allow_degenerate=True).data
        frame3 = cam.render_rows(world, 0, 1, first_sample=3)
        frame.setflags(write=False), frame3.setflags(write=False)
        _cache[name] = (world, cam, frame, frame3, gs)
    return _cache[name]


def _lists(W, H):
    """The four list shapes: every pixel in a fixed-seed random order; one pixel; 65 (one more than a wave claim); 130 with the four
    corners, duplicates, the last row and the last column."""
    rng = np.random.default_rng(20261018)
    perm = rng.permutation(W * H)
    py, px = np.divmod(perm, W)
    one = (np.array([W - 2]), np.array([H // 2]))
    i65 = rng.integers(0, W * H, 65)
    y65, x65 = np.divmod(i65, W)
    xs = [0, W - 1, 0, W - 1, 5, 5, 5, W - 1, W - 1]  # corners, a triple, a doubled corner
    ys = [0, 0, H - 1, H - 1, 7, 7, 7, H - 1, H - 1]
    xs = xs + list(range(W))  # the last row
    ys = ys + [H - 1] * W
    assert len(xs) + H <= 130
    xs = xs + [W - 1] * (130 - len(xs))  # the last column, and once more from its top
    ys = ys + [k % H for k in range(130 - len(ys))]
    return {"perm": (px, py), "one": one, "65": (x65, y65), "130": (np.array(xs), np.array(ys))}


def _assert_bits(out, frame, xs, ys, what):
    want = np.ascontiguousarray(frame[ys, xs])
    assert out.shape == want.shape and out.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("name", SCENES)
def test_listed_pixels_are_the_frames_pixels_bit_for_bit(rl, golden, name):
    world, cam, frame, frame3, _ = _setup(rl, golden, name)
    W, H = cam.c.image_width, cam.c.image_height
    assert frame.shape == (H, W, 3) and W <= 64 and H <= 48
    lists = _lists(W, H)
    assert len(lists["130"][0]) == 130 and len(lists["65"][0]) == 65 and len(lists["perm"][0]) == W * H
    try:
        for coop in ((True, False) if name in SPHERE_SCENES else (True,)):
            for fast in (True, False):
                rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
                for key, (xs, ys) in lists.items():
                    out = cam.render_pixels(world, xs, ys, allow_degenerate=True)
                    _assert_bits(out, frame, xs, ys, (name, coop, fast, key, 0))
                    out3 = cam.render_pixels(world, xs, ys, first_sample=3, allow_degenerate=True)
                    _assert_bits(out3, frame3, xs, ys, (name, coop, fast, key, 3))
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)
    # duplicates got identical bits (the triple at (5, 7) of the 130 list)
    xs, ys = lists["130"]
    out = cam.render_pixels(world, xs, ys, allow_degenerate=True)
    assert out[4].tobytes() == out[5].tobytes() == out[6].tobytes()


@pytest.mark.parametrize("name", SCENES)
def test_counting_list_of_every_pixel_has_the_frames_counters(rl, golden, name):
    """All seven counters of a counting render_pixels over a permutation of the frame equal the counting render's — for sphere-only scenes
    too, where the frame runs the guarded LDS layout of the sphere kernel and the list runs the general kernel."""
    world, cam, frame, _, gs = _setup(rl, golden, name)
    xs, ys = _lists(cam.c.image_width, cam.c.image_height)["perm"]
    ls = {}
    out = cam.render_pixels(world, xs, ys, stats=ls, allow_degenerate=True)
    _assert_bits(out, frame, xs, ys, name)
    for k in COUNTERS:
        assert ls[k] == gs[k], (name, k, ls[k], gs[k])
    assert ls["rc"] == gs["rc"]


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_smoke"])
def test_listed_pixels_against_the_oracle(rl, oracle, golden, name):
    world, p = _scene(rl, golden, name, width=96)
    cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=4))
    W, H = cam.c.image_width, cam.c.image_height
    idx = np.random.default_rng(7).integers(0, W * H, 300)
    ys, xs = np.divmod(idx, W)
    gs, cs = {}, {}
    gpu = cam.render_pixels(world, xs, ys, stats=gs, allow_degenerate=True)
    cpu = oracle.rtiow_render_pixels(world.desc, cam.c, xs, ys, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    err = np.abs(gpu - cpu).max()
    print(f"{name}: max |gpu - oracle| = {err:.3e} (sums), rays {gs['rays']}")
    assert err / 4 <= TOL
    assert err <= 1e-9 * max(1.0, np.abs(cpu).max()), err
    fast = cam.render_pixels(world, xs, ys, allow_degenerate=True)  # the counter-free path: the same bits
    assert fast.tobytes() == gpu.tobytes()


def test_list_longer_than_the_frame_paths_cooperative_threshold(rl):
    """A sphere-scene list longer than 160 elements per CU — the bound up to which the frame path and the list path use the cooperative
    kernel — with the switches at their defaults (the reference-order kernel takes it), with the bound lifted (the cooperative kernel at a
    length the frame never gives it), and a list of exactly the bound: each equals the frame bit for bit."""
    world = rl.World.bouncing_spheres(1)
    p = dataclasses.replace(world.params, image_width=256, aspect_ratio=4.0 / 3.0, samples_per_pixel=1, max_depth=8)
    cam = rl.Camera(p)
    W, H = cam.c.image_width, cam.c.image_height
    assert (W, H) == (256, 192)
    name = C.create_string_buffer(64)
    bound = rl.api.render_lib().rl_device_info(name, 64) * 160
    assert W * H > bound
    frame = cam.render(world).data
    ys, xs = np.divmod(np.random.default_rng(3).permutation(W * H), W)
    out = cam.render_pixels(world, xs, ys)
    _assert_bits(out, frame, xs, ys, "crossing, defaults")
    out = cam.render_pixels(world, xs[:bound], ys[:bound])
    _assert_bits(out, frame, xs[:bound], ys[:bound], "at the bound")
    try:
        rl.api.set_coop_pixels_max(1 << 40)
        out = cam.render_pixels(world, xs, ys)
    finally:
        rl.api.set_coop_pixels_max(0)
    _assert_bits(out, frame, xs, ys, "crossing, bound lifted")


@pytest.mark.parametrize("path", ["coop", "reference", "fast_general"])
def test_device_form_and_pixels_outside_the_image(rl, golden, path):
    import torch
    dev = torch.device("cuda", 0)
    api = rl.api
    world, cam, frame, _, _ = _setup(rl, golden, "cornell_smoke" if path == "fast_general" else "golden_test_scene")
    W, H = cam.c.image_width, cam.c.image_height
    xs, ys = _lists(W, H)["130"]
    xs, ys = xs.copy(), ys.copy()
    bad = [3, 64, 129]
    xs[3], ys[64], xs[129], ys[129] = W, H, 0xFFFFFFFF, 0xFFFFFFFF  # one past the last column / row, and far outside
    good = np.setdiff1d(np.arange(130), bad)
    d_xs = torch.from_numpy(xs.astype(np.uint32).view(np.int32)).to(dev)
    d_ys = torch.from_numpy(ys.astype(np.uint32).view(np.int32)).to(dev)
    d_out = torch.full((130, 3), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    try:
        api.set_fast_traversal(path != "reference")
        cam.render_pixels_device(world, d_xs.data_ptr(), d_ys.data_ptr(), 130, d_out.data_ptr(), stream=stream.cuda_stream)
        st = api.render_status(world, allow_degenerate=True)
        host = cam.render_pixels(world, xs[good], ys[good], allow_degenerate=True)
        cs = {}
        cam.render_pixels(world, xs[good], ys[good], stats=cs, allow_degenerate=True)
    finally:
        api.set_fast_traversal(True)
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    assert out[good].tobytes() == host.tobytes()  # the same bytes as the host form's; neighbours of the bad elements unaffected
    _assert_bits(out[good], frame, xs[good], ys[good], path)
    assert not out[bad].any() and not np.isnan(out).any()  # written as zeros
    assert st["rays"] == cs["rays"]  # and nothing was traced for them
    # the host form refuses the list before anything is launched and leaves `out` untouched
    h_out = np.full((130, 3), np.nan)
    x32, y32 = xs.astype(np.uint32), ys.astype(np.uint32)
    rc = api.render_lib().rl_rtiow_render_pixels(world.device(), C.byref(cam.c), 0, x32.ctypes.data, y32.ctypes.data, 130, h_out.ctypes.data, None)
    assert rc == api.RL_E_INVALID and np.isnan(h_out).all()
    with pytest.raises(rl.RLError) as e:
        cam.render_pixels(world, xs, ys)
    assert e.value.code == api.RL_E_INVALID


def test_empty_list_null_buffers_and_the_other_family(rl, golden):
    api = rl.api
    lib = api.render_lib()
    world, cam, _, _, _ = _setup(rl, golden, "golden_test_scene")
    rw = rl.RtcWorld.test_csg_scene(60, 40)
    st = api.Stats()
    st.rays = 77
    assert lib.rl_rtiow_render_pixels(world.device(), C.byref(cam.c), 0, None, None, 0, None, C.byref(st)) == api.RL_OK and st.rays == 0
    assert cam.render_pixels(world, [], []).shape == (0, 3) and rw.render_pixels([], []).shape == (0, 3)
    xs = np.zeros(2, dtype=np.uint32)
    out = np.full((2, 3), np.nan)
    assert lib.rl_rtiow_render_pixels(world.device(), C.byref(cam.c), 0, xs.ctypes.data, None, 2, out.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_pixels(world.device(), C.byref(cam.c), 0, xs.ctypes.data, xs.ctypes.data, 2, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_pixels(rw.device(), C.byref(cam.c), 0, xs.ctypes.data, xs.ctypes.data, 2, out.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtc_render_pixels(world.device(), C.byref(rw.camera), 1, xs.ctypes.data, xs.ctypes.data, 2, out.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtc_render_pixels(rw.device(), C.byref(rw.camera), 0, xs.ctypes.data, xs.ctypes.data, 2, out.ctypes.data, None) == api.RL_E_INVALID
    n_big = 0xFFFF0000  # the 32-bit work counter's bound: refused before any buffer is read
    assert lib.rl_rtiow_render_pixels_device(world.device(), C.byref(cam.c), 0, xs.ctypes.data, xs.ctypes.data, n_big, out.ctypes.data, None, None) == api.RL_E_INVALID
    assert b"image too large" in lib.rl_last_error()
    assert lib.rl_rtc_render_pixels_device(rw.device(), C.byref(rw.camera), 1, xs.ctypes.data, xs.ctypes.data, n_big, out.ctypes.data, None, None) == api.RL_E_INVALID
    assert b"image too large" in lib.rl_last_error()
    assert np.isnan(out).all()


@pytest.mark.parametrize("scene", ["obj", "csg", "mirror"])
def test_rtc_listed_pixels_are_the_frames_pixels(rl, golden, scene):
    """test_obj_scene goes through rtc_kernel, the CSG and mirror scenes through rtc_full_kernel."""
    import torch
    dev = torch.device("cuda", 0)
    W, H = 60, 40
    rw = (rl.RtcWorld.test_obj_scene(golden("teapot-low.obj"), W, H) if scene == "obj" else
          rl.RtcWorld.test_csg_scene(W, H) if scene == "csg" else rl.RtcWorld.test_mirror_scene(W, H))
    lists = _lists(W, H)
    for aa in (1, 2):
        fs = {}
        frame = rw.render(aa, stats=fs)
        for key, (xs, ys) in lists.items():
            ls = {}
            out = rw.render_pixels(xs, ys, aa, stats=ls)
            _assert_bits(out, frame, xs, ys, (scene, aa, key))
            if key == "perm":
                for k in COUNTERS:
                    assert ls[k] == fs[k], (scene, aa, k, ls[k], fs[k])
    # the _device form on a stream of its own, with elements outside the image
    xs, ys = lists["130"]
    xs, ys = xs.copy(), ys.copy()
    xs[0], ys[77] = W, H
    good = np.setdiff1d(np.arange(130), [0, 77])
    d_xs = torch.from_numpy(xs.astype(np.uint32).view(np.int32)).to(dev)
    d_ys = torch.from_numpy(ys.astype(np.uint32).view(np.int32)).to(dev)
    d_out = torch.full((130, 3), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    rw.render_pixels_device(d_xs.data_ptr(), d_ys.data_ptr(), 130, d_out.data_ptr(), 2, stream=stream.cuda_stream)
    rl.api.render_status(rw)
    torch.cuda.synchronize(dev)
    out = d_out.cpu().numpy()
    _assert_bits(out[good], frame, xs[good], ys[good], (scene, "device"))
    assert not out[[0, 77]].any()
    with pytest.raises(rl.RLError) as e:
        rw.render_pixels(xs, ys, 2)
    assert e.value.code == rl.api.RL_E_INVALID


def test_two_asynchronous_list_renders_are_both_accounted_for(rl, golden):
    """Two rl_rtiow_render_pixels_device calls back to back on one scene, on two streams, no host sync between them: both outputs are the
    frame's pixels, and rl_render_status reports the rays of the one enqueued last and no flag."""
    import torch
    dev = torch.device("cuda", 0)
    world, cam, frame, _, _ = _setup(rl, golden, "bouncing_spheres")
    lists = _lists(cam.c.image_width, cam.c.image_height)
    rays, bufs, streams = {}, {}, {}
    for key in ("perm", "130"):
        xs, ys = lists[key]
        cs = {}
        cam.render_pixels(world, xs, ys, stats=cs)
        rays[key] = cs["rays"]
        bufs[key] = (torch.from_numpy(xs.astype(np.uint32).view(np.int32)).to(dev), torch.from_numpy(ys.astype(np.uint32).view(np.int32)).to(dev),
                     torch.full((len(xs), 3), float("nan"), dtype=torch.float64, device=dev))
        streams[key] = torch.cuda.Stream(dev)
    assert rays["perm"] != rays["130"]
    torch.cuda.synchronize(dev)
    for key in ("perm", "130"):
        d_xs, d_ys, d_out = bufs[key]
        cam.render_pixels_device(world, d_xs.data_ptr(), d_ys.data_ptr(), d_xs.numel(), d_out.data_ptr(), stream=streams[key].cuda_stream)
    st = rl.api.render_status(world)
    torch.cuda.synchronize(dev)
    assert st["rays"] == rays["130"] and st["flagged"] == 0
    for key in ("perm", "130"):
        _assert_bits(bufs[key][2].cpu().numpy(), frame, *lists[key], key)


def test_progress_follows_a_list_render(rl, golden):
    world, p = _scene(rl, golden, "golden_test_scene")
    cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=2))
    assert rl.api.render_progress(world) == (0, 0, 0)  # the first call switches the host-visible work counters on
    xs, ys = _lists(cam.c.image_width, cam.c.image_height)["130"]
    for coop in (True, False):
        try:
            rl.api.set_coop(coop)
            cam.render_pixels(world, xs, ys)
        finally:
            rl.api.set_coop(True)
        assert rl.api.render_progress(world) == (130, 130, 0)


def test_cpp_mirror_renders_listed_pixels(rl):
    H = rl.api.host_lib()
    H.rlh_render_pixels_probe.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
    world = rl.World.golden_test_scene()
    cam = rl.Camera(dataclasses.replace(world.params, image_width=48, samples_per_pixel=3))
    frame = cam.render(world).data
    xs, ys = _lists(cam.c.image_width, cam.c.image_height)["65"]
    x32, y32 = xs.astype(np.uint32), ys.astype(np.uint32)
    out = np.zeros((65, 3))
    assert H.rlh_render_pixels_probe(0, 48, 3, x32.ctypes.data, y32.ctypes.data, 65, out.ctypes.data) == 0, H.rlh_last_error()
    _assert_bits(out, frame, xs, ys, "rtiow mirror")
    rw = rl.RtcWorld.test_mirror_scene(60, 40)
    frame = rw.render(2)
    xs, ys = _lists(60, 40)["65"]
    x32, y32 = xs.astype(np.uint32), ys.astype(np.uint32)
    assert H.rlh_render_pixels_probe(1, 60, 2, x32.ctypes.data, y32.ctypes.data, 65, out.ctypes.data) == 0, H.rlh_last_error()
    _assert_bits(out, frame, xs, ys, "rtc mirror")
