"""GPU tier: the renders with second moments (Camera.render_moments / render_pixels_moments and their _device forms; include/rl_render.h
"Second moments").

No tolerance anywhere.  The second moment of a pixel and channel is sq = 0; for n ascending: sq = sq + c_n * c_n in binary64 (the product
rounded, then added), c_n being the colour sample n adds to the pixel's sum.  The yardstick takes the c_n from calls that do not know about
moments — the host loop of Camera.get_rays and World.ray_color_rays with the cursor carried from sample to sample — is first pinned to
Camera.render's frame (sum_n c_n in order, bit for bit), and then folded in numpy float64.  Every kernel that has the flavour (the wave
kernel's layouts, the cooperative kernel, the fast general kernel, the reference-order general kernel; frame and list forms) must give
those bits, and the sums next to them must stay the plain calls' bytes."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
SPHERE_SCENES = ["golden_test_scene", "bouncing_spheres"]
SCENES = SPHERE_SCENES + ["cornell_smoke", "flat_world"]
SPP = 3


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_coop(True)
    rl.api.set_fast_traversal(True)


def _routes(name):
    """(coop, fast) switch settings and the kernels a counter-free call then takes: sphere scenes — the cooperative kernel, the wave kernel's
    fast layout, its guarded compact layout (lists: the reference-order kernel); general scenes — the fast general kernel, the
    reference-order kernel."""
    return [(True, True), (False, True), (True, False)] if name in SPHERE_SCENES else [(True, True), (True, False)]


def _scene(rl, name, width=None, spp=SPP):
    w = rl.World.golden_test_scene() if name == "golden_test_scene" else rl.World.bouncing_spheres(1) if name == "bouncing_spheres" else rl.World.example_scene(name)
    p = w.params
    p.image_width = width or (24 if p.aspect_ratio >= 4.0 / 3.0 else 18)
    p.max_depth = min(p.max_depth, 10)
    cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=spp))
    assert cam.c.image_width <= 24 and cam.c.image_height <= 18
    return w, cam


def _pixels(cam):
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
    return x, y


def _sample_colours(rl, world, cam, F, S):
    """c[n, pixel, 3]: the colours of samples F .. F + S - 1 of every pixel (row-major), chained as Camera::_render chains them
    (camera.rs:161-174): sample n on stream (F + n) * W * H + x * W + y, from the word position the pixel's previous sample ended at."""
    api = rl.api
    W, H = cam.c.image_width, cam.c.image_height
    p = cam.params
    px, py = _pixels(cam)
    pos = np.zeros(px.shape[0], dtype=np.uint64)
    c = np.zeros((S, px.shape[0], 3))
    for n in range(S):
        cur = api.pack_cursors(np.uint64(F + n) * np.uint64(W * H) + px * np.uint64(W) + py, pos)
        rays, cur = cam.get_rays(px, py, cur)
        c[n], cur, _ = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays, allow_degenerate=True)
        pos = cur["word_pos"].copy()
    return c


def _fold(c):
    """(sum, sq) of c[n, ...] in ascending n, from 0.0, each product rounded before it is added."""
    s, q = np.zeros(c.shape[1:]), np.zeros(c.shape[1:])
    for n in range(c.shape[0]):
        s = s + c[n]
        q = q + c[n] * c[n]
    return s, q


_cache = {}


def _setup(rl, name):
    """Scene, camera at SPP samples, the plain frames of first_sample 0 and 3 and the yardstick's folds for both — built once, with the
    switches at their defaults, pinned to the plain frames, and never written to afterwards."""
    if name not in _cache:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)
        world, cam = _scene(rl, name)
        W, H = cam.c.image_width, cam.c.image_height
        out = {"world": world, "cam": cam}
        for F in (0, 3):
            gs = {}
            frame = cam.render_rows(world, 0, 1, first_sample=F, stats=gs)
            s, q = _fold(_sample_colours(rl, world, cam, F, SPP))
            s, q = s.reshape(H, W, 3), q.reshape(H, W, 3)
            assert s.tobytes() == frame.tobytes(), (name, F, "the yardstick's sums are not Camera.render's frame")
            for a in (frame, s, q):
                a.setflags(write=False)
            out[F] = (frame, q, gs)
        _cache[name] = out
    return _cache[name]


def _frame_device(rl, cam, world, first_sample=0, row_first=0, row_step=1):
    """render_moments_device into NaN-filled device buffers on a stream of its own -> (sums, sq) on the host.  The counter-free frame form:
    what reaches the cooperative, wave and fast general kernels (the host form counts, as Camera.render does)."""
    import torch
    dev = torch.device("cuda", 0)
    nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    d_s = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    d_q = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    cam.render_moments_device(world, d_s.data_ptr(), d_q.data_ptr(), stream=stream.cuda_stream, row_first=row_first, row_step=row_step, first_sample=first_sample)
    rl.api.render_status(world, allow_degenerate=True)
    torch.cuda.synchronize(dev)
    return d_s.cpu().numpy(), d_q.cpu().numpy()


def _same(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _shuffled(cam):
    W, H = cam.c.image_width, cam.c.image_height
    py, px = np.divmod(np.random.default_rng(20261018).permutation(W * H), W)
    return px, py


def _lists(W, H):
    """The 65-element list (one more than a wave claim) and the 130-element list with the four corners, duplicates, the last row and the
    last column (as tests/test_gpu_render_pixels.py)."""
    rng = np.random.default_rng(20261018)
    y65, x65 = np.divmod(rng.integers(0, W * H, 65), W)
    xs = [0, W - 1, 0, W - 1, 5, 5, 5, W - 1, W - 1]  # corners, a triple, a doubled corner
    ys = [0, 0, H - 1, H - 1, 7, 7, 7, H - 1, H - 1]
    xs = xs + list(range(W))  # the last row
    ys = ys + [H - 1] * W
    assert len(xs) + H <= 130
    xs = xs + [W - 1] * (130 - len(xs))  # the last column, and once more from its top
    ys = ys + [k % H for k in range(130 - len(ys))]
    return {"65": (x65, y65), "130": (np.array(xs), np.array(ys))}


@pytest.mark.parametrize("name", SCENES)
def test_sums_are_the_plain_calls_bytes_and_chained_moments_are_the_yardsticks(rl, name):
    """Cases 1 and 3: on every route, at first_sample 0 and 3, for the frame (device form and the counting host form) and for a list of all
    pixels in a shuffled order: sums = the plain call's bytes, sq = the yardstick's fold."""
    S = _setup(rl, name)
    world, cam = S["world"], S["cam"]
    px, py = _shuffled(cam)
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            for F in (0, 3):
                frame, want_sq, _ = S[F]
                what = (name, coop, fast, F)
                sums, sq = _frame_device(rl, cam, world, first_sample=F)
                assert _same(sums, frame), what
                assert _same(sq, want_sq), (what, "frame, device form")
                m = cam.render_moments(world, first_sample=F)
                assert m.samples == SPP and _same(m.sums, frame) and _same(m.sq, want_sq), (what, "frame, host form")
                lsums, lsq = cam.render_pixels_moments(world, px, py, first_sample=F)
                assert _same(lsums, cam.render_pixels(world, px, py, first_sample=F)) and _same(lsums, frame[py, px]), (what, "list sums")
                assert _same(lsq, want_sq[py, px]), (what, "list")
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)
    assert _same(S[0][0], cam.render(world).data)  # render itself is render_rows(0, 1): the frames above are Camera.render's


@pytest.mark.parametrize("name", SCENES)
def test_one_sample_moment_is_the_squared_sum(rl, name):
    """Case 2: with one sample per pixel sq = 0.0 + c * c and sums = 0.0 + c, on every route.  Needs no yardstick."""
    world, cam = _scene(rl, name, spp=1)
    px, py = _shuffled(cam)
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            for sums, sq in (_frame_device(rl, cam, world), cam.render_pixels_moments(world, px, py)):
                assert sums.any() and sq.tobytes() == (sums * sums).tobytes(), (name, coop, fast)
            m = cam.render_moments(world)
            assert m.sq.tobytes() == (m.sums * m.sums).tobytes(), (name, coop, fast, "host form")
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)


@pytest.mark.parametrize("name", ["golden_test_scene", "flat_world"])
def test_cost_sorted_resume_launch_carries_the_moments(rl, name):
    """Case 4: 72 samples per pixel on a 16-wide frame with the cooperative kernel off take the cost-sorted two-launch render (samples
    [0, 8), sort, resume): sq is stored at the end of the first launch and re-loaded by the second.  It equals the yardstick's fold, and,
    byte for byte, what the cooperative route (sphere scene) and the list route give."""
    S72 = 72
    world, cam = _scene(rl, name, width=16, spp=S72)
    W, H = cam.c.image_width, cam.c.image_height
    want_s, want_q = _fold(_sample_colours(rl, world, cam, 0, S72))
    want_s, want_q = want_s.reshape(H, W, 3), want_q.reshape(H, W, 3)
    px, py = _shuffled(cam)
    try:
        rl.api.set_coop(False), rl.api.set_fast_traversal(True)
        sums, sq = _frame_device(rl, cam, world)  # the wave kernel's fast layout / the fast general kernel, two launches
        assert _same(sums, want_s) and _same(sums, cam.render(world).data), name
        assert _same(sq, want_q), (name, "resume launch")
        rl.api.set_fast_traversal(False)
        sums, sq = _frame_device(rl, cam, world)  # the wave kernel's guarded compact layout / the reference-order kernel, two launches
        assert _same(sums, want_s) and _same(sq, want_q), (name, "resume launch, reference order")
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)
        if name in SPHERE_SCENES:
            csums, csq = _frame_device(rl, cam, world)  # the cooperative kernel, resumed too
            assert _same(csums, want_s) and _same(csq, want_q), (name, "cooperative")
        lsums, lsq = cam.render_pixels_moments(world, px, py)
        assert _same(lsums, want_s[py, px]) and _same(lsq, want_q[py, px]), (name, "list")
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)


@pytest.mark.parametrize("name", SCENES)
def test_row_shards_are_rows_of_the_full_frame(rl, name):
    """Case 5: row_first = 1, row_step = 3 gives rows 1, 4, 7, ... of the full frame's sums and sq."""
    S = _setup(rl, name)
    world, cam = S["world"], S["cam"]
    frame, want_sq, _ = S[0]
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            sums, sq = _frame_device(rl, cam, world, row_first=1, row_step=3)
            assert sums.shape[0] == len(range(1, cam.c.image_height, 3))
            assert _same(sums, frame[1::3]) and _same(sq, want_sq[1::3]), (name, coop, fast)
            assert _same(sums, cam.render_rows(world, 1, 3))
        m = cam.render_moments(world, row_first=1, row_step=3)
        assert _same(m.sums, frame[1::3]) and _same(m.sq, want_sq[1::3]), (name, "host form")
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)


@pytest.mark.parametrize("name", SCENES)
def test_lists_with_duplicates_corners_and_elements_outside_the_image(rl, name):
    """Case 6: every element of the 65 and the 130 list equals the frame's pixel in both outputs, duplicates get identical bits; in the
    _device form an element with x = W writes zeros to both outputs and changes no neighbour."""
    import torch
    dev = torch.device("cuda", 0)
    S = _setup(rl, name)
    world, cam = S["world"], S["cam"]
    frame, want_sq, _ = S[0]
    W, H = cam.c.image_width, cam.c.image_height
    lists = _lists(W, H)
    assert len(lists["65"][0]) == 65 and len(lists["130"][0]) == 130
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            for key, (xs, ys) in lists.items():
                sums, sq = cam.render_pixels_moments(world, xs, ys)
                assert _same(sums, frame[ys, xs]) and _same(sq, want_sq[ys, xs]), (name, coop, fast, key)
                if key == "130":  # the triple at (5, 7)
                    assert sq[4].tobytes() == sq[5].tobytes() == sq[6].tobytes() and sums[4].tobytes() == sums[5].tobytes() == sums[6].tobytes()
            xs, ys = lists["130"]
            xs, ys = xs.copy(), ys.copy()
            bad = [3, 64, 129]
            xs[3], xs[64], xs[129] = W, W, W  # one past the last column
            good = np.setdiff1d(np.arange(130), bad)
            d_xs = torch.from_numpy(xs.astype(np.uint32).view(np.int32)).to(dev)
            d_ys = torch.from_numpy(ys.astype(np.uint32).view(np.int32)).to(dev)
            d_s = torch.full((130, 3), float("nan"), dtype=torch.float64, device=dev)
            d_q = torch.full((130, 3), float("nan"), dtype=torch.float64, device=dev)
            stream = torch.cuda.Stream(dev)
            torch.cuda.synchronize(dev)
            cam.render_pixels_moments_device(world, d_xs.data_ptr(), d_ys.data_ptr(), 130, d_s.data_ptr(), d_q.data_ptr(), stream=stream.cuda_stream)
            rl.api.render_status(world, allow_degenerate=True)
            torch.cuda.synchronize(dev)
            sums, sq = d_s.cpu().numpy(), d_q.cpu().numpy()
            assert not sums[bad].any() and not sq[bad].any() and not np.isnan(sums).any() and not np.isnan(sq).any(), (name, coop, fast)
            assert _same(sums[good], frame[ys[good], xs[good]]) and _same(sq[good], want_sq[ys[good], xs[good]]), (name, coop, fast, "device form")
            with pytest.raises(rl.RLError) as e:  # the host form refuses the list
                cam.render_pixels_moments(world, xs, ys)
            assert e.value.code == rl.api.RL_E_INVALID
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)


@pytest.mark.parametrize("name", SCENES)
def test_counting_calls_have_the_plain_calls_counters(rl, name):
    """Case 7: with stats, the seven counters equal those of the plain call with the same arguments (frame, row shard, list)."""
    import torch
    S = _setup(rl, name)
    world, cam = S["world"], S["cam"]
    frame, want_sq, gs = S[0]
    ms = {}
    m = cam.render_moments(world, stats=ms)
    assert _same(m.sums, frame) and _same(m.sq, want_sq)
    for k in COUNTERS:
        assert ms[k] == gs[k], (name, "frame", k, ms[k], gs[k])
    ps, ms = {}, {}
    cam.render_rows(world, 2, 5, first_sample=3, stats=ps)
    m = cam.render_moments(world, first_sample=3, row_first=2, row_step=5, stats=ms)
    assert _same(m.sq, S[3][1][2::5])
    for k in COUNTERS:
        assert ms[k] == ps[k], (name, "rows", k, ms[k], ps[k])
    xs, ys = _lists(cam.c.image_width, cam.c.image_height)["130"]
    ps, ms = {}, {}
    cam.render_pixels(world, xs, ys, stats=ps)
    lsums, lsq = cam.render_pixels_moments(world, xs, ys, stats=ms)
    assert _same(lsq, want_sq[ys, xs])
    for k in COUNTERS:
        assert ms[k] == ps[k], (name, "list", k, ms[k], ps[k])
    # the device form with stats is synchronous and counts too
    d_s = torch.zeros((cam.c.image_height, cam.c.image_width, 3), dtype=torch.float64, device="cuda:0")
    d_q = torch.zeros_like(d_s)
    ds = {}
    cam.render_moments_device(world, d_s.data_ptr(), d_q.data_ptr(), stats=ds)
    for k in COUNTERS:
        assert ds[k] == gs[k], (name, "device form", k, ds[k], gs[k])
    assert _same(d_q.cpu().numpy(), want_sq)


@pytest.mark.parametrize("name", SCENES)
def test_a_moments_render_leaves_no_residue(rl, name):
    """Case 8: render, render_moments (every route), render on one scene object: the two plain frames are byte-equal; a
    render_from_checkpoint after a moments render equals one made before it."""
    S = _setup(rl, name)
    world, cam = S["world"], S["cam"]
    before = cam.render(world)
    cp_before = cam.render_from_checkpoint(world, before)
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            _frame_device(rl, cam, world)
            cam.render_moments(world)
            cam.render_pixels_moments(world, *_shuffled(cam))
    finally:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True)
    after = cam.render(world)
    assert _same(before.data, after.data) and _same(after.data, S[0][0])
    cp_after = cam.render_from_checkpoint(world, after)
    assert cp_after.samples == cp_before.samples == 2 * SPP and _same(cp_before.data, cp_after.data)


@pytest.mark.parametrize("name", SCENES)
def test_merged_moments_add(rl, name):
    """Case 9: a 3-sample render merged with the first_sample = 3 render of 3 samples holds sums1 + sums2 and sq1 + sq2, 6 samples."""
    S = _setup(rl, name)
    world, cam = S["world"], S["cam"]
    a = cam.render_moments(world)
    b = cam.render_moments(world, first_sample=3)
    m = a.merge(b)
    assert m.samples == 6
    assert _same(m.sums, S[0][0] + S[3][0]) and _same(m.sq, S[0][1] + S[3][1])
    cv = m.canvas()
    assert (cv.samples, cv.width, cv.height) == (6, cam.c.image_width, cam.c.image_height)
    assert _same(cv.data, cam.render_from_checkpoint(world, cam.render(world)).data)
    v = m.variance_of_mean()
    assert v.shape == m.sums.shape and (v >= 0).all() and v.any()


def test_null_buffers_empty_list_and_the_other_family(rl):
    api = rl.api
    lib = api.render_lib()
    S = _setup(rl, "golden_test_scene")
    world, cam = S["world"], S["cam"]
    rw = rl.RtcWorld.test_csg_scene(24, 16)
    n = cam.c.image_width * cam.c.image_height * 3
    a, b = np.full(n, np.nan), np.full(n, np.nan)
    c = C.byref(cam.c)
    xs = np.zeros(2, dtype=np.uint32)
    assert lib.rl_rtiow_render_moments_rows(world.device(), c, 0, 0, 1, a.ctypes.data, None, None) == api.RL_E_INVALID  # no second buffer
    assert lib.rl_rtiow_render_moments_rows(world.device(), c, 0, 0, 1, None, b.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_moments_rows(world.device(), c, 0, 0, 0, a.ctypes.data, b.ctypes.data, None) == api.RL_E_INVALID  # row_step 0
    assert lib.rl_rtiow_render_moments_device(world.device(), c, 0, 0, 1, a.ctypes.data, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_moments_rows(rw.device(), c, 0, 0, 1, a.ctypes.data, b.ctypes.data, None) == api.RL_E_INVALID  # an RTC scene
    assert lib.rl_rtiow_render_pixels_moments(world.device(), c, 0, xs.ctypes.data, xs.ctypes.data, 2, a.ctypes.data, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_pixels_moments(world.device(), c, 0, xs.ctypes.data, None, 2, a.ctypes.data, b.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_pixels_moments_device(world.device(), c, 0, xs.ctypes.data, xs.ctypes.data, 2, a.ctypes.data, None, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_pixels_moments_device(world.device(), c, 0, xs.ctypes.data, xs.ctypes.data, 0xFFFF0000, a.ctypes.data, b.ctypes.data, None,
                                                     None) == api.RL_E_INVALID
    assert b"image too large" in lib.rl_last_error()
    st = api.Stats()
    st.rays = 77
    assert lib.rl_rtiow_render_pixels_moments(world.device(), c, 0, None, None, 0, a.ctypes.data, b.ctypes.data, C.byref(st)) == api.RL_OK and st.rays == 0
    st.rays = 77  # row_first past the last row: RL_OK, nothing touched, the stats zeroed
    assert lib.rl_rtiow_render_moments_rows(world.device(), c, 0, cam.c.image_height, 1, a.ctypes.data, b.ctypes.data, C.byref(st)) == api.RL_OK and st.rays == 0
    assert np.isnan(a).all() and np.isnan(b).all()
    sums, sq = cam.render_pixels_moments(world, [], [])
    assert sums.shape == (0, 3) and sq.shape == (0, 3)


def test_cpp_mirror_renders_moments(rl):
    H = rl.api.host_lib()
    H.rlh_render_moments_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
    S = _setup(rl, "golden_test_scene")
    cam = S["cam"]
    frame, want_sq, _ = S[0]
    W, Hh = cam.c.image_width, cam.c.image_height
    sums, sq = np.zeros((Hh, W, 3)), np.zeros((Hh, W, 3))
    # the mirror's golden_test_scene at the test's width and samples, but its own max_depth: compare with a camera of that depth
    world = rl.World.golden_test_scene()
    cam2 = rl.Camera(dataclasses.replace(world.params, image_width=W, samples_per_pixel=SPP))
    want = cam2.render_moments(world)
    assert H.rlh_render_moments_probe(W, SPP, None, None, 0, sums.ctypes.data, sq.ctypes.data) == 0, H.rlh_last_error()
    assert _same(sums, want.sums) and _same(sq, want.sq)
    xs, ys = _lists(W, Hh)["65"]
    x32, y32 = xs.astype(np.uint32), ys.astype(np.uint32)
    lsums, lsq = np.zeros((65, 3)), np.zeros((65, 3))
    assert H.rlh_render_moments_probe(W, SPP, x32.ctypes.data, y32.ctypes.data, 65, lsums.ctypes.data, lsq.ctypes.data) == 0, H.rlh_last_error()
    assert _same(lsums, want.sums[ys, xs]) and _same(lsq, want.sq[ys, xs])
