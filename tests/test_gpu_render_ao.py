"""GPU tier: the ambient-occlusion renders (rl.render_ao* / rl.render_pixels_ao*; include/rl_render.h "Ambient-occlusion renders",
DESIGN.md §3.20).  Both outputs are integers, so every comparison is of bytes:
  1. against the host composition get_rays -> hit_rays -> K x (scatter_rays on a Lambertian -> normalise -> occluded_rays), counters included;
  2. counter-free and counting calls, and the reference-order route with the fast traversal switched off;
  3. against the definition in Python on the CPU oracle (tests/ao_model.py);
  4. the two known answers of tests/test_ao_model.py, on the device;
  5. row shards, pixel lists, continued calls, one output of the two, a media scene;
  6. the hand-over of ambient rays from the any-hit walk to the reference's fold does happen."""
import ctypes as C
import dataclasses
import os

import ao_model
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
INF = float("inf")
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
FLAT, LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT, ISOTROPIC = range(6)  # include/rl_render.h RL_MAT_*
W0, H0 = 37, 19  # 703 pixels: not a multiple of a wave or of a workgroup; non-square, so x*W + y is not y*W + x
CASES = [(3, 5, INF), (2, 1, 0.5), (1, 16, 2.0)]  # (S, K, R)
SCENES = ["golden_test_scene", "random_world", "cornell_box", "stress60"]


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


def _random_world(rl):
    """A ground sphere and 40 small spheres of Lambertian, Metal, Dielectric, DiffuseLight and Flat materials, every third one moving."""
    rng = np.random.default_rng(2026)

    def build(b):
        mats = [b.lambertian(b.solid((0.6, 0.5, 0.4))), b.metal((0.8, 0.8, 0.7), 0.3), b.dielectric(1.5), b.diffuse_light(b.solid((4.0, 4.0, 4.0))), b.flat()]
        objs = [b.sphere((0.0, -100.0, 0.0), 100.0, mats[0])]
        for i in range(40):
            c = np.array([rng.uniform(-3.0, 3.0), rng.uniform(0.2, 1.6), rng.uniform(-3.0, 3.0)])
            c2 = c + (0.0, rng.uniform(0.1, 0.5), 0.0) if i % 3 == 0 else None
            objs.append(b.sphere(c, rng.uniform(0.15, 0.5), mats[i % len(mats)], center2=c2))
        return b.bvh(objs)
    w = rl.World.build(build)
    w.params = rl.CameraParams(vfov=40.0, lookfrom=(6.0, 2.5, 5.0), lookat=(0.0, 0.5, 0.0), defocus_angle=0.6, focus_dist=8.0, seed=11)
    return w


_worlds = {}


def _world(rl, golden, name):
    if name not in _worlds:
        if name == "golden_test_scene":
            w = rl.World.golden_test_scene()
        elif name == "random_world":
            w = _random_world(rl)
        elif name == "stress60":  # the tree is larger than the LDS top; a mesh under a transform
            w = rl.World.stress_scene(60, 1, golden("spot_triangulated.obj.gz"), _spot_texture())
        else:
            w = rl.World.example_scene(name)
        _worlds[name] = w
    return _worlds[name]


def _camera(rl, world, S, W=W0, H=H0):
    p = dataclasses.replace(world.params, image_width=W, aspect_ratio=W / (H + 0.5), samples_per_pixel=S)  # height = floor(W / aspect) = H
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (W, H)
    return cam


def _pixels(cam):
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
    return x, y


def _compose(rl, world, cam, px, py, K, R, F=0):
    """The host composition -> (open [n], hits [n], the summed counters of its counting calls with rng_words = the summed final word
    positions of the cursors)."""
    api = rl.api
    W, H, S = cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel
    px, py = np.asarray(px, dtype=np.uint64), np.asarray(py, dtype=np.uint64)
    mats = world.materials()
    lam = int(np.nonzero(mats["kind"] == LAMBERTIAN)[0][0])  # the index of a Lambertian of the scene
    op, hc = np.zeros(px.shape[0], dtype=np.uint32), np.zeros(px.shape[0], dtype=np.uint32)
    tot = dict.fromkeys(COUNTERS, 0)

    def add(st):
        for k in COUNTERS:
            if k != "rng_words":
                tot[k] += st[k]
    for s in range(F, F + S):
        cur = api.pack_cursors(np.uint64(s) * np.uint64(W * H) + px * np.uint64(W) + py, 0)
        rays, cur = cam.get_rays(px, py, cur)
        st = {}
        hits = world.hit_rays(rays["origin"], rays["dir"], times=rays["time"], tmin=1e-10, stats=st, allow_degenerate=True)
        add(st)
        idx = np.nonzero(hits["hit"] != 0)[0]
        hc[idx] += 1
        tot["rng_words"] += int(cur["word_pos"][hits["hit"] == 0].sum(dtype=np.uint64))
        if idx.size == 0:
            continue
        h, r, c = hits[idx].copy(), rays[idx].copy(), cur[idx].copy()
        h["material"] = lam
        for _ in range(K):
            sc, c = world.scatter_rays(r, h, c, cam.params.seed)
            d = sc["scattered"]["dir"]
            dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
            a = d * (1.0 / np.sqrt(dx * dx + dy * dy + dz * dz))[:, None]
            st = {}
            occ = rl.occluded_rays(world, h["p"], a, times=r["time"], tmin=1e-10, tmax=R, stats=st, allow_degenerate=True)
            add(st)
            op[idx] += (~occ).astype(np.uint32)
        tot["rng_words"] += int(c["word_pos"].sum(dtype=np.uint64))
    return op, hc, tot


_frames = {}


def _yardstick(rl, golden, name, case):
    """The composition's W0 x H0 frame of `name` for case = (S, K, R), computed once and shared."""
    if (name, case) not in _frames:
        world = _world(rl, golden, name)
        S, K, R = case
        cam = _camera(rl, world, S)
        op, hc, tot = _compose(rl, world, cam, *_pixels(cam), K, R)
        op.setflags(write=False), hc.setflags(write=False)
        _frames[(name, case)] = (op.reshape(H0, W0), hc.reshape(H0, W0), tot)
    return _frames[(name, case)]


def _free_frame(rl, world, cam, K, R, F=0):
    """The whole frame through a counter-free call (the host list form without stats) -> (AmbientOcclusion [H, W], last_query())."""
    x, y = _pixels(cam)
    ao = rl.render_pixels_ao(cam, world, x, y, K, R, first_sample=F, allow_degenerate=True)
    q = rl.api.last_query()
    H, W = cam.c.image_height, cam.c.image_width
    return rl.AmbientOcclusion(ao.open.reshape(H, W), ao.hits.reshape(H, W), K), q


def _same(got, want):
    return got is not None and got.dtype == np.uint32 and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


# ----------------------------------------------------------------------------- 1. + 2. composition, counters, routes
def test_the_yardstick_itself_sees_hits_misses_and_both_answers(rl, golden):
    """Asserted on the composition alone, before any result of the feature is looked at."""
    for name in SCENES:
        for case in CASES:
            S, K, R = case
            op, hc, tot = _yardstick(rl, golden, name, case)
            assert hc.sum() > 0 and tot["rays"] == S * W0 * H0 + K * int(hc.sum()), (name, case)
            assert (op <= K * hc).all()
    missed = full = 0
    for name in SCENES:
        op, hc, _ = _yardstick(rl, golden, name, CASES[0])
        print(name, "pixels without a hit", int((hc == 0).sum()), "with 3", int((hc == 3).sum()), "open", int(op.sum()), "of", 5 * int(hc.sum()))
        missed, full = missed + int((hc == 0).sum()), full + int((hc == 3).sum())
    assert missed > 0 and full > 0  # the set has pixels that miss the scene and pixels that are covered
    op, hc, _ = _yardstick(rl, golden, "golden_test_scene", CASES[0])
    assert 0 < op.sum() < 5 * hc.sum()  # some ambient rays are occluded, some are not
    assert (_yardstick(rl, golden, "random_world", CASES[0])[0] != _yardstick(rl, golden, "random_world", CASES[2])[0]).any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-K%d-R%s" % c)
@pytest.mark.parametrize("name", SCENES)
def test_frames_are_the_compositions_bytes_on_every_route(rl, golden, name, case):
    api = rl.api
    S, K, R = case
    world = _world(rl, golden, name)
    cam = _camera(rl, world, S)
    op, hc, tot = _yardstick(rl, golden, name, case)
    st = {}
    counting = rl.render_ao(cam, world, K, R, stats=st, allow_degenerate=True)
    assert api.last_query() == {"kernel": "ao_reference", "retraced": 0}
    assert _same(counting.open, op) and _same(counting.hits, hc), (name, case, np.argwhere(counting.open != op)[:8])
    assert counting.ao_rays == K
    # the counters and rng_words are the composition's sums
    assert {k: st[k] for k in COUNTERS} == tot, (name, case, st, tot)
    assert st["rays"] == S * W0 * H0 + K * int(hc.sum())
    for on, route in ((True, "ao_fast"), (False, "ao_reference")):
        api.set_fast_traversal(on)
        try:
            free, q = _free_frame(rl, world, cam, K, R)
        finally:
            api.set_fast_traversal(True)
        assert q["kernel"] == route, (name, case, q)
        assert _same(free.open, op) and _same(free.hits, hc), (name, case, route, np.argwhere(free.open != op)[:8])
        if not on:
            assert q["retraced"] == 0
    # the counting list form too
    x, y = _pixels(cam)
    st2 = {}
    lst = rl.render_pixels_ao(cam, world, x, y, K, R, stats=st2, allow_degenerate=True)
    assert api.last_query()["kernel"] == "ao_reference"
    assert _same(lst.open.reshape(H0, W0), op) and _same(lst.hits.reshape(H0, W0), hc)
    assert {k: st2[k] for k in COUNTERS} == tot


# ----------------------------------------------------------------------------- 3. the oracle
@pytest.mark.parametrize("name", ["golden_test_scene", "cornell_box"])
def test_frames_equal_the_definition_on_the_cpu_oracle(rl, oracle, golden, name):
    world = _world(rl, golden, name)
    cam = _camera(rl, world, 2, 8, 6)
    K, R = 3, (INF if name == "golden_test_scene" else 150.0)  # cornell_box is 555 across
    op, hc, words = ao_model.frame(oracle, world.desc, cam.c, K, R)
    assert hc.sum() > 0 and 0 < op.sum() < K * hc.sum(), (name, op, hc)
    st = {}
    got = rl.render_ao(cam, world, K, R, stats=st)
    assert _same(got.open, op) and _same(got.hits, hc), (name, got.open, op)
    assert st["rng_words"] == words and st["rays"] == 2 * 48 + K * int(hc.sum())
    free, q = _free_frame(rl, world, cam, K, R)
    assert q["kernel"] == "ao_fast" and _same(free.open, op) and _same(free.hits, hc), name


# ----------------------------------------------------------------------------- 4. known answers
def test_known_answers_on_the_device(rl):
    K = 4
    cases = ao_model.known_answer_cases(rl)
    world, cam = cases["lone_sphere"]
    for ao in (rl.render_ao(cam, world, K, INF), _free_frame(rl, world, cam, K, INF)[0]):
        assert 0 < ao.hits.sum() < 2 * 12 * 8
        assert _same(ao.open, K * ao.hits), (ao.open, ao.hits)  # a convex body occludes none of its own ambient rays
        assert (ao.visibility(miss=0.5)[ao.hits == 0] == 0.5).all() and (ao.visibility()[ao.hits > 0] == 1.0).all()
    world, cam = cases["inside"]
    for ao in (rl.render_ao(cam, world, K, INF), _free_frame(rl, world, cam, K, INF)[0]):
        assert _same(ao.hits, np.full((8, 12), 2, dtype=np.uint32)) and not ao.open.any()  # closed in
        assert not ao.visibility().any()


# ----------------------------------------------------------------------------- 5. shapes
def test_row_shards_lists_continued_calls_and_one_output(rl, golden):
    name, case = "random_world", CASES[0]
    S, K, R = case
    world = _world(rl, golden, name)
    cam = _camera(rl, world, S)
    op, hc, _ = _yardstick(rl, golden, name, case)
    for first, step in ((0, 1), (1, 3), (2, 3)):
        sh = rl.render_ao(cam, world, K, R, row_first=first, row_step=step, allow_degenerate=True)
        assert _same(sh.open, op[first::step]) and _same(sh.hits, hc[first::step]), (first, step)
    # a shuffled list with duplicates, counter-free and counting
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, W0, 900), rng.integers(0, H0, 900)
    assert np.unique(x * 100 + y).size < 900
    for st in (None, {}):
        lst = rl.render_pixels_ao(cam, world, x, y, K, R, stats=st, allow_degenerate=True)
        assert _same(lst.open, op[y, x]) and _same(lst.hits, hc[y, x])
    empty = rl.render_pixels_ao(cam, world, [], [], K, R)
    assert empty.open.shape == (0,)
    with pytest.raises(rl.RLError) as e:  # the host form refuses a pixel outside the image
        rl.render_pixels_ao(cam, world, [0, W0], [0, 0], K, R)
    assert e.value.code == rl.api.RL_E_INVALID
    # (F = 0, S = 2) + (F = 2, S = 1) == (F = 0, S = 3), exactly
    two, one = _camera(rl, world, 2), _camera(rl, world, 1)
    a = rl.render_ao(two, world, K, R, first_sample=0, allow_degenerate=True)
    b = rl.render_ao(one, world, K, R, first_sample=2, allow_degenerate=True)
    m = a.merge(b)
    assert _same(m.open, op) and _same(m.hits, hc)
    fa, fb = _free_frame(rl, world, two, K, R, 0)[0], _free_frame(rl, world, one, K, R, 2)[0]
    assert _same(fa.merge(fb).open, op) and _same(fa.open, a.open) and _same(fb.hits, b.hits)
    # one output: the same bits, the other not produced
    for want in (("open",), ("hits",)):
        part = rl.render_ao(cam, world, K, R, want=want, allow_degenerate=True)
        lpart = rl.render_pixels_ao(cam, world, x, y, K, R, want=want, allow_degenerate=True)
        if want == ("open",):
            assert _same(part.open, op) and part.hits is None and _same(lpart.open, op[y, x]) and lpart.hits is None
        else:
            assert _same(part.hits, hc) and part.open is None and _same(lpart.hits, hc[y, x]) and lpart.open is None


def test_device_forms_an_outside_pixel_and_an_untouched_buffer(rl, golden):
    import torch
    name, case = "random_world", CASES[0]
    S, K, R = case
    world = _world(rl, golden, name)
    cam = _camera(rl, world, S)
    op, hc, _ = _yardstick(rl, golden, name, case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda:0")
    host = lambda t: t.cpu().numpy().view(np.uint32)
    stream = torch.cuda.Stream()
    # the frame, asynchronous and counter-free on a side stream; then with stats
    d_open, d_hits = dev(np.full(W0 * H0, 77, dtype=np.uint32)), dev(np.full(W0 * H0, 77, dtype=np.uint32))
    rl.render_ao_device(cam, world, K, R, stream=stream.cuda_stream, d_open=d_open.data_ptr(), d_hits=d_hits.data_ptr())
    stream.synchronize()
    status = rl.api.render_status(world, allow_degenerate=True)
    assert _same(host(d_open).reshape(H0, W0), op) and _same(host(d_hits).reshape(H0, W0), hc)
    assert status["rays"] == S * W0 * H0 + K * int(hc.sum())
    # one output: the other buffer is untouched
    d_open.fill_(77), d_hits.fill_(77)
    rl.render_ao_device(cam, world, K, R, d_hits=d_hits.data_ptr(), stats={}, allow_degenerate=True)
    assert _same(host(d_hits).reshape(H0, W0), hc) and (host(d_open) == 77).all()
    d_hits.fill_(77)
    rl.render_ao_device(cam, world, K, R, row_first=1, row_step=3, d_open=d_open.data_ptr(), stats={}, allow_degenerate=True)
    n = op[1::3].size
    assert _same(host(d_open)[:n].reshape(-1, W0), op[1::3]) and (host(d_open)[n:] == 77).all() and (host(d_hits) == 77).all()
    # the device list: shuffled, duplicates, one pixel outside the image -> zeros there
    rng = np.random.default_rng(8)
    x, y = rng.integers(0, W0, 300).astype(np.uint32), rng.integers(0, H0, 300).astype(np.uint32)
    x[0], y[0] = x[1], y[1]
    x[150], y[150] = W0, 3
    inside = np.arange(300) != 150
    d_x, d_y = dev(x), dev(y)
    for st in (None, {}):
        d_o, d_h = dev(np.full(302, 77, dtype=np.uint32)), dev(np.full(302, 77, dtype=np.uint32))
        rl.render_pixels_ao_device(cam, world, d_x.data_ptr(), d_y.data_ptr(), 300, K, R, d_open=d_o.data_ptr(), d_hits=d_h.data_ptr(), stats=st,
                                   allow_degenerate=True)
        torch.cuda.synchronize()
        if st is None:
            rl.api.render_status(world, allow_degenerate=True)
        go, gh = host(d_o), host(d_h)
        assert _same(go[:300][inside], op[y[inside], x[inside]]) and _same(gh[:300][inside], hc[y[inside], x[inside]])
        assert go[150] == 0 and gh[150] == 0 and (go[300:] == 77).all() and (gh[300:] == 77).all()


def test_errors_with_a_device(rl, golden):
    api = rl.api
    world = _world(rl, golden, "golden_test_scene")
    cam = _camera(rl, world, 2)
    smoke = rl.World.example_scene("cornell_smoke")
    scam = _camera(rl, smoke, 1)
    for call in (lambda: rl.render_ao(scam, smoke, 2, 100.0), lambda: rl.render_pixels_ao(scam, smoke, [0], [0], 2, 100.0),
                 lambda: rl.render_pixels_ao(scam, smoke, [0], [0], 2, 100.0, stats={})):
        with pytest.raises(rl.RLError) as e:  # a scene with ConstantMedium objects: there is no seeded any-hit
            call()
        assert e.value.code == api.RL_E_UNSUPPORTED and "ConstantMedium" in str(e.value)
    for k, r in ((0, 1.0), (4, 0.0), (4, float("nan")), (4, -2.0), (1 << 31, 1.0)):  # S = 2: K = 2^31 is S K = 2^32
        with pytest.raises(rl.RLError) as e:
            rl.render_ao(cam, world, k, r)
        assert e.value.code == api.RL_E_INVALID, (k, r)
    # the plain renders' rules, on the C ABI: row_step 0, a NULL camera, an RTC scene; outputs untouched
    lib = api.render_lib()
    buf = np.full(W0 * H0, 7, dtype=np.uint32)
    p = buf.ctypes.data
    assert lib.rl_rtiow_render_ao_rows(world.device(), C.byref(cam.c), 0, 0, 0, 4, 1.0, p, p, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_ao_rows(world.device(), None, 0, 0, 1, 4, 1.0, p, p, None) == api.RL_E_INVALID
    rtc = rl.RtcWorld.test_mirror_scene(30, 20)
    assert lib.rl_rtiow_render_ao_rows(rtc.device(), C.byref(cam.c), 0, 0, 1, 4, 1.0, p, p, None) == api.RL_E_INVALID
    assert (buf == 7).all()
    st = {"rays": 5}
    past = rl.render_ao(cam, world, 4, 1.0, row_first=H0, stats=st)  # a row past the frame: no rows, zeroed stats
    assert past.open.shape == (0, W0) and st["rays"] == 0


def test_cpp_mirror_renders_ao(rl, golden):
    H = rl.api.host_lib()
    H.rlh_ao_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p]
    H.rlh_ao_probe.restype = C.c_int
    world = _world(rl, golden, "golden_test_scene")
    cam = rl.Camera(dataclasses.replace(world.params, image_width=20, samples_per_pixel=2))
    n = cam.c.image_width * cam.c.image_height
    op, hc = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    assert H.rlh_ao_probe(20, 2, 1, 3, 0.75, op.ctypes.data, hc.ctypes.data) == 0, H.rlh_last_error()
    want = rl.render_ao(cam, world, 3, 0.75, first_sample=1)
    assert _same(op, want.open.reshape(-1)) and _same(hc, want.hits.reshape(-1)) and hc.sum() > 0


# ----------------------------------------------------------------------------- 6. the hand-over to the fold is exercised
def test_the_any_hit_walk_hands_ambient_rays_to_the_fold(rl, golden):
    """The slow-trace counter of a counter-free call counts the camera rays AND the ambient rays its walks re-traced.  The camera rays'
    share is what a counter-free feature render of the same camera reports (the same function walks them); the rest are ambient rays."""
    world = _world(rl, golden, "stress60")
    S, K, R = CASES[0]
    cam = _camera(rl, world, S)
    op, hc, _ = _yardstick(rl, golden, "stress60", CASES[0])
    free, q = _free_frame(rl, world, cam, K, R)
    assert q["kernel"] == "ao_fast" and _same(free.open, op)
    x, y = _pixels(cam)
    cam.render_pixels_features(world, x, y, want=("hit_count",), allow_degenerate=True)
    fq = rl.api.last_query()
    assert fq["kernel"] == "features_fast"
    ambient = q["retraced"] - fq["retraced"]
    print("stress60 37x19 S=3 K=5 R=inf: ambient rays", K * int(hc.sum()), "re-traced", ambient, "; camera rays", S * W0 * H0, "re-traced", fq["retraced"])
    assert ambient > 0, (q, fq)
    assert ambient < K * int(hc.sum()), (q, fq)  # and the walk decides rays by itself: the fold does not do all the work
