"""GPU tier: the direct-lighting renders (rl.render_direct* / rl.render_pixels_direct*; include/rl_render.h "Direct-lighting renders",
DESIGN.md §3.21).  Every comparison is of bytes:
  1. against the host composition get_rays -> hit_rays -> the light points' draws from the oracle's ChaCha script at the cursor get_rays
     returned -> the definition's arithmetic in numpy -> occluded_rays(tmax = T), counters included; counting and counter-free calls, and the
     reference-order route with the fast traversal switched off;
  2. against the definition in Python on the CPU oracle (tests/direct_model.py);
  3. the known answers of tests/test_direct_model.py, on the device;
  4. row shards, pixel lists (also longer than one launch's lanes), every subset of the outputs, continued calls, device forms, a media
     scene, the C++ mirror;
  5. the hand-over of shadow segments from the any-hit walk to the reference's fold does happen."""
import dataclasses
import itertools
import os

import ao_model
import direct_model as dm
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
W0, H0 = 37, 19  # 703 pixels: not a multiple of a wave or of a workgroup; non-square, so x*W + y is not y*W + x
CASES = [(3, 2), (1, 1), (2, 5)]  # (S, K)
SCENES = ["cornell_box", "golden_test_scene", "random_world", "stress60"]
T = 1.0 - 1e-6
# cornell_box: its own light (cornell_box.rs), which is geometry of the scene at t = 1 of every segment; the others: two lights above the scene,
# one level and one tilted, of different colours
LIGHTS = {
    "cornell_box": [((343.0, 554.0, 332.0), (-130.0, 0.0, 0.0), (0.0, 0.0, -105.0), 15.0)],
    "golden_test_scene": [((-1.0, 3.0, -2.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (4.0, 4.0, 4.0)), ((2.0, 2.5, 0.0), (0.0, 0.0, -2.0), (1.0, 1.0, 0.0), (3.0, 2.0, 1.0))],
    "random_world": [((-2.0, 5.0, -2.0), (4.0, 0.0, 0.0), (0.0, 0.0, 4.0), (4.0, 4.0, 4.0)), ((4.0, 4.0, -1.0), (0.0, 0.0, 2.0), (1.0, 1.5, 0.0), (3.0, 2.0, 1.0))],
    "stress60": [((-6.0, 20.0, -6.0), (12.0, 0.0, 0.0), (0.0, 0.0, 12.0), (4.0, 4.0, 4.0)), ((14.0, 6.0, -4.0), (0.0, 0.0, 8.0), (2.0, 3.0, 0.0), (3.0, 2.0, 1.0))],
}
# a lamp 0.05 under the pole of stress60's ground sphere (test_the_any_hit_walk_hands_segments_to_the_fold says why)
BURIED_LAMP = ((-0.3, -0.05, -0.3), (0.6, 0.0, 0.0), (0.0, 0.0, 0.6), (4.0, 4.0, 4.0))


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
    """The AO suite's: a ground sphere and 40 small spheres of five materials, every third one MOVING (the segments inherit the ray's time)."""
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


def _compose(rl, oracle, world, cam, px, py, lights, K, seg_tmax, F=0):
    """The host composition over DISTINCT pixels -> (direct [n, 3], unshadowed [n, 3], hits [n], the summed counters of its counting calls
    with rng_words = the cursors' word positions behind get_ray + 4 per light point, segments traced)."""
    api = rl.api
    W, H, S = cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel
    px, py = np.asarray(px, dtype=np.uint64), np.asarray(py, dtype=np.uint64)
    L = rl.pack_lights(lights)
    n = px.shape[0]
    di, un, hc = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=np.uint32)
    tot = dict.fromkeys(COUNTERS, 0)
    traced = 0

    def add(st):
        for k in COUNTERS:
            if k != "rng_words":
                tot[k] += st[k]
    for s in range(F, F + S):
        streams = np.uint64(s) * np.uint64(W * H) + px * np.uint64(W) + py
        rays, cur = cam.get_rays(px, py, api.pack_cursors(streams, 0))
        st = {}
        hits = world.hit_rays(rays["origin"], rays["dir"], times=rays["time"], tmin=1e-10, stats=st, allow_degenerate=True)
        add(st)
        idx = np.nonzero(hits["hit"] != 0)[0]
        hc[idx] += 1
        tot["rng_words"] += int(cur["word_pos"].sum(dtype=np.uint64)) + 4 * L.shape[0] * K * idx.size
        if idx.size == 0:
            continue
        # the light points' draws: the sample's own stream, from the word get_ray stopped at (every draw so far took one u64 = two words)
        ab = np.zeros((idx.size, L.shape[0], K, 2))
        for j, i in enumerate(idx):
            rng = ao_model.Stream(oracle, cam.params.seed, int(streams[i]))
            assert int(cur["word_pos"][i]) % 2 == 0
            rng.i = int(cur["word_pos"][i]) // 2
            ab[j] = np.array([rng.f64() for _ in range(2 * L.shape[0] * K)]).reshape(L.shape[0], K, 2)
        p, nrm, time = hits["p"][idx], hits["normal"][idx], rays["time"][idx]
        for l in range(L.shape[0]):
            Q, u, v, E = L[l, 0:3], L[l, 3:6], L[l, 6:9], L[l, 9:12]
            nl = np.array(dm.cross([float(c) for c in u], [float(c) for c in v]))
            for k in range(K):
                a, b = ab[:, l, k, 0:1], ab[:, l, k, 1:2]
                yl = (Q + u * a) + v * b
                d = yl - p
                d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                cs = nrm[:, 0] * d[:, 0] + nrm[:, 1] * d[:, 1] + nrm[:, 2] * d[:, 2]
                cl = np.abs(nl[0] * d[:, 0] + nl[1] * d[:, 1] + nl[2] * d[:, 2])
                ok = np.nonzero((cs > 0.0) & (cl > 0.0) & (d2 > 0.0))[0]
                if ok.size == 0:
                    continue
                g = (cs[ok] * cl[ok]) / (d2[ok] * d2[ok])
                st = {}
                occ = rl.occluded_rays(world, p[ok], d[ok], times=time[ok], tmin=1e-10, tmax=seg_tmax, stats=st, allow_degenerate=True)
                add(st)
                traced += ok.size
                e = E[None, :] * g[:, None]
                un[idx[ok]] = un[idx[ok]] + e
                lit = ok[~occ]
                di[idx[lit]] = di[idx[lit]] + e[~occ]
    return di, un, hc, tot, traced


_frames = {}


def _yardstick(rl, oracle, golden, name, case):
    """The composition's W0 x H0 frame of `name` for case = (S, K), computed once and shared."""
    if (name, case) not in _frames:
        world = _world(rl, golden, name)
        S, K = case
        cam = _camera(rl, world, S)
        di, un, hc, tot, traced = _compose(rl, oracle, world, cam, *_pixels(cam), LIGHTS[name], K, T)
        for a in (di, un, hc):
            a.setflags(write=False)
        _frames[(name, case)] = (di.reshape(H0, W0, 3), un.reshape(H0, W0, 3), hc.reshape(H0, W0), tot, traced)
    return _frames[(name, case)]


def _free_frame(rl, world, cam, lights, K, F=0, want=None, seg_tmax=T):
    """The whole frame through a counter-free call (the host list form without stats) -> (DirectLight [H, W(, 3)], last_query())."""
    x, y = _pixels(cam)
    dl = rl.render_pixels_direct(cam, world, x, y, lights, K, seg_tmax, first_sample=F, want=want, allow_degenerate=True)
    q = rl.api.last_query()
    H, W = cam.c.image_height, cam.c.image_width
    r3 = lambda a: None if a is None else a.reshape(H, W, 3)
    return rl.DirectLight(r3(dl.direct), r3(dl.unshadowed), None if dl.hits is None else dl.hits.reshape(H, W), K), q


def _same(got, want):
    return got is not None and got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


def _same3(got, di, un, hc):
    return _same(got.direct, di) and _same(got.unshadowed, un) and _same(got.hits, hc)


# ----------------------------------------------------------------------------- 1. composition, counters, routes
def test_the_yardstick_itself_sees_light_shadow_and_skipped_samples(rl, oracle, golden):
    """Asserted on the composition alone, before any result of the feature is looked at."""
    for name in SCENES:
        for case in CASES:
            S, K = case
            di, un, hc, tot, traced = _yardstick(rl, oracle, golden, name, case)
            nl = len(LIGHTS[name])
            assert hc.sum() > 0 and tot["rays"] == S * W0 * H0 + traced and traced <= nl * K * int(hc.sum()), (name, case)
            assert (di <= un).all() and (un >= 0.0).all() and not un[hc == 0].any()
        di, un, hc, tot, traced = _yardstick(rl, oracle, golden, name, CASES[0])
        print(name, "pixels without a hit", int((hc == 0).sum()), "segments", traced, "of", len(LIGHTS[name]) * 2 * int(hc.sum()), "lit pixels", int((di > 0).any(-1).sum()),
              "shadowed or partly", int((di < un).any(-1).sum()))
        assert 0 < traced < len(LIGHTS[name]) * 2 * int(hc.sum())  # some light samples are skipped (faces away), some are traced
        assert (di > 0).any() and (di < un).any()                    # some segments are free, some are blocked
    assert sum(int((_yardstick(rl, oracle, golden, n, CASES[0])[2] == 0).sum()) for n in SCENES) > 0  # pixels that miss the scene


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-K%d" % c)
@pytest.mark.parametrize("name", SCENES)
def test_frames_are_the_compositions_bytes_on_every_route(rl, oracle, golden, name, case):
    api = rl.api
    S, K = case
    world = _world(rl, golden, name)
    cam = _camera(rl, world, S)
    lights = LIGHTS[name]
    di, un, hc, tot, traced = _yardstick(rl, oracle, golden, name, case)
    st = {}
    counting = rl.render_direct(cam, world, lights, K, T, stats=st, allow_degenerate=True)
    assert api.last_query() == {"kernel": "direct_reference", "retraced": 0}
    assert _same3(counting, di, un, hc), (name, case, np.argwhere(counting.direct != di)[:8], np.argwhere(counting.unshadowed != un)[:8])
    assert counting.light_samples == K
    # the counters and rng_words are the composition's sums
    assert {k: st[k] for k in COUNTERS} == tot, (name, case, st, tot)
    assert st["rays"] == S * W0 * H0 + traced
    for on, route in ((True, "direct_fast"), (False, "direct_reference")):
        api.set_fast_traversal(on)
        try:
            free, q = _free_frame(rl, world, cam, lights, K)
        finally:
            api.set_fast_traversal(True)
        assert q["kernel"] == route, (name, case, q)
        assert _same3(free, di, un, hc), (name, case, route, np.argwhere(free.direct != di)[:8])
        if not on:
            assert q["retraced"] == 0
    # the counting list form too
    x, y = _pixels(cam)
    st2 = {}
    lst = rl.render_pixels_direct(cam, world, x, y, lights, K, T, stats=st2, allow_degenerate=True)
    assert api.last_query()["kernel"] == "direct_reference"
    assert _same(lst.direct.reshape(H0, W0, 3), di) and _same(lst.unshadowed.reshape(H0, W0, 3), un) and _same(lst.hits.reshape(H0, W0), hc)
    assert {k: st2[k] for k in COUNTERS} == tot


# ----------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("name", ["golden_test_scene", "cornell_box"])
def test_frames_equal_the_definition_on_the_cpu_oracle(rl, oracle, golden, name):
    world = _world(rl, golden, name)
    cam = _camera(rl, world, 2, 12, 8)
    K, lights = 3, LIGHTS[name]
    di, un, hc, words, traced = dm.frame(oracle, world.desc, cam.c, rl.pack_lights(lights), K, T)
    assert hc.sum() > 0 and (di > 0).any() and (di < un).any(), name
    st = {}
    got = rl.render_direct(cam, world, lights, K, T, stats=st)
    assert _same3(got, di, un, hc), (name, got.direct, di)
    assert st["rng_words"] == words and st["rays"] == 2 * 96 + traced
    free, q = _free_frame(rl, world, cam, lights, K)
    assert q["kernel"] == "direct_fast" and _same3(free, di, un, hc), name


# ----------------------------------------------------------------------------- 3. known answers
def test_known_answers_on_the_device(rl):
    K = 3
    cases = dm.known_answer_cases(rl)
    world, cam = cases["open"]
    opened = []
    for dl in (rl.render_direct(cam, world, dm.LIGHT_ABOVE, K), _free_frame(rl, world, cam, dm.LIGHT_ABOVE, K)[0]):
        assert 0 < (dl.hits > 0).sum() < 12 * 8
        assert _same(dl.direct, dl.unshadowed) and (dl.direct[dl.hits > 0] > 0.0).all() and not dl.direct[dl.hits == 0].any()  # nothing shadows
        assert (dl.shadow() == 1.0).all() and (dl.irradiance(miss=-1.0)[dl.hits == 0] == -1.0).all()
        opened.append(dl)
    assert _same3(opened[0], opened[1].direct, opened[1].unshadowed, opened[1].hits)
    world, cam = cases["blocked"]
    floor = opened[0].hits > 0
    for dl in (rl.render_direct(cam, world, dm.LIGHT_ABOVE, K), _free_frame(rl, world, cam, dm.LIGHT_ABOVE, K)[0]):
        assert not dl.direct.any() and (dl.unshadowed[floor] > 0.0).all()  # the blocker is between every floor point and the light
        assert dl.unshadowed[floor].tobytes() == opened[0].unshadowed[floor].tobytes() and (dl.hits >= opened[0].hits).all()
        assert not dl.shadow()[floor].any()
    world, cam = cases["open"]
    for stats in ({}, None):
        if stats is None:
            dl = _free_frame(rl, world, cam, dm.LIGHT_BELOW, K)[0]
        else:
            dl = rl.render_direct(cam, world, dm.LIGHT_BELOW, K, stats=stats)
            # nothing traced beyond the camera rays, and still 4 L K words per hit
            assert stats["rays"] == 2 * 96 and stats["rng_words"] == 6 * 2 * 96 + 4 * K * int(dl.hits.sum())
        assert not dl.direct.any() and not dl.unshadowed.any() and _same(dl.hits, opened[0].hits)  # the light is behind the floor


# ----------------------------------------------------------------------------- 4. launch forms
def test_row_shards_lists_and_every_subset_of_the_outputs(rl, oracle, golden):
    name, case = "random_world", CASES[0]
    S, K = case
    world, lights = _world(rl, golden, name), LIGHTS[name]
    cam = _camera(rl, world, S)
    di, un, hc, _, _ = _yardstick(rl, oracle, golden, name, case)
    for first, step in ((0, 1), (1, 3), (2, 3)):
        sh = rl.render_direct(cam, world, lights, K, T, row_first=first, row_step=step, allow_degenerate=True)
        assert _same3(sh, di[first::step], un[first::step], hc[first::step]), (first, step)
    # a shuffled list with duplicates, counter-free and counting
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, W0, 900), rng.integers(0, H0, 900)
    assert np.unique(x * 100 + y).size < 900
    for st in (None, {}):
        lst = rl.render_pixels_direct(cam, world, x, y, lights, K, T, stats=st, allow_degenerate=True)
        assert _same3(lst, di[y, x], un[y, x], hc[y, x])
    empty = rl.render_pixels_direct(cam, world, [], [], lights, K, T)
    assert empty.direct.shape == (0, 3) and empty.hits.shape == (0,)
    with pytest.raises(rl.RLError) as e:  # the host form refuses a pixel outside the image
        rl.render_pixels_direct(cam, world, [0, W0], [0, 0], lights, K, T)
    assert e.value.code == rl.api.RL_E_INVALID
    # every non-empty subset of the three outputs: the same bytes, the others not produced
    full = {"direct": di, "unshadowed": un, "hits": hc}
    for r in (1, 2, 3):
        for want in itertools.combinations(("direct", "unshadowed", "hits"), r):
            part = rl.render_direct(cam, world, lights, K, T, want=want, allow_degenerate=True)
            lpart = rl.render_pixels_direct(cam, world, x, y, lights, K, T, want=want, allow_degenerate=True)
            for k in full:
                if k in want:
                    assert _same(getattr(part, k), full[k]) and _same(getattr(lpart, k), full[k][y, x]), (want, k)
                else:
                    assert getattr(part, k) is None and getattr(lpart, k) is None, (want, k)


def test_a_list_longer_than_one_launchs_lanes(rl, golden):
    """More slots than the launch has lanes: the grid-stride loop runs more than once, and every repeat of the 703 pixels equals the first."""
    world, lights = _world(rl, golden, "golden_test_scene"), LIGHTS["golden_test_scene"]
    cam = _camera(rl, world, 1)
    lanes = rl.api.features_max_lanes()
    reps = lanes // (W0 * H0) + 2
    x, y = _pixels(cam)
    xs, ys = np.tile(x, reps), np.tile(y, reps)
    assert xs.size > lanes
    dl = rl.render_pixels_direct(cam, world, xs, ys, lights, 1, T)
    assert rl.api.last_query()["kernel"] == "direct_fast"
    d, u, h = dl.direct.reshape(reps, -1, 3), dl.unshadowed.reshape(reps, -1, 3), dl.hits.reshape(reps, -1)
    assert h[0].sum() > 0 and (d[0] > 0).any()
    for a in (d.view(np.uint64), u.view(np.uint64), h):  # bits, not values
        assert (a == a[0:1]).all()
    frame = rl.render_direct(cam, world, lights, 1, T)
    assert _same(frame.direct.reshape(-1, 3), d[0]) and _same(frame.unshadowed.reshape(-1, 3), u[0]) and _same(frame.hits.reshape(-1), h[0])


def test_first_sample_continuation(rl, oracle, golden):
    """hit_count of calls that continue each other adds exactly; the float sums of a continued call are that call's own fold: the model's for
    that first_sample."""
    world, lights = _world(rl, golden, "golden_test_scene"), LIGHTS["golden_test_scene"]
    K = 2
    three, two, one = _camera(rl, world, 3, 12, 8), _camera(rl, world, 2, 12, 8), _camera(rl, world, 1, 12, 8)
    whole = rl.render_direct(three, world, lights, K, T)
    a = rl.render_direct(two, world, lights, K, T, first_sample=0)
    b = rl.render_direct(one, world, lights, K, T, first_sample=2)
    assert _same(a.merge(b).hits, whole.hits) and whole.hits.sum() > 0
    di, un, hc, words, traced = dm.frame(oracle, world.desc, one.c, rl.pack_lights(lights), K, T, first_sample=2)
    assert _same3(b, di, un, hc) and (di > 0).any()
    fb = _free_frame(rl, world, one, lights, K, F=2)[0]
    assert _same3(fb, di, un, hc)
    # the merged floats are the same estimate, not one call's bits: two folds added, each a few roundings from the one fold
    assert np.allclose(a.merge(b).direct, whole.direct, rtol=1e-12, atol=0.0)


def test_device_forms_an_outside_pixel_and_an_untouched_buffer(rl, oracle, golden):
    import torch
    name, case = "random_world", CASES[0]
    S, K = case
    world, lights = _world(rl, golden, name), LIGHTS[name]
    cam = _camera(rl, world, S)
    di, un, hc, _, traced = _yardstick(rl, oracle, golden, name, case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)).to("cuda:0")
    host_f = lambda t: t.cpu().numpy().view(np.float64)
    host_u = lambda t: t.cpu().numpy().view(np.uint32)
    n = W0 * H0
    stream = torch.cuda.Stream()
    # the frame, asynchronous and counter-free on a side stream; the lights' array is dropped at once: the launch holds them by value
    d_di, d_un, d_hc = dev(np.full(n * 3, 77.0)), dev(np.full(n * 3, 77.0)), dev(np.full(n, 77, dtype=np.uint32))
    rl.render_direct_device(cam, world, lights, K, T, stream=stream.cuda_stream, d_direct=d_di.data_ptr(), d_unshadowed=d_un.data_ptr(), d_hits=d_hc.data_ptr())
    stream.synchronize()
    status = rl.api.render_status(world, allow_degenerate=True)
    assert _same(host_f(d_di).reshape(H0, W0, 3), di) and _same(host_f(d_un).reshape(H0, W0, 3), un) and _same(host_u(d_hc).reshape(H0, W0), hc)
    assert status["rays"] == S * n + traced
    # one output: the other buffers are untouched
    d_di.copy_(dev(np.full(n * 3, 77.0))), d_un.copy_(dev(np.full(n * 3, 77.0))), d_hc.fill_(77)
    rl.render_direct_device(cam, world, lights, K, T, d_unshadowed=d_un.data_ptr(), stats={}, allow_degenerate=True)
    assert _same(host_f(d_un).reshape(H0, W0, 3), un) and (host_f(d_di) == 77.0).all() and (host_u(d_hc) == 77).all()
    d_un.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_direct_device(cam, world, lights, K, T, row_first=1, row_step=3, d_direct=d_di.data_ptr(), stats={}, allow_degenerate=True)
    m = di[1::3].size
    assert _same(host_f(d_di)[:m].reshape(-1, W0, 3), di[1::3]) and (host_f(d_di)[m:] == 77.0).all() and (host_f(d_un) == 77.0).all()
    # the device list: shuffled, duplicates, one pixel outside the image -> zeros there
    rng = np.random.default_rng(8)
    x, y = rng.integers(0, W0, 300).astype(np.uint32), rng.integers(0, H0, 300).astype(np.uint32)
    x[0], y[0] = x[1], y[1]
    x[150], y[150] = W0, 3
    inside = np.arange(300) != 150
    d_x, d_y = dev(x), dev(y)
    for st in (None, {}):
        d_d, d_u, d_h = dev(np.full(302 * 3, 77.0)), dev(np.full(302 * 3, 77.0)), dev(np.full(302, 77, dtype=np.uint32))
        rl.render_pixels_direct_device(cam, world, d_x.data_ptr(), d_y.data_ptr(), 300, lights, K, T, d_direct=d_d.data_ptr(), d_unshadowed=d_u.data_ptr(),
                                       d_hits=d_h.data_ptr(), stats=st, allow_degenerate=True)
        torch.cuda.synchronize()
        if st is None:
            rl.api.render_status(world, allow_degenerate=True)
        gd, gu, gh = host_f(d_d).reshape(302, 3), host_f(d_u).reshape(302, 3), host_u(d_h)
        assert _same(gd[:300][inside], di[y[inside], x[inside]]) and _same(gu[:300][inside], un[y[inside], x[inside]])
        assert _same(gh[:300][inside], hc[y[inside], x[inside]])
        assert not gd[150].any() and not gu[150].any() and gh[150] == 0
        assert (gd[300:] == 77.0).all() and (gu[300:] == 77.0).all() and (gh[300:] == 77).all()


def test_errors_with_a_device(rl, golden):
    api = rl.api
    world, lights = _world(rl, golden, "golden_test_scene"), LIGHTS["golden_test_scene"]
    cam = _camera(rl, world, 2)
    smoke = rl.World.example_scene("cornell_smoke")
    scam = _camera(rl, smoke, 1)
    cl = LIGHTS["cornell_box"]
    for call in (lambda: rl.render_direct(scam, smoke, cl, 2), lambda: rl.render_pixels_direct(scam, smoke, [0], [0], cl, 2),
                 lambda: rl.render_pixels_direct(scam, smoke, [0], [0], cl, 2, stats={})):
        with pytest.raises(rl.RLError) as e:  # a scene with ConstantMedium objects: there is no seeded any-hit
            call()
        assert e.value.code == api.RL_E_UNSUPPORTED and "ConstantMedium" in str(e.value)
    for k, t in ((0, T), (2, 0.0), (2, float("nan")), (2, 1.5), (1 << 30, T)):  # S = 2, L = 2: K = 2^30 is S L K = 2^32
        with pytest.raises(rl.RLError) as e:
            rl.render_direct(cam, world, lights, k, t)
        assert e.value.code == api.RL_E_INVALID, (k, t)
    st = {"rays": 5}
    past = rl.render_direct(cam, world, lights, 2, T, row_first=H0, stats=st)  # a row past the frame: no rows, zeroed stats
    assert past.direct.shape == (0, W0, 3) and past.hits.shape == (0, W0) and st["rays"] == 0


def test_cpp_mirror_renders_direct(rl, golden):
    world, lights = _world(rl, golden, "golden_test_scene"), LIGHTS["golden_test_scene"]
    got = rl.direct.cpp_mirror_probe(20, 2, 1, lights, 3, 0.75)
    cam = rl.Camera(dataclasses.replace(world.params, image_width=20, samples_per_pixel=2))
    want = rl.render_direct(cam, world, lights, 3, 0.75, first_sample=1)
    assert _same3(got, want.direct, want.unshadowed, want.hits) and want.hits.sum() > 0 and (want.direct > 0).any()


# ----------------------------------------------------------------------------- 5. the hand-over to the fold is exercised
def test_the_any_hit_walk_hands_segments_to_the_fold(rl, oracle, golden):
    """The slow-trace counter of a counter-free call counts the camera rays AND the segments its walks re-traced.  The camera rays' share is
    what a counter-free feature render of the same camera reports (the same function walks them); the rest are shadow segments.
    Where the lights have to be: with the two lights of LIGHTS["stress60"] and with 18 other placements above, beside and just over the
    ground at K up to 32, four of them at K = 512 (1.1 million segments on this frame), the walk decided EVERY segment by itself (measured: 0 re-traced), and a
    1920 x 1080 frame re-traces 3,422 of 34 million rays, camera rays included.  The ambient rays the AO frame re-traces at R = 2 were
    listed one by one: all seven meet the 1e6-radius ground sphere within ~0.5 of its pole at the origin, where a root's error bound
    reaches the axis-pole band of fast_hit_is_order_sensitive (r - |q.y| = rho^2 / 2r against eps |d.y| ~ 1.2e-7 .. 1.7e-7).  A segment
    meets the ground only on the way to a light point UNDER it, so one of this test's two lights is a lamp buried 0.05 below the
    pole: its segments leave sphere and mesh surfaces that face it sideways, cross the ground next to the pole and are left to the
    fold (which finds them occluded).  The other light is the level one above the scene."""
    world = _world(rl, golden, "stress60")
    lights = [BURIED_LAMP, LIGHTS["stress60"][0]]
    S, K = CASES[2]
    cam = _camera(rl, world, S)
    di, un, hc, _, traced = _compose(rl, oracle, world, cam, *_pixels(cam), lights, K, T)
    di, un, hc = di.reshape(H0, W0, 3), un.reshape(H0, W0, 3), hc.reshape(H0, W0)
    free, q = _free_frame(rl, world, cam, lights, K)
    assert q["kernel"] == "direct_fast" and _same3(free, di, un, hc)
    x, y = _pixels(cam)
    cam.render_pixels_features(world, x, y, want=("hit_count",), allow_degenerate=True)
    fq = rl.api.last_query()
    assert fq["kernel"] == "features_fast"
    segments = q["retraced"] - fq["retraced"]
    print("stress60 37x19 S=%d K=%d L=2: segments traced" % (S, K), traced, "re-traced", segments, "; camera rays", S * W0 * H0, "re-traced", fq["retraced"])
    assert segments > 0, (q, fq)
    assert segments < traced, (q, fq)  # and the walk decides segments by itself: the fold does not do all the work
