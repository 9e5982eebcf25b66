"""GPU tier: the NEE path renders (rl.render_nee* / rl.render_pixels_nee*; include/rl_render.h "NEE path renders").
  1. bytes against the host composition get_rays -> per vertex hit_rays -> the light points' draws from the oracle's ChaCha script at the
     path's cursor -> the definition's arithmetic in numpy -> occluded_rays(tmax = T) -> scatter_rays at the advanced cursor, counters
     included; counting and counter-free calls, and the reference-order route with the fast traversal switched off;
  2. bytes against the definition in Python on the CPU oracle (tests/nee_model.py);
  3. row shards, pixel lists (also longer than one launch's lanes), each output alone, continued calls, device forms, a media scene, the
     C++ mirror;
  4. the estimator has ray_color's expectation (a statistical bound with fixed seeds);
  5. and a smaller variance on cornell_box;
  6. the hand-over of shadow segments from the any-hit walk to the reference's fold does happen."""
import dataclasses
import math
import os

import nee_model as nm
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
W0, H0 = 37, 19  # 703 pixels: not a multiple of a wave or of a workgroup; non-square, so x*W + y is not y*W + x
CASES = [(3, 2, 4), (1, 1, 1), (2, 3, 6)]  # (S, K, max_depth)
SCENES = ["cornell_box", "built_world", "stress60"]
T = 1.0 - 1e-6
# built_world's lights are geometry of the scene (DiffuseLight quads, _built_world): one level, one tilted, of different colours
BUILT_LIGHTS = [((-1.5, 4.0, -1.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), (6.0, 6.0, 6.0)), ((4.0, 2.0, -1.0), (0.0, 0.0, 2.0), (1.0, 1.5, 0.0), (5.0, 3.5, 2.0))]
LIGHTS = {
    "cornell_box": [((343.0, 554.0, 332.0), (-130.0, 0.0, 0.0), (0.0, 0.0, -105.0), 15.0)],  # its own light (cornell_box.rs)
    "built_world": BUILT_LIGHTS,
    # the direct suite's two lights above the scene (not geometry of it)
    "stress60": [((-6.0, 20.0, -6.0), (12.0, 0.0, 0.0), (0.0, 0.0, 12.0), (4.0, 4.0, 4.0)), ((14.0, 6.0, -4.0), (0.0, 0.0, 8.0), (2.0, 3.0, 0.0), (3.0, 2.0, 1.0))],
}
# the direct suite's lamp 0.05 under the pole of stress60's ground sphere (tests/test_gpu_render_direct.py says why)
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


def _built_world(rl):
    """A Lambertian ground sphere and 30 small spheres of four materials (Lambertian, Metal, Dielectric, Flat), every third one MOVING (segments
    and scattered rays inherit the ray's time), under two DiffuseLight quads: BUILT_LIGHTS, which lists every emitter of the scene."""
    rng = np.random.default_rng(2027)

    def build(b):
        mats = [b.lambertian(b.solid((0.6, 0.5, 0.4))), b.metal((0.8, 0.8, 0.7), 0.3), b.dielectric(1.5), b.flat()]
        objs = [b.sphere((0.0, -100.0, 0.0), 100.0, b.lambertian(b.solid((0.5, 0.6, 0.5))))]
        for i in range(30):
            c = np.array([rng.uniform(-3.0, 3.0), rng.uniform(0.2, 1.4), rng.uniform(-3.0, 3.0)])
            c2 = c + (0.0, rng.uniform(0.1, 0.4), 0.0) if i % 3 == 0 else None
            objs.append(b.sphere(c, rng.uniform(0.15, 0.5), mats[i % len(mats)], center2=c2))
        for q, u, v, e in BUILT_LIGHTS:
            objs.append(b.quad(q, u, v, b.diffuse_light(b.solid(e))))
        return b.bvh(objs)
    w = rl.World.build(build)
    w.params = rl.CameraParams(vfov=40.0, lookfrom=(6.0, 2.5, 5.0), lookat=(0.0, 0.5, 0.0), defocus_angle=0.6, focus_dist=8.0, background=(0.05, 0.06, 0.08),
                               seed=11)
    return w


_worlds = {}


def _world(rl, golden, name):
    if name not in _worlds:
        if name == "built_world":
            w = _built_world(rl)
        elif name == "stress60":  # the tree is larger than the LDS top; a mesh under a transform
            w = rl.World.stress_scene(60, 1, golden("spot_triangulated.obj.gz"), _spot_texture())
        else:
            w = rl.World.example_scene(name)
        _worlds[name] = w
    return _worlds[name]


def _camera(rl, world, S, max_depth, W=W0, H=H0):
    p = dataclasses.replace(world.params, image_width=W, aspect_ratio=W / (H + 0.5), samples_per_pixel=S, max_depth=max_depth)  # height = floor(W / aspect) = H
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (W, H)
    return cam


def _pixels(cam):
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
    return x, y


def _compose(rl, oracle, world, cam, px, py, lights, K, seg_tmax, F=0):
    """The host composition over DISTINCT pixels -> (sums [n, 3], sq [n, 3], the summed counters of its counting calls with rng_words = the
    paths' final word positions, path rays, segments traced, light-sampling vertices)."""
    api = rl.api
    W, H, S, D = cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel, cam.c.max_depth
    seed = cam.params.seed
    px, py = np.asarray(px, dtype=np.uint64), np.asarray(py, dtype=np.uint64)
    L = rl.pack_lights(lights)
    nL = L.shape[0]
    normals = [np.array(nm.cross([float(c) for c in L[l, 3:6]], [float(c) for c in L[l, 6:9]])) for l in range(nL)]
    kinds = world.materials()["kind"]
    bg = np.array([float(v) for v in cam.c.background])
    kf = 1.0 / (math.pi * K)
    n = px.shape[0]
    sums, sq = np.zeros((n, 3)), np.zeros((n, 3))
    tot = dict.fromkeys(COUNTERS, 0)
    path_rays = traced = sampled_vertices = 0

    def add(st, keys=COUNTERS):
        for k in keys:
            if k != "rng_words":
                tot[k] += st[k]
    for s in range(F, F + S):
        streams = np.uint64(s) * np.uint64(W * H) + px * np.uint64(W) + py
        rays, cur = cam.get_rays(px, py, api.pack_cursors(streams, 0))
        wp = cur["word_pos"].astype(np.uint64)
        c, thr = np.zeros((n, 3)), np.ones((n, 3))
        count_em = np.ones(n, dtype=bool)
        alive = np.arange(n)
        for i in range(1, D + 1):
            if alive.size == 0:
                break
            # 1. the closest hit
            st = {}
            hits = world.hit_rays(rays["origin"][alive], rays["dir"][alive], times=rays["time"][alive], tmin=1e-10, stats=st, allow_degenerate=True)
            add(st)
            path_rays += alive.size
            hit = hits["hit"] != 0
            miss = alive[~hit]
            c[miss] = c[miss] + thr[miss] * bg
            alive, hits = alive[hit], hits[hit]
            if alive.size == 0:
                break
            lam = (kinds[hits["material"]] == api.MAT_LAMBERTIAN) & (i < D)
            # 4. scatter and emitted, at the cursor behind the light points (the arithmetic of 2. and 3. below needs its texture value)
            cursors = api.pack_cursors(streams[alive], wp[alive] + np.where(lam, 4 * nL * K, 0).astype(np.uint64))
            st = {}
            sc, cur2 = world.scatter_rays(rays[alive], hits, cursors, seed, stats=st, allow_degenerate=True)
            add(st, ("flagged",))
            # 2. emitted
            em = count_em[alive]
            c[alive[em]] = c[alive[em]] + thr[alive[em]] * sc["emitted"][em]
            # 3. the light points: the path's own stream, from the word it stands at (every draw so far took one u64 = two words)
            li = np.nonzero(lam)[0]
            sampled_vertices += li.size
            if li.size:
                ab = np.zeros((li.size, nL, K, 2))
                for j, e in enumerate(li):
                    first = int(wp[alive[e]])
                    assert first % 2 == 0
                    script = oracle.chacha_script(seed, [("set_stream", int(streams[alive[e]]))] + [("f64",)] * (first // 2 + 2 * nL * K))[0][1:]
                    ab[j] = script[first // 2:].reshape(nL, K, 2)
                p, nrm, time = hits["p"][li], hits["normal"][li], rays["time"][alive[li]]
                dsum = np.zeros((li.size, 3))
                for l in range(nL):
                    Q, u, v, E = L[l, 0:3], L[l, 3:6], L[l, 6:9], L[l, 9:12]
                    nl = normals[l]
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
                        free = ok[~occ]
                        dsum[free] = dsum[free] + E[None, :] * g[~occ][:, None]
                tex = sc["attenuation"][li]  # the Lambertian's texture value
                c[alive[li]] = c[alive[li]] + ((thr[alive[li]] * tex) * dsum) * kf
            wp[alive] = cur2["word_pos"]
            some = sc["scatter"] != 0
            go = alive[some]
            thr[go] = thr[go] * sc["attenuation"][some]
            rays[go] = sc["scattered"][some]
            count_em[go] = ~lam[some]
            alive = go
        sums = sums + c
        sq = sq + c * c
        tot["rng_words"] += int(wp.sum(dtype=np.uint64))
    tot["rays"] = path_rays + traced  # (scatter_rays' own `rays` counts elements, not rays)
    return sums, sq, tot, path_rays, traced, sampled_vertices


_frames = {}


def _yardstick(rl, oracle, golden, name, case, lights=None):
    """The composition's W0 x H0 frame of `name` for case = (S, K, max_depth), computed once and shared."""
    key = (name, case, None if lights is None else repr(lights))
    if key not in _frames:
        world = _world(rl, golden, name)
        S, K, D = case
        cam = _camera(rl, world, S, D)
        su, sq, tot, path_rays, traced, sv = _compose(rl, oracle, world, cam, *_pixels(cam), LIGHTS[name] if lights is None else lights, K, T)
        for a in (su, sq):
            a.setflags(write=False)
        _frames[key] = (su.reshape(H0, W0, 3), sq.reshape(H0, W0, 3), tot, path_rays, traced, sv)
    return _frames[key]


def _free_frame(rl, world, cam, lights, K, F=0, want=None, seg_tmax=T):
    """The whole frame through a counter-free call (the host list form without stats) -> (PathNEE [H, W, 3], last_query())."""
    x, y = _pixels(cam)
    r = rl.render_pixels_nee(cam, world, x, y, lights, K, seg_tmax, first_sample=F, want=want, allow_degenerate=True)
    q = rl.api.last_query()
    H, W = cam.c.image_height, cam.c.image_width
    r3 = lambda a: None if a is None else a.reshape(H, W, 3)
    return rl.PathNEE(r3(r.sums), r3(r.sq), r.samples, K), q


def _same(got, want):
    return got is not None and got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == np.ascontiguousarray(want).tobytes()


def _same2(got, su, sq):
    return _same(got.sums, su) and _same(got.sq, sq)


# ----------------------------------------------------------------------------- 1. composition, counters, routes
def test_the_yardstick_itself_sees_connections_shadows_and_long_paths(rl, oracle, golden):
    """Asserted on the composition alone, before any result of the feature is looked at."""
    for name in SCENES:
        for case in CASES:
            S, K, D = case
            su, sq, tot, path_rays, traced, sv = _yardstick(rl, oracle, golden, name, case)
            nl = len(LIGHTS[name])
            assert np.isfinite(su).all() and (su >= 0.0).all() and (sq >= 0.0).all(), (name, case)
            assert S * W0 * H0 <= path_rays <= S * W0 * H0 * D and traced <= nl * K * sv, (name, case)
            if D == 1:
                assert sv == 0 and traced == 0 and path_rays == S * W0 * H0  # no light point without a vertex behind it
            else:
                assert 0 < traced < nl * K * sv and path_rays > S * W0 * H0, (name, case)  # some light samples skipped, some traced; paths go on
        su, sq, tot, path_rays, traced, sv = _yardstick(rl, oracle, golden, name, CASES[0])
        print(name, "path rays", path_rays, "light-sampling vertices", sv, "segments", traced, "lit pixels", int((su > 0).any(-1).sum()))
        assert (su > 0).any()


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-K%d-D%d" % c)
@pytest.mark.parametrize("name", SCENES)
def test_frames_are_the_compositions_bytes_on_every_route(rl, oracle, golden, name, case):
    api = rl.api
    S, K, D = case
    world = _world(rl, golden, name)
    cam = _camera(rl, world, S, D)
    lights = LIGHTS[name]
    su, sq, tot, path_rays, traced, _ = _yardstick(rl, oracle, golden, name, case)
    st = {}
    counting = rl.render_nee(cam, world, lights, K, T, stats=st, allow_degenerate=True)
    assert api.last_query() == {"kernel": "nee_reference", "retraced": 0}
    assert _same2(counting, su, sq), (name, case, np.argwhere(counting.sums != su)[:8], np.argwhere(counting.sq != sq)[:8])
    assert counting.samples == S and counting.light_samples == K
    # all seven counters are the composition's sums
    assert {k: st[k] for k in COUNTERS} == tot, (name, case, st, tot)
    assert st["rays"] == path_rays + traced
    for on, route in ((True, "nee_fast"), (False, "nee_reference")):
        api.set_fast_traversal(on)
        try:
            free, q = _free_frame(rl, world, cam, lights, K)
        finally:
            api.set_fast_traversal(True)
        assert q["kernel"] == route, (name, case, q)
        assert _same2(free, su, sq), (name, case, route, np.argwhere(free.sums != su)[:8])
        if not on:
            assert q["retraced"] == 0
    # the counting list form too
    x, y = _pixels(cam)
    st2 = {}
    lst = rl.render_pixels_nee(cam, world, x, y, lights, K, T, stats=st2, allow_degenerate=True)
    assert api.last_query()["kernel"] == "nee_reference"
    assert _same(lst.sums.reshape(H0, W0, 3), su) and _same(lst.sq.reshape(H0, W0, 3), sq)
    assert {k: st2[k] for k in COUNTERS} == tot


# ----------------------------------------------------------------------------- 2. the oracle
def test_frames_equal_the_definition_on_the_cpu_oracle(rl, oracle, golden):
    world = _world(rl, golden, "cornell_box")
    cam = _camera(rl, world, 2, 4, 12, 8)
    K, lights = 3, LIGHTS["cornell_box"]
    su, sq, words, rays = nm.frame(oracle, world.desc, world.materials(), cam.c, rl.pack_lights(lights), K, T)
    assert (su > 0).any() and rays > 2 * 96
    st = {}
    got = rl.render_nee(cam, world, lights, K, T, stats=st)
    assert _same2(got, su, sq), (got.sums, su)
    assert st["rng_words"] == words and st["rays"] == rays
    free, q = _free_frame(rl, world, cam, lights, K)
    assert q["kernel"] == "nee_fast" and _same2(free, su, sq)


# ----------------------------------------------------------------------------- 3. launch forms
def test_row_shards_lists_and_each_output_alone(rl, oracle, golden):
    name, case = "built_world", CASES[0]
    S, K, D = case
    world, lights = _world(rl, golden, name), LIGHTS[name]
    cam = _camera(rl, world, S, D)
    su, sq, _, _, _, _ = _yardstick(rl, oracle, golden, name, case)
    for first, step in ((0, 1), (1, 3), (2, 3)):
        sh = rl.render_nee(cam, world, lights, K, T, row_first=first, row_step=step, allow_degenerate=True)
        assert _same2(sh, su[first::step], sq[first::step]), (first, step)
    # a shuffled list with duplicates, counter-free and counting
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, W0, 900), rng.integers(0, H0, 900)
    assert np.unique(x * 100 + y).size < 900
    for st in (None, {}):
        lst = rl.render_pixels_nee(cam, world, x, y, lights, K, T, stats=st, allow_degenerate=True)
        assert _same2(lst, su[y, x], sq[y, x])
    empty = rl.render_pixels_nee(cam, world, [], [], lights, K, T)
    assert empty.sums.shape == (0, 3) and empty.sq.shape == (0, 3)
    with pytest.raises(rl.RLError) as e:  # the host form refuses a pixel outside the image
        rl.render_pixels_nee(cam, world, [0, W0], [0, 0], lights, K, T)
    assert e.value.code == rl.api.RL_E_INVALID
    # each output alone: the same bytes, the other not produced
    full = {"sums": su, "sq": sq}
    for want in (("sums",), ("sq",)):
        part = rl.render_nee(cam, world, lights, K, T, want=want, allow_degenerate=True)
        lpart = rl.render_pixels_nee(cam, world, x, y, lights, K, T, want=want, allow_degenerate=True)
        for k in full:
            if k in want:
                assert _same(getattr(part, k), full[k]) and _same(getattr(lpart, k), full[k][y, x]), (want, k)
            else:
                assert getattr(part, k) is None and getattr(lpart, k) is None, (want, k)


def test_a_list_longer_than_one_launchs_lanes(rl, golden):
    """More slots than the launch has lanes: the grid-stride loop runs more than once, and every repeat of the 703 pixels equals the first."""
    world, lights = _world(rl, golden, "built_world"), LIGHTS["built_world"]
    cam = _camera(rl, world, 1, 3)
    lanes = rl.api.features_max_lanes()
    reps = lanes // (W0 * H0) + 2
    x, y = _pixels(cam)
    xs, ys = np.tile(x, reps), np.tile(y, reps)
    assert xs.size > lanes
    r = rl.render_pixels_nee(cam, world, xs, ys, lights, 1, T, allow_degenerate=True)
    assert rl.api.last_query()["kernel"] == "nee_fast"
    a, b = r.sums.reshape(reps, -1, 3), r.sq.reshape(reps, -1, 3)
    assert (a[0] > 0).any()
    for v in (a.view(np.uint64), b.view(np.uint64)):  # bits, not values
        assert (v == v[0:1]).all()
    frame = rl.render_nee(cam, world, lights, 1, T, allow_degenerate=True)
    assert _same(frame.sums.reshape(-1, 3), a[0]) and _same(frame.sq.reshape(-1, 3), b[0])


def test_first_sample_continuation_is_moments_merge(rl, golden):
    """A sample's colour depends on its index alone, so renders that continue each other hold disjoint terms of one render's sums.
    Moments.merge states the continuation: samples add, sums and sq are added (two folds, each rounded on its own: the same estimate up
    to a few roundings, not one fold's bits).  The continued call itself is the definition from first_sample on: the oracle's bytes."""
    world, lights = _world(rl, golden, "cornell_box"), LIGHTS["cornell_box"]
    K, D = 2, 4
    three, two, one = (_camera(rl, world, s, D, 12, 8) for s in (3, 2, 1))
    whole = rl.render_nee(three, world, lights, K, T).moments()
    a = rl.render_nee(two, world, lights, K, T, first_sample=0)
    b = rl.render_nee(one, world, lights, K, T, first_sample=2)
    m = a.moments().merge(b.moments())
    assert m.samples == 3 == whole.samples and (whole.sums > 0).any()
    assert _same(m.sums, a.sums + b.sums) and _same(m.sq, a.sq + b.sq)
    assert np.allclose(m.sums, whole.sums, rtol=1e-12, atol=0.0) and np.allclose(m.sq, whole.sq, rtol=1e-12, atol=0.0)
    # S = 1 from sample 2 on: sq is the square of sums, and whole = (a's fold) + b's colour in one more rounded addition
    assert _same(b.sq, b.sums * b.sums)
    assert _same(whole.sums, a.sums + b.sums) and _same(whole.sq, a.sq + b.sums * b.sums)
    fb = _free_frame(rl, world, one, lights, K, F=2)[0]
    assert _same2(fb, b.sums, b.sq)
    assert m.variance_of_mean().shape == (8, 12, 3)


def test_device_forms_an_outside_pixel_and_an_untouched_buffer(rl, oracle, golden):
    import torch
    name, case = "built_world", CASES[0]
    S, K, D = case
    world, lights = _world(rl, golden, name), LIGHTS[name]
    cam = _camera(rl, world, S, D)
    su, sq, _, path_rays, traced, _ = _yardstick(rl, oracle, golden, name, case)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)).to("cuda:0")
    host_f = lambda t: t.cpu().numpy().view(np.float64)
    n = W0 * H0
    stream = torch.cuda.Stream()
    # the frame, asynchronous and counter-free on a side stream; the launch holds the lights by value
    d_su, d_sq = dev(np.full(n * 3, 77.0)), dev(np.full(n * 3, 77.0))
    rl.render_nee_device(cam, world, lights, K, T, stream=stream.cuda_stream, d_sums=d_su.data_ptr(), d_sq=d_sq.data_ptr())
    stream.synchronize()
    status = rl.api.render_status(world, allow_degenerate=True)
    assert _same(host_f(d_su).reshape(H0, W0, 3), su) and _same(host_f(d_sq).reshape(H0, W0, 3), sq)
    assert status["rays"] == path_rays + traced
    # one output: the other buffer is untouched
    d_su.copy_(dev(np.full(n * 3, 77.0))), d_sq.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_nee_device(cam, world, lights, K, T, d_sq=d_sq.data_ptr(), stats={}, allow_degenerate=True)
    assert _same(host_f(d_sq).reshape(H0, W0, 3), sq) and (host_f(d_su) == 77.0).all()
    d_sq.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_nee_device(cam, world, lights, K, T, row_first=1, row_step=3, d_sums=d_su.data_ptr(), stats={}, allow_degenerate=True)
    m = su[1::3].size
    assert _same(host_f(d_su)[:m].reshape(-1, W0, 3), su[1::3]) and (host_f(d_su)[m:] == 77.0).all() and (host_f(d_sq) == 77.0).all()
    # the device list: shuffled, duplicates, one pixel outside the image -> zeros there
    rng = np.random.default_rng(8)
    x, y = rng.integers(0, W0, 300).astype(np.uint32), rng.integers(0, H0, 300).astype(np.uint32)
    x[0], y[0] = x[1], y[1]
    x[150], y[150] = W0, 3
    inside = np.arange(300) != 150
    d_x, d_y = dev(x), dev(y)
    for st in (None, {}):
        d_a, d_b = dev(np.full(302 * 3, 77.0)), dev(np.full(302 * 3, 77.0))
        rl.render_pixels_nee_device(cam, world, d_x.data_ptr(), d_y.data_ptr(), 300, lights, K, T, d_sums=d_a.data_ptr(), d_sq=d_b.data_ptr(), stats=st,
                                    allow_degenerate=True)
        torch.cuda.synchronize()
        if st is None:
            rl.api.render_status(world, allow_degenerate=True)
        ga, gb = host_f(d_a).reshape(302, 3), host_f(d_b).reshape(302, 3)
        assert _same(ga[:300][inside], su[y[inside], x[inside]]) and _same(gb[:300][inside], sq[y[inside], x[inside]])
        assert not ga[150].any() and not gb[150].any()
        assert (ga[300:] == 77.0).all() and (gb[300:] == 77.0).all()


def test_errors_with_a_device(rl, golden):
    api = rl.api
    world, lights = _world(rl, golden, "built_world"), LIGHTS["built_world"]
    cam = _camera(rl, world, 2, 4)
    smoke = rl.World.example_scene("cornell_smoke")
    scam = _camera(rl, smoke, 1, 4)
    cl = LIGHTS["cornell_box"]
    for call in (lambda: rl.render_nee(scam, smoke, cl, 2), lambda: rl.render_pixels_nee(scam, smoke, [0], [0], cl, 2),
                 lambda: rl.render_pixels_nee(scam, smoke, [0], [0], cl, 2, stats={})):
        with pytest.raises(rl.RLError) as e:  # a scene with ConstantMedium objects: there is no seeded any-hit
            call()
        assert e.value.code == api.RL_E_UNSUPPORTED and "ConstantMedium" in str(e.value)
    for k, t in ((0, T), (2, 0.0), (2, float("nan")), (2, 1.5), (1 << 30, T)):  # S = 2, L = 2: K = 2^30 is S L K = 2^32
        with pytest.raises(rl.RLError) as e:
            rl.render_nee(cam, world, lights, k, t)
        assert e.value.code == api.RL_E_INVALID, (k, t)
    with pytest.raises(rl.RLError) as e:
        rl.render_nee(_camera(rl, world, 2, 0), world, lights, 2, T)
    assert e.value.code == api.RL_E_INVALID
    st = {"rays": 5}
    past = rl.render_nee(cam, world, lights, 2, T, row_first=H0, stats=st)  # a row past the frame: no rows, zeroed stats
    assert past.sums.shape == (0, W0, 3) and past.sq.shape == (0, W0, 3) and st["rays"] == 0


def test_cpp_mirror_renders_nee(rl):
    world = rl.World.golden_test_scene()
    lights = [((-1.0, 3.0, -2.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (4.0, 4.0, 4.0)), ((2.0, 2.5, 0.0), (0.0, 0.0, -2.0), (1.0, 1.0, 0.0), (3.0, 2.0, 1.0))]
    got = rl.nee.cpp_mirror_probe(20, 2, 1, lights, 3, 0.75)
    cam = rl.Camera(dataclasses.replace(world.params, image_width=20, samples_per_pixel=2))
    want = rl.render_nee(cam, world, lights, 3, 0.75, first_sample=1, allow_degenerate=True)
    assert _same2(got, want.sums, want.sq) and (want.sums > 0).any() and got.samples == 2


# ----------------------------------------------------------------------------- 4. the expectation is ray_color's
_stat = {}


def _moments_pair(rl, golden, name, S_nee, S_plain, D=6):
    """(NEE at S_nee samples, K = 1; Camera.render_moments at S_plain) of `name` at W0 x H0, max_depth D, both through counter-free device
    work where offered, computed once."""
    key = (name, S_nee, S_plain, D)
    if key not in _stat:
        world, lights = _world(rl, golden, name), LIGHTS[name]
        cn, cp = _camera(rl, world, S_nee, D), _camera(rl, world, S_plain, D)
        nee = _free_frame(rl, world, cn, lights, 1)[0].moments()
        plain = cp.render_moments(world, allow_degenerate=True)
        _stat[key] = (nee, plain)
    return _stat[key]


@pytest.mark.parametrize("name", ["cornell_box", "built_world"])
def test_the_estimator_has_ray_colors_expectation(rl, golden, name):
    """NEE at S = 256, K = 1 against the plain path tracer at 1024 spp, max_depth 6 both.  The two are unbiased estimators of the same
    pixel values provided `lights` lists every emitter (it does, on both scenes), and pixels have independent streams, so the mean over
    a set of P pixels has variance V = (sum of the pixels' variance_of_mean) / P^2.  Per channel, for the whole frame and for three row
    bands: |mean_nee - mean_plain| <= 6 sqrt(V_nee + V_plain).  Seeds are fixed, so the outcome is fixed.  A failure is a bias to find
    (the depth rule, a double count, kf), not a bound to widen."""
    nee, plain = _moments_pair(rl, golden, name, 256, 1024)
    assert nee.samples == 256 and plain.samples == 1024
    vn, vp = nee.variance_of_mean(), plain.variance_of_mean()
    mn, mp = nee.sums / nee.samples, plain.sums / plain.samples
    bands = {"frame": slice(0, H0), "top": slice(0, 6), "middle": slice(6, 13), "bottom": slice(13, H0)}
    for band, rows in bands.items():
        P = mn[rows].shape[0] * W0
        a, b = mn[rows].reshape(-1, 3).sum(0) / P, mp[rows].reshape(-1, 3).sum(0) / P
        V = (vn[rows].reshape(-1, 3).sum(0) + vp[rows].reshape(-1, 3).sum(0)) / (P * P)
        print(name, band, "mean nee", a, "mean plain", b, "difference", a - b, "bound", 6.0 * np.sqrt(V))
        assert (b > 0).all(), (name, band)
        assert (np.abs(a - b) <= 6.0 * np.sqrt(V)).all(), (name, band, a, b, 6.0 * np.sqrt(V))


# ----------------------------------------------------------------------------- 5. and less variance where the light is found by chance
def test_the_variance_on_cornell_box_is_below_the_plain_path_tracers(rl, golden):
    nee, plain = _moments_pair(rl, golden, "cornell_box", 64, 64)
    vn, vp = float(nee.variance_of_mean().sum()), float(plain.variance_of_mean().sum())
    print("cornell_box 37x19, 64 spp, max_depth 6: frame sum of variance_of_mean, NEE K = 1:", vn, " plain:", vp, " ratio:", vp / vn)
    assert 0.0 < vn < vp


# ----------------------------------------------------------------------------- 6. the hand-over to the fold is exercised
def test_the_any_hit_walk_hands_segments_to_the_fold(rl, oracle, golden):
    """The direct suite's buried lamp on stress60 (its docstring says why segments towards it are left undecided), beside the level light
    above the scene: the counter-free call reports re-traced rays and its bytes are still the composition's.  The re-traced path rays
    are set apart by a second render with the lamp lifted far above the scene: a path's rays do not depend on where the lights are (every
    light point costs its 4 words whether it counts or not), so the two renders walk the same path rays and differ in segments only; the
    direct suite measured that the walk decides every segment towards lights above this scene by itself."""
    name, case = "stress60", CASES[2]
    S, K, D = case
    world = _world(rl, golden, name)
    lights = [BURIED_LAMP, LIGHTS[name][0]]
    lifted = [((-0.3, 30.0, -0.3),) + BURIED_LAMP[1:], LIGHTS[name][0]]
    cam = _camera(rl, world, S, D)
    su, sq, _, path_rays, traced, _ = _yardstick(rl, oracle, golden, name, case, lights)
    free, q = _free_frame(rl, world, cam, lights, K)
    assert q["kernel"] == "nee_fast" and q["retraced"] > 0
    assert _same2(free, su, sq)
    _, q2 = _free_frame(rl, world, cam, lifted, K)
    segments = q["retraced"] - q2["retraced"]
    print("stress60 37x19 S=%d K=%d D=%d L=2: path rays" % case, path_rays, "segments traced", traced, "re-traced", q["retraced"], "of them segments", segments)
    assert 0 < segments < traced, (q, q2)
