"""GPU tier: the NEE path renders with multiple importance sampling (rl.render_nee_mis* / rl.render_pixels_nee_mis*; include/rl_render.h "NEE
path renders with multiple importance sampling"), on the NEE suite's frame, cases, scenes and lights.
  1. bytes and all seven counters against the host composition: the NEE suite's (get_rays -> per vertex hit_rays -> the light points'
     draws from the oracle's ChaCha script -> the definition's arithmetic in numpy -> occluded_rays(tmax = T) -> scatter_rays) with the
     weights and, from scatter_rays' direction, the scattered-ray step in numpy and occluded_rays for its segments; both heuristics,
     counting and counter-free calls, and the reference-order route with the fast traversal switched off;
  2. bytes against the definition in Python on the CPU oracle (tests/nee_mis_model.py);
  3. the relations to render_nee: the same words; other bytes, except where no strategy reaches a light;
  4. row shards, pixel lists (also longer than one launch's lanes), each output alone, continued calls, device forms, a media scene, the
     C++ mirror;
  5. the estimator has render_nee's expectation, also for lights that are not geometry of the scene (a statistical bound, fixed seeds);
  6. no sample exceeds what the lights emit, and the variance falls where plain NEE's fireflies are;
  7. the hand-over of segments from the any-hit walk to the reference's fold does happen."""
import ctypes
import dataclasses
import math

import nee_mis_model as mm
import nee_model as nm
import numpy as np
import pytest
from test_gpu_render_nee import BURIED_LAMP, CASES, COUNTERS, H0, LIGHTS, SCENES, T, W0, _camera, _pixels, _same, _same2, _world

pytestmark = pytest.mark.gpu
HEURISTICS = ("balance", "power")
CORNER_VIEW = dict(lookat=(364.0, 555.0, 280.0), vfov=1.0)  # cornell_box: the ceiling beside the light, one unit above it


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _weights(g, kf, bs):
    """-> {heuristic: wl (bs False) or wb (bs True)} of geometry terms g, one rounded operation per line of the definition."""
    q = g * kf
    q2 = q * q
    if bs:
        return {"balance": q / (1.0 + q), "power": q2 / (1.0 + q2)}
    return {"balance": g / (1.0 + q), "power": g / (1.0 + q2)}


def _compose(rl, oracle, world, cam, px, py, lights, K, seg_tmax, F=0):
    """The host composition over DISTINCT pixels, both heuristics at once (the path, the draws and every segment are the same for both:
    only the weights differ) -> ({heuristic: (sums [n, 3], sq [n, 3])}, the summed counters of its counting calls with rng_words = the
    paths' final word positions, path rays, light segments traced, scattered-ray segments traced, of them free)."""
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
    sums, sq = {h: np.zeros((n, 3)) for h in HEURISTICS}, {h: np.zeros((n, 3)) for h in HEURISTICS}
    tot = dict.fromkeys(COUNTERS, 0)
    path_rays = traced = made = free_made = 0

    def add(st, keys=COUNTERS):
        for k in keys:
            if k != "rng_words":
                tot[k] += st[k]
    for s in range(F, F + S):
        streams = np.uint64(s) * np.uint64(W * H) + px * np.uint64(W) + py
        rays, cur = cam.get_rays(px, py, api.pack_cursors(streams, 0))
        wp = cur["word_pos"].astype(np.uint64)
        c, thr = {h: np.zeros((n, 3)) for h in HEURISTICS}, np.ones((n, 3))
        count_em = np.ones(n, dtype=bool)
        alive = np.arange(n)
        for i in range(1, D + 1):
            if alive.size == 0:
                break
            # the closest hit
            st = {}
            hits = world.hit_rays(rays["origin"][alive], rays["dir"][alive], times=rays["time"][alive], tmin=1e-10, stats=st, allow_degenerate=True)
            add(st)
            path_rays += alive.size
            hit = hits["hit"] != 0
            miss = alive[~hit]
            for h in HEURISTICS:
                c[h][miss] = c[h][miss] + thr[miss] * bg
            alive, hits = alive[hit], hits[hit]
            if alive.size == 0:
                break
            lam = (kinds[hits["material"]] == api.MAT_LAMBERTIAN) & (i < D)
            # scatter and emitted, at the cursor behind the light points
            cursors = api.pack_cursors(streams[alive], wp[alive] + np.where(lam, 4 * nL * K, 0).astype(np.uint64))
            st = {}
            sc, cur2 = world.scatter_rays(rays[alive], hits, cursors, seed, stats=st, allow_degenerate=True)
            add(st, ("flagged",))
            em = count_em[alive]
            for h in HEURISTICS:
                c[h][alive[em]] = c[h][alive[em]] + thr[alive[em]] * sc["emitted"][em]
            li = np.nonzero(lam)[0]
            if li.size:
                # the light strategy: the NEE suite's draws and geometry, wl in g's place
                ab = np.zeros((li.size, nL, K, 2))
                for j, e in enumerate(li):
                    first = int(wp[alive[e]])
                    assert first % 2 == 0
                    script = oracle.chacha_script(seed, [("set_stream", int(streams[alive[e]]))] + [("f64",)] * (first // 2 + 2 * nL * K))[0][1:]
                    ab[j] = script[first // 2:].reshape(nL, K, 2)
                p, nrm, time = hits["p"][li], hits["normal"][li], rays["time"][alive[li]]
                dsum = {h: np.zeros((li.size, 3)) for h in HEURISTICS}
                for l in range(nL):
                    Q, u, v, E = L[l, 0:3], L[l, 3:6], L[l, 6:9], L[l, 9:12]
                    nl = normals[l]
                    for k in range(K):
                        a, b = ab[:, l, k, 0:1], ab[:, l, k, 1:2]
                        yl = (Q + u * a) + v * b
                        d = yl - p
                        d2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
                        cs = _dot(nrm, d)
                        cl = np.abs(_dot(nl[None, :], d))
                        ok = np.nonzero((cs > 0.0) & (cl > 0.0) & (d2 > 0.0))[0]
                        g = (cs[ok] * cl[ok]) / (d2[ok] * d2[ok])
                        ok, g = ok[g < np.inf], g[g < np.inf]
                        if ok.size == 0:
                            continue
                        st = {}
                        occ = rl.occluded_rays(world, p[ok], d[ok], times=time[ok], tmin=1e-10, tmax=seg_tmax, stats=st, allow_degenerate=True)
                        add(st)
                        traced += ok.size
                        fr = ok[~occ]
                        for h, wl in _weights(g[~occ], kf, False).items():
                            dsum[h][fr] = dsum[h][fr] + E[None, :] * wl[:, None]
                tex = sc["attenuation"][li]  # the Lambertian's texture value
                for h in HEURISTICS:
                    c[h][alive[li]] = c[h][alive[li]] + ((thr[alive[li]] * tex) * dsum[h]) * kf
            wp[alive] = cur2["word_pos"]
            some = sc["scatter"] != 0
            go = alive[some]
            thr[go] = thr[go] * sc["attenuation"][some]
            # the scattered-ray strategy, behind thr = thr * att: scatter_rays' direction against every light's parallelogram
            bi = np.nonzero(lam & some)[0]
            if bi.size:
                x, nrm, time, w = hits["p"][bi], hits["normal"][bi], rays["time"][alive[bi]], sc["scattered"]["dir"][bi]
                bsum = {h: np.zeros((bi.size, 3)) for h in HEURISTICS}
                for l in range(nL):
                    Q, u, v, E = L[l, 0:3], L[l, 3:6], L[l, 6:9], L[l, 9:12]
                    nl = normals[l][None, :]
                    den = _dot(nl, w)
                    ok = np.nonzero(np.abs(den) > 0.0)[0]
                    t = _dot(nl, Q[None, :] - x[ok]) / den[ok]
                    ok, t = ok[(t > 0.0) & (t < np.inf)], t[(t > 0.0) & (t < np.inf)]
                    d = w[ok] * t[:, None]
                    hv = (x[ok] + d) - Q[None, :]
                    nn = _dot(nl, nl)
                    al = _dot(nl, _cross(hv, v[None, :])) / nn
                    be = _dot(nl, _cross(u[None, :], hv)) / nn
                    d2, cs, cl = _dot(d, d), _dot(nrm[ok], d), np.abs(_dot(nl, d))
                    keep = (0.0 <= al) & (al <= 1.0) & (0.0 <= be) & (be <= 1.0) & (cs > 0.0) & (cl > 0.0) & (d2 > 0.0)
                    ok, d, d2, cs, cl = ok[keep], d[keep], d2[keep], cs[keep], cl[keep]
                    g = (cs * cl) / (d2 * d2)
                    ok, d, g = ok[g < np.inf], d[g < np.inf], g[g < np.inf]
                    if ok.size == 0:
                        continue
                    st = {}
                    occ = rl.occluded_rays(world, x[ok], d, times=time[ok], tmin=1e-10, tmax=seg_tmax, stats=st, allow_degenerate=True)
                    add(st)
                    made += ok.size
                    free_made += int((~occ).sum())
                    fr = ok[~occ]
                    for h, wb in _weights(g[~occ], kf, True).items():
                        bsum[h][fr] = bsum[h][fr] + E[None, :] * wb[:, None]
                for h in HEURISTICS:
                    c[h][alive[bi]] = c[h][alive[bi]] + thr[alive[bi]] * bsum[h]
            rays[go] = sc["scattered"][some]
            count_em[go] = ~lam[some]
            alive = go
        for h in HEURISTICS:
            sums[h] = sums[h] + c[h]
            sq[h] = sq[h] + c[h] * c[h]
        tot["rng_words"] += int(wp.sum(dtype=np.uint64))
    tot["rays"] = path_rays + traced + made
    return {h: (sums[h], sq[h]) for h in HEURISTICS}, tot, path_rays, traced, made, free_made


_frames = {}


def _yardstick(rl, oracle, golden, name, case, lights=None):
    """The composition's W0 x H0 frames of `name` for case = (S, K, max_depth), computed once and shared
    -> ({heuristic: (sums, sq)}, counters, path rays, light segments, scattered-ray segments, of them free)."""
    key = (name, case, None if lights is None else repr(lights))
    if key not in _frames:
        world = _world(rl, golden, name)
        S, K, D = case
        cam = _camera(rl, world, S, D)
        out, tot, path_rays, traced, made, free_made = _compose(rl, oracle, world, cam, *_pixels(cam), LIGHTS[name] if lights is None else lights, K, T)
        frames = {}
        for h, (su, sq) in out.items():
            su, sq = su.reshape(H0, W0, 3), sq.reshape(H0, W0, 3)
            su.setflags(write=False), sq.setflags(write=False)
            frames[h] = (su, sq)
        _frames[key] = (frames, tot, path_rays, traced, made, free_made)
    return _frames[key]


def _free_frame(rl, world, cam, lights, K, heuristic, F=0, want=None, seg_tmax=T):
    """The whole frame through a counter-free call (the host list form without stats) -> (PathNEE [H, W, 3], last_query())."""
    x, y = _pixels(cam)
    r = rl.render_pixels_nee_mis(cam, world, x, y, lights, K, seg_tmax, heuristic, first_sample=F, want=want, allow_degenerate=True)
    q = rl.api.last_query()
    H, W = cam.c.image_height, cam.c.image_width
    r3 = lambda a: None if a is None else a.reshape(H, W, 3)
    return rl.PathNEE(r3(r.sums), r3(r.sq), r.samples, K), q


def _nee_frame(rl, world, cam, lights, K, seg_tmax=T):
    x, y = _pixels(cam)
    r = rl.render_pixels_nee(cam, world, x, y, lights, K, seg_tmax, allow_degenerate=True)
    H, W = cam.c.image_height, cam.c.image_width
    return rl.PathNEE(r.sums.reshape(H, W, 3), r.sq.reshape(H, W, 3), r.samples, K)


# ----------------------------------------------------------------------------- 1. composition, counters, routes
def test_the_yardstick_itself_sees_both_strategies_free_and_occluded(rl, oracle, golden):
    """Asserted on the composition alone, before any result of the feature is looked at: in every scene scattered rays do cross lights, some
    of those segments are occluded and some free; light points count too; the two heuristics give different frames."""
    for name in SCENES:
        seen = free = 0
        for case in CASES:
            S, K, D = case
            frames, tot, path_rays, traced, made, free_made = _yardstick(rl, oracle, golden, name, case)
            for h in HEURISTICS:
                su, sq = frames[h]
                assert np.isfinite(su).all() and (su >= 0.0).all() and (sq >= 0.0).all(), (name, case, h)
            if D == 1:
                assert traced == 0 and made == 0 and path_rays == S * W0 * H0  # no strategy without a vertex behind it
                assert _same(frames["balance"][0], frames["power"][0])
            else:
                assert traced > 0 and 0 <= free_made <= made and path_rays > S * W0 * H0, (name, case)
                assert not _same(frames["balance"][0], frames["power"][0]), (name, case)
            seen, free = seen + made, free + free_made
            print(name, case, "path rays", path_rays, "light segments", traced, "scattered-ray segments", made, "of them free", free_made)
        assert 0 < free < seen, (name, seen, free)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "S%d-K%d-D%d" % c)
@pytest.mark.parametrize("name", SCENES)
def test_frames_are_the_compositions_bytes_on_every_route(rl, oracle, golden, name, case):
    api = rl.api
    S, K, D = case
    world = _world(rl, golden, name)
    cam = _camera(rl, world, S, D)
    lights = LIGHTS[name]
    frames, tot, path_rays, traced, made, _ = _yardstick(rl, oracle, golden, name, case)
    x, y = _pixels(cam)
    for h in HEURISTICS:
        su, sq = frames[h]
        st = {}
        counting = rl.render_nee_mis(cam, world, lights, K, T, h, stats=st, allow_degenerate=True)
        assert api.last_query() == {"kernel": "nee_mis_reference", "retraced": 0}
        assert _same2(counting, su, sq), (name, case, h, np.argwhere(counting.sums != su)[:8], np.argwhere(counting.sq != sq)[:8])
        assert counting.samples == S and counting.light_samples == K
        # all seven counters are the composition's sums
        assert {k: st[k] for k in COUNTERS} == tot, (name, case, h, st, tot)
        assert st["rays"] == path_rays + traced + made
        for on, route in ((True, "nee_mis_fast"), (False, "nee_mis_reference")):
            api.set_fast_traversal(on)
            try:
                free, q = _free_frame(rl, world, cam, lights, K, h)
            finally:
                api.set_fast_traversal(True)
            assert q["kernel"] == route, (name, case, h, q)
            assert _same2(free, su, sq), (name, case, h, route, np.argwhere(free.sums != su)[:8])
            if not on:
                assert q["retraced"] == 0
        # the counting list form too
        st2 = {}
        lst = rl.render_pixels_nee_mis(cam, world, x, y, lights, K, T, h, stats=st2, allow_degenerate=True)
        assert api.last_query()["kernel"] == "nee_mis_reference"
        assert _same(lst.sums.reshape(H0, W0, 3), su) and _same(lst.sq.reshape(H0, W0, 3), sq)
        assert {k: st2[k] for k in COUNTERS} == tot


# ----------------------------------------------------------------------------- 2. the oracle
def _lambertian_world(rl):
    """A Lambertian ground sphere and 12 Lambertian spheres, every third one moving, under built_world's two DiffuseLight quads: what
    tests/nee_mis_model.py states (Lambertian, DiffuseLight) with a sphere tree, occluders between surfaces and lights, and a tilted light."""
    rng = np.random.default_rng(31)
    lights = LIGHTS["built_world"]

    def build(b):
        objs = [b.sphere((0.0, -100.0, 0.0), 100.0, b.lambertian(b.solid((0.5, 0.6, 0.5))))]
        for i in range(12):
            c = np.array([rng.uniform(-2.5, 2.5), rng.uniform(0.3, 1.6), rng.uniform(-2.5, 2.5)])
            c2 = c + (0.0, 0.3, 0.0) if i % 3 == 0 else None
            objs.append(b.sphere(c, rng.uniform(0.3, 0.7), b.lambertian(b.solid(rng.uniform(0.2, 0.9, 3))), center2=c2))
        for q, u, v, e in lights:
            objs.append(b.quad(q, u, v, b.diffuse_light(b.solid(e))))
        return b.bvh(objs)
    w = rl.World.build(build)
    w.params = rl.CameraParams(vfov=40.0, lookfrom=(6.0, 2.5, 5.0), lookat=(0.0, 0.5, 0.0), background=(0.05, 0.06, 0.08), seed=5)
    return w, lights


@pytest.mark.parametrize("scene", ["cornell_box", "lambertian_world"])
def test_frames_equal_the_definition_on_the_cpu_oracle(rl, oracle, golden, scene):
    if scene == "cornell_box":
        world, lights = _world(rl, golden, "cornell_box"), LIGHTS["cornell_box"]
    else:
        world, lights = _lambertian_world(rl)
    cam = _camera(rl, world, 2, 4, 12, 8)
    K = 3
    made = 0
    for code, h in enumerate(HEURISTICS):
        su, sq, words, rays, info = mm.frame(oracle, world.desc, world.materials(), cam.c, rl.pack_lights(lights), K, T, heuristic=code)
        assert (su > 0).any() and rays > 2 * 96 and info["counted"] > 0
        made += info["made"]
        st = {}
        got = rl.render_nee_mis(cam, world, lights, K, T, h, stats=st)
        assert _same2(got, su, sq), (scene, h, got.sums, su)
        assert st["rng_words"] == words and st["rays"] == rays
        free, q = _free_frame(rl, world, cam, lights, K, h)
        assert q["kernel"] == "nee_mis_fast" and _same2(free, su, sq)
    print(scene, "scattered-ray connections of the two model frames", made)
    if scene == "lambertian_world":
        assert made > 0  # (cornell_box's light is small: a 12 x 8 frame at 2 samples may cross it nowhere)


# ----------------------------------------------------------------------------- 3. relations to render_nee
def test_the_words_are_render_nees_and_the_bytes_are_not(rl, golden):
    world, lights = _world(rl, golden, "cornell_box"), LIGHTS["cornell_box"]
    S, K, D = CASES[0]
    cam = _camera(rl, world, S, D)
    st0 = {}
    nee = rl.render_nee(cam, world, lights, K, T, stats=st0, allow_degenerate=True)
    for h in HEURISTICS:
        st = {}
        mis = rl.render_nee_mis(cam, world, lights, K, T, h, stats=st, allow_degenerate=True)
        assert st["rng_words"] == st0["rng_words"] and st["rays"] >= st0["rays"] and st["flagged"] == st0["flagged"]
        # every counted light point is weighted by 1 / (1 + q^b) < 1, however small q is
        assert not _same(mis.sums, nee.sums) and not _same(mis.sq, nee.sq)


def test_lights_no_strategy_reaches_leave_render_nees_bytes(rl):
    """nee_model's floor with a light under it: no light point counts (cs < 0) and a scattered ray crosses the light's plane at t < 0."""
    world, cam = nm.known_answer_cases(rl, 3, 2)["open"]
    st0 = {}
    nee = rl.render_nee(cam, world, nm.LIGHT_BELOW, 3, stats=st0)
    assert (nee.sums > 0).any()
    for h in HEURISTICS:
        st = {}
        mis = rl.render_nee_mis(cam, world, nm.LIGHT_BELOW, 3, heuristic=h, stats=st)
        assert _same2(mis, nee.sums, nee.sq) and {k: st[k] for k in COUNTERS} == {k: st0[k] for k in COUNTERS}


# ----------------------------------------------------------------------------- 4. launch forms
def test_row_shards_lists_and_each_output_alone(rl, oracle, golden):
    name, case, h = "built_world", CASES[0], "power"
    S, K, D = case
    world, lights = _world(rl, golden, name), LIGHTS[name]
    cam = _camera(rl, world, S, D)
    su, sq = _yardstick(rl, oracle, golden, name, case)[0][h]
    for first, step in ((0, 1), (1, 3), (2, 3)):
        sh = rl.render_nee_mis(cam, world, lights, K, T, h, row_first=first, row_step=step, allow_degenerate=True)
        assert _same2(sh, su[first::step], sq[first::step]), (first, step)
    # a shuffled list with duplicates, counter-free and counting
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, W0, 900), rng.integers(0, H0, 900)
    assert np.unique(x * 100 + y).size < 900
    for st in (None, {}):
        lst = rl.render_pixels_nee_mis(cam, world, x, y, lights, K, T, h, stats=st, allow_degenerate=True)
        assert _same2(lst, su[y, x], sq[y, x])
    empty = rl.render_pixels_nee_mis(cam, world, [], [], lights, K, T, h)
    assert empty.sums.shape == (0, 3) and empty.sq.shape == (0, 3)
    with pytest.raises(rl.RLError) as e:  # the host form refuses a pixel outside the image
        rl.render_pixels_nee_mis(cam, world, [0, W0], [0, 0], lights, K, T, h)
    assert e.value.code == rl.api.RL_E_INVALID
    # each output alone: the same bytes, the other not produced
    full = {"sums": su, "sq": sq}
    for want in (("sums",), ("sq",)):
        part = rl.render_nee_mis(cam, world, lights, K, T, h, want=want, allow_degenerate=True)
        lpart = rl.render_pixels_nee_mis(cam, world, x, y, lights, K, T, h, want=want, allow_degenerate=True)
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
    r = rl.render_pixels_nee_mis(cam, world, xs, ys, lights, 1, T, "balance", allow_degenerate=True)
    assert rl.api.last_query()["kernel"] == "nee_mis_fast"
    a, b = r.sums.reshape(reps, -1, 3), r.sq.reshape(reps, -1, 3)
    assert (a[0] > 0).any()
    for v in (a.view(np.uint64), b.view(np.uint64)):  # bits, not values
        assert (v == v[0:1]).all()
    frame = rl.render_nee_mis(cam, world, lights, 1, T, "balance", allow_degenerate=True)
    assert _same(frame.sums.reshape(-1, 3), a[0]) and _same(frame.sq.reshape(-1, 3), b[0])


def test_first_sample_continuation_is_moments_merge(rl, golden):
    """A sample's colour depends on its index alone: renders that continue each other hold disjoint terms of one render's sums, and
    Moments.merge adds them (the NEE suite's test of the same name says what is bits and what is a few roundings)."""
    world, lights = _world(rl, golden, "cornell_box"), LIGHTS["cornell_box"]
    K, D, h = 2, 4, "balance"
    three, two, one = (_camera(rl, world, s, D, 12, 8) for s in (3, 2, 1))
    whole = rl.render_nee_mis(three, world, lights, K, T, h).moments()
    a = rl.render_nee_mis(two, world, lights, K, T, h, first_sample=0)
    b = rl.render_nee_mis(one, world, lights, K, T, h, first_sample=2)
    m = a.moments().merge(b.moments())
    assert m.samples == 3 == whole.samples and (whole.sums > 0).any()
    assert _same(m.sums, a.sums + b.sums) and _same(m.sq, a.sq + b.sq)
    assert np.allclose(m.sums, whole.sums, rtol=1e-12, atol=0.0) and np.allclose(m.sq, whole.sq, rtol=1e-12, atol=0.0)
    assert _same(b.sq, b.sums * b.sums)
    assert _same(whole.sums, a.sums + b.sums) and _same(whole.sq, a.sq + b.sums * b.sums)
    fb = _free_frame(rl, world, one, lights, K, h, F=2)[0]
    assert _same2(fb, b.sums, b.sq)
    assert m.variance_of_mean().shape == (8, 12, 3)


def test_device_forms_an_outside_pixel_and_an_untouched_buffer(rl, oracle, golden):
    import torch
    name, case, h = "built_world", CASES[0], "balance"
    S, K, D = case
    world, lights = _world(rl, golden, name), LIGHTS[name]
    cam = _camera(rl, world, S, D)
    frames, _, path_rays, traced, made, _ = _yardstick(rl, oracle, golden, name, case)
    su, sq = frames[h]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)).to("cuda:0")
    host_f = lambda t: t.cpu().numpy().view(np.float64)
    n = W0 * H0
    stream = torch.cuda.Stream()
    # the frame, asynchronous and counter-free on a side stream; the launch holds the lights by value
    d_su, d_sq = dev(np.full(n * 3, 77.0)), dev(np.full(n * 3, 77.0))
    rl.render_nee_mis_device(cam, world, lights, K, T, h, stream=stream.cuda_stream, d_sums=d_su.data_ptr(), d_sq=d_sq.data_ptr())
    stream.synchronize()
    status = rl.api.render_status(world, allow_degenerate=True)
    assert _same(host_f(d_su).reshape(H0, W0, 3), su) and _same(host_f(d_sq).reshape(H0, W0, 3), sq)
    assert status["rays"] == path_rays + traced + made
    # one output: the other buffer is untouched
    d_su.copy_(dev(np.full(n * 3, 77.0))), d_sq.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_nee_mis_device(cam, world, lights, K, T, h, d_sq=d_sq.data_ptr(), stats={}, allow_degenerate=True)
    assert _same(host_f(d_sq).reshape(H0, W0, 3), sq) and (host_f(d_su) == 77.0).all()
    d_sq.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_nee_mis_device(cam, world, lights, K, T, h, row_first=1, row_step=3, d_sums=d_su.data_ptr(), stats={}, allow_degenerate=True)
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
        rl.render_pixels_nee_mis_device(cam, world, d_x.data_ptr(), d_y.data_ptr(), 300, lights, K, T, h, d_sums=d_a.data_ptr(), d_sq=d_b.data_ptr(), stats=st,
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
    for call in (lambda: rl.render_nee_mis(scam, smoke, cl, 2), lambda: rl.render_pixels_nee_mis(scam, smoke, [0], [0], cl, 2, heuristic="power"),
                 lambda: rl.render_pixels_nee_mis(scam, smoke, [0], [0], cl, 2, stats={})):
        with pytest.raises(rl.RLError) as e:  # a scene with ConstantMedium objects: there is no seeded any-hit
            call()
        assert e.value.code == api.RL_E_UNSUPPORTED and "ConstantMedium" in str(e.value)
    for k, t in ((0, T), (2, 0.0), (2, float("nan")), (2, 1.5), (1 << 30, T)):  # S = 2, L = 2: K = 2^30 is S L K = 2^32
        with pytest.raises(rl.RLError) as e:
            rl.render_nee_mis(cam, world, lights, k, t)
        assert e.value.code == api.RL_E_INVALID, (k, t)
    with pytest.raises(rl.RLError) as e:
        rl.render_nee_mis(_camera(rl, world, 2, 0), world, lights, 2, T)
    assert e.value.code == api.RL_E_INVALID
    # a third heuristic reaches the library only past the Python layer: refused there too, with a device
    sums = np.full((H0, W0, 3), 7.0)
    lp = rl.pack_lights(lights)
    rc = api.render_lib().rl_rtiow_render_nee_mis_rows(world.device(), ctypes.byref(cam.c), 0, 0, 1, lp.shape[0], lp.ctypes.data, 2, T, 2, sums.ctypes.data, None, None)
    assert rc == api.RL_E_INVALID and (sums == 7.0).all()
    st = {"rays": 5}
    past = rl.render_nee_mis(cam, world, lights, 2, T, row_first=H0, stats=st)  # a row past the frame: no rows, zeroed stats
    assert past.sums.shape == (0, W0, 3) and past.sq.shape == (0, W0, 3) and st["rays"] == 0


def test_cpp_mirror_renders_nee_mis(rl):
    world = rl.World.golden_test_scene()
    lights = [((-1.0, 3.0, -2.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (4.0, 4.0, 4.0)), ((2.0, 2.5, 0.0), (0.0, 0.0, -2.0), (1.0, 1.0, 0.0), (3.0, 2.0, 1.0))]
    cam = rl.Camera(dataclasses.replace(world.params, image_width=20, samples_per_pixel=2))
    seen = []
    for h in HEURISTICS:
        got = rl.nee.cpp_mirror_probe_mis(20, 2, 1, lights, 3, 0.75, h)
        want = rl.render_nee_mis(cam, world, lights, 3, 0.75, h, first_sample=1, allow_degenerate=True)
        assert _same2(got, want.sums, want.sq) and (want.sums > 0).any() and got.samples == 2
        seen.append(want.sums)
    assert not _same(seen[0], seen[1])  # the mirror hands the heuristic on


# ----------------------------------------------------------------------------- 5. the expectation is render_nee's
_stat = {}


def _moments(rl, golden, name, S, D, heuristic, view=None, K=1):
    """NEE (heuristic None) or MIS moments of `name` at W0 x H0 through counter-free calls, computed once."""
    key = (name, S, D, heuristic, None if view is None else repr(view), K)
    if key not in _stat:
        world, lights = _world(rl, golden, name), LIGHTS[name]
        p = world.params if view is None else dataclasses.replace(world.params, **view)
        p = dataclasses.replace(p, image_width=W0, aspect_ratio=W0 / (H0 + 0.5), samples_per_pixel=S, max_depth=D)
        cam = rl.Camera(p)
        assert (cam.c.image_width, cam.c.image_height) == (W0, H0)
        r = _nee_frame(rl, world, cam, lights, K) if heuristic is None else _free_frame(rl, world, cam, lights, K, heuristic)[0]
        _stat[key] = r.moments()
    return _stat[key]


@pytest.mark.parametrize("heuristic", HEURISTICS)
@pytest.mark.parametrize("name", SCENES)
def test_the_estimator_has_render_nees_expectation(rl, golden, name, heuristic):
    """MIS at S = 256, K = 1 against render_nee at 256 samples, max_depth 6 both.  Both strategies estimate the listed lights' contribution
    through the segment test and their weights sum to one, so the two renders are unbiased estimators of the same pixel values for ANY
    lights: stress60's are not geometry of the scene and the equality must hold there too.  Pixels have independent streams, so the mean
    over a set of P pixels has variance V = (sum of the pixels' variance_of_mean) / P^2.  Per channel, for the whole frame and for the NEE
    suite's three row bands: |mean_mis - mean_nee| <= 6 sqrt(V_mis + V_nee).  (The two renders share their draws, which makes them
    positively correlated; the bound is the independent one and therefore the wider.)  Seeds are fixed, so the outcome is fixed.  A
    failure is a bias to find (a weight, a double count, the crossing test), not a bound to widen."""
    mis, nee = _moments(rl, golden, name, 256, 6, heuristic), _moments(rl, golden, name, 256, 6, None)
    assert mis.samples == 256 and nee.samples == 256
    vm, vn = mis.variance_of_mean(), nee.variance_of_mean()
    mm_, mn = mis.sums / mis.samples, nee.sums / nee.samples
    bands = {"frame": slice(0, H0), "top": slice(0, 6), "middle": slice(6, 13), "bottom": slice(13, H0)}
    for band, rows in bands.items():
        P = mm_[rows].shape[0] * W0
        a, b = mm_[rows].reshape(-1, 3).sum(0) / P, mn[rows].reshape(-1, 3).sum(0) / P
        V = (vm[rows].reshape(-1, 3).sum(0) + vn[rows].reshape(-1, 3).sum(0)) / (P * P)
        print(name, heuristic, band, "mean mis", a, "mean nee", b, "difference", a - b, "bound", 6.0 * np.sqrt(V))
        assert (b > 0).all(), (name, band)
        assert (np.abs(a - b) <= 6.0 * np.sqrt(V)).all(), (name, heuristic, band, a, b, 6.0 * np.sqrt(V))


# ----------------------------------------------------------------------------- 6. the cap on fireflies
@pytest.mark.parametrize("name", SCENES)
def test_no_sample_exceeds_what_the_lights_emit(rl, golden, name):
    """S = 1: sq is the square of one sample.  A sample is at most B = max(background) + Emax (1 + (D - 1) L (K + 1)): the background or an
    emitter seen once (thr <= 1, textures <= 1), and at each of at most D - 1 sampling vertices L K weighted light points of at most
    thr tex E kf' (wl kf <= 1) and L scattered-ray terms of at most thr E (wb <= 1).  Plain NEE has no such bound."""
    world, lights = _world(rl, golden, name), LIGHTS[name]
    Emax = float(rl.pack_lights(lights)[:, 9:12].max())
    for K, D in ((1, 6), (3, 50)):
        cam = _camera(rl, world, 1, D)
        B = max(float(v) for v in cam.c.background) + Emax * (1.0 + (D - 1) * len(lights) * (K + 1))
        for h in HEURISTICS:
            for F in (0, 1, 2, 3):
                r = _free_frame(rl, world, cam, lights, K, h, F=F)[0]
                assert np.isfinite(r.sq).all() and (r.sq <= B * B).all(), (name, K, D, h, F, float(r.sq.max()), B * B)
                assert _same(r.sq, r.sums * r.sums)


def test_the_variance_beside_cornell_boxs_light_is_below_render_nees(rl, golden):
    """cornell_box looked at where the ceiling meets its light (the light hangs one unit under it), S = 16, K = 1, max_depth 3: plain NEE's
    geometry term reaches 1e4 there.  The CPU model gave a frame sum of variance_of_mean of 195.2 for NEE against 60.9 (balance) and 61.6
    (power)."""
    nee = _moments(rl, golden, "cornell_box", 16, 3, None, CORNER_VIEW)
    vn = float(nee.variance_of_mean().sum())
    for h in HEURISTICS:
        mis = _moments(rl, golden, "cornell_box", 16, 3, h, CORNER_VIEW)
        vm = float(mis.variance_of_mean().sum())
        print("cornell_box beside the light, 37x19, 16 spp, max_depth 3: frame sum of variance_of_mean, NEE:", vn, h, vm, "largest sample bound sqrt(max sq)",
              math.sqrt(float(nee.sq.max())), math.sqrt(float(mis.sq.max())))
        assert 0.0 < vm < vn


def test_the_variance_under_a_ceiling_light_is_below_render_nees(rl, oracle):
    """nee_model's floor under a 2000 x 2000 light, S = 16, K = 1, max_depth 2, on the pixels whose every sample starts on the floor."""
    world, cam = nm.known_answer_cases(rl, 2, 16)["ceiling"]
    floor = (mm.first_hit_kinds(oracle, world, cam.c) == nm.MAT_LAMBERTIAN).all(axis=0)
    assert floor.sum() >= 36
    nee = rl.render_nee(cam, world, [nm.CEILING], 1).moments()
    vn = float(nee.variance_of_mean()[floor].sum())
    E = np.array(nm.CEILING[3])
    for h in HEURISTICS:
        mis = rl.render_nee_mis(cam, world, [nm.CEILING], 1, heuristic=h).moments()
        v = mis.variance_of_mean()[floor]
        P = int(floor.sum())
        mean = (mis.sums[floor] / 16).sum(0) / P
        print("ceiling floor pixels", P, h, "mean", mean, "variance", float(v.sum()), "NEE", vn)
        assert 0.0 < float(v.sum()) < vn
        assert (np.abs(mean - nm.ALBEDO * E) <= 6.0 * np.sqrt(v.sum(0)) / P).all()


# ----------------------------------------------------------------------------- 7. the hand-over to the fold is exercised
def test_the_any_hit_walk_hands_segments_to_the_fold(rl, oracle, golden):
    """The NEE suite's buried-lamp case (its docstring says why segments towards the lamp are left undecided): the counter-free call
    reports re-traced rays and its bytes are still the composition's."""
    name, case = "stress60", CASES[2]
    S, K, D = case
    world = _world(rl, golden, name)
    lights = [BURIED_LAMP, LIGHTS[name][0]]
    cam = _camera(rl, world, S, D)
    frames, _, path_rays, traced, made, free_made = _yardstick(rl, oracle, golden, name, case, lights)
    for h in HEURISTICS:
        free, q = _free_frame(rl, world, cam, lights, K, h)
        assert q["kernel"] == "nee_mis_fast" and q["retraced"] > 0, q
        assert _same2(free, *frames[h])
    print("stress60 37x19 S=%d K=%d D=%d L=2: path rays" % case, path_rays, "light segments", traced, "scattered-ray segments", made, "free", free_made,
          "re-traced", q["retraced"])
