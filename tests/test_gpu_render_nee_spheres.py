"""GPU tier: the NEE path renders with sphere lights (rl.render_nee_mis*(..., sphere_lights=); include/rl_render.h "NEE path renders with
sphere lights").
  1. the yardstick (the host composition) meets all eight kinds of term on the chosen inputs, checked before any result is looked at;
  2. bytes and all seven counters against the host composition: get_rays -> per vertex hit_rays -> the light points' draws from the
     model's stream (f64 pairs for the quads, UnitSphere for the spheres, whose word count varies) -> the definition's arithmetic in
     numpy -> occluded_rays(tmax = T) -> scatter_rays at the cursor behind the draws -> the scattered ray's candidates in numpy ->
     occluded_rays; both heuristics, the counting call, and both counter-free routes;
  3. bytes against the definition in Python on the CPU oracle (tests/nee_spheres_model.py);
  4. no sphere: render_nee_mis' bytes and kernels;  5.-8. shards, lists, continuation, device forms;  9. errors;  10. the C++ mirror;
  11. the expectation is render_moments' with both of simple_light's emitters listed, and NOT with the sphere left out; the analytic
      floor under a sphere;  12. the cap on every sample."""
import dataclasses
import math

import nee_spheres_model as sm
import numpy as np
import pytest
from nee_model import cross as _cross3
from test_gpu_render_nee import COUNTERS, H0, T, W0, _camera, _pixels, _same, _same2
from test_gpu_render_nee_mis import HEURISTICS, _dot, _lambertian_world, _weights

pytestmark = pytest.mark.gpu
QUAD = ((3.0, 1.0, -2.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), (4.0, 4.0, 4.0))  # simple_light.rs' quad light
BALL = ((0.0, 7.0, 0.0), 2.0, (4.0, 4.0, 4.0))                                 # and its sphere light


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


def _floor_world(rl):
    """nee_model's grey floor quad at y = 0 alone, its camera at (0, 1, 6), a dim background."""
    w = rl.World.build(lambda b: b.list([b.quad((-10.0, 0.0, -10.0), (20.0, 0.0, 0.0), (0.0, 0.0, 18.0), b.lambertian(b.solid((0.5, 0.5, 0.5))))]))
    w.params = rl.CameraParams(vfov=60.0, lookfrom=(0.0, 1.0, 6.0), lookat=(0.0, 0.0, 0.0), background=(0.02, 0.03, 0.04), seed=7)
    return w


_inputs = {}


def _input(rl, name):
    """-> (world, quad lights, sphere lights, (S, K, max_depth)) of the four byte-test inputs."""
    if name not in _inputs:
        if name == "simple_light":  # Perlin textures; both lights are geometry of the scene
            _inputs[name] = (rl.World.simple_light(), [QUAD], [BALL], (2, 2, 5))
        elif name == "lambertian_world":  # a sphere light that is NOT geometry, over 12 spheres that stand between it and the ground
            w, quads = _lambertian_world(rl)
            _inputs[name] = (w, quads, [((0.5, 5.0, -0.5), 1.0, (3.0, 4.0, 5.0)), ((-2.0, 1.0, 2.0), 0.25, 6.0)], (2, 1, 4))
        elif name == "enclosing":  # the floor points within 1.94 of the origin are INSIDE the sphere light: nothing from it there
            _inputs[name] = (_floor_world(rl), [], [((0.0, 0.5, 0.0), 2.0, (2.0, 3.0, 4.0))], (3, 2, 3))
        elif name == "tangent":  # the floor touches the sphere at the origin: d2 -> 0 around it and g grows without bound
            _inputs[name] = (_floor_world(rl), [], [((0.0, 1.0, 0.0), 1.0, (2.0, 3.0, 4.0))], (4, 3, 2))
    return _inputs[name]


INPUTS = ("simple_light", "lambertian_world", "enclosing", "tangent")


def _compose(rl, oracle, world, cam, px, py, lights, spheres, K, seg_tmax, F=0):
    """The host composition over DISTINCT pixels, both heuristics at once -> ({heuristic: (sums [n, 3], sq [n, 3])}, the summed counters of
    its counting calls with rng_words = the paths' final word positions, info: the eight kinds of term counted, the sphere points drawn
    and skipped, the largest g, the candidates the g < inf skip took)."""
    api = rl.api
    W, H, S, D = cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel, cam.c.max_depth
    seed = cam.params.seed
    px, py = np.asarray(px, dtype=np.uint64), np.asarray(py, dtype=np.uint64)
    L = rl.pack_lights(lights) if len(lights) else np.zeros((0, 12))
    Sp = rl.pack_sphere_lights(spheres)
    nL, nS = L.shape[0], Sp.shape[0]
    normals = [np.array(_cross3([float(c) for c in L[l, 3:6]], [float(c) for c in L[l, 6:9]])) for l in range(nL)]
    areas = [(4.0 * math.pi) * (float(Sp[j, 3]) * float(Sp[j, 3])) for j in range(nS)]
    kinds = world.materials()["kind"]
    bg = np.array([float(v) for v in cam.c.background])
    kf = 1.0 / (math.pi * K)
    n = px.shape[0]
    sums, sq = {h: np.zeros((n, 3)) for h in HEURISTICS}, {h: np.zeros((n, 3)) for h in HEURISTICS}
    tot = dict.fromkeys(COUNTERS, 0)
    info = sm.new_info()
    info.update(path_rays=0, segments=0, g_max=0.0, g_not_finite=0)

    def add(st, keys=COUNTERS):
        for k in keys:
            if k != "rng_words":
                tot[k] += st[k]

    def connect(x, nrm, time, ok, d, cl, facing, E, kind, strategy, acc):
        """The shared statement behind a candidate: d2, cs, the skip, g, its skip, the weight, the segment, the sum.  ok indexes acc."""
        d2, cs = _dot(d, d), _dot(nrm[ok], d)
        keep = (cs > 0.0) & facing & (d2 > 0.0)
        ok, d, d2, cs, cl = ok[keep], d[keep], d2[keep], cs[keep], cl[keep]
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            g = (cs * cl) / (d2 * d2)
        fin = g < np.inf
        info["g_not_finite"] += int((~fin).sum())
        ok, d, g = ok[fin], d[fin], g[fin]
        if ok.size == 0:
            return
        info["g_max"] = max(info["g_max"], float(g.max()))
        st = {}
        occ = rl.occluded_rays(world, x[ok], d, times=time[ok], tmin=1e-10, tmax=seg_tmax, stats=st, allow_degenerate=True)
        add(st)
        info["segments"] += ok.size
        info[f"{kind}_{strategy}_free"] += int((~occ).sum())
        info[f"{kind}_{strategy}_occluded"] += int(occ.sum())
        fr = ok[~occ]
        for h, w in _weights(g[~occ], kf, strategy == "scatter").items():
            acc[h][fr] = acc[h][fr] + E[None, :] * w[:, None]
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
            st = {}
            hits = world.hit_rays(rays["origin"][alive], rays["dir"][alive], times=rays["time"][alive], tmin=1e-10, stats=st, allow_degenerate=True)
            add(st)
            info["path_rays"] += alive.size
            hit = hits["hit"] != 0
            miss = alive[~hit]
            for h in HEURISTICS:
                c[h][miss] = c[h][miss] + thr[miss] * bg
            alive, hits = alive[hit], hits[hit]
            if alive.size == 0:
                break
            lam = (kinds[hits["material"]] == api.MAT_LAMBERTIAN) & (i < D)
            li = np.nonzero(lam)[0]
            # the light points' draws, from the model's stream at the path's cursor: their word count varies with the tries
            after = wp[alive].copy()
            ab, wu = np.zeros((li.size, nL, K, 2)), np.zeros((li.size, nS, K, 3))
            for j, e in enumerate(li):
                first = int(wp[alive[e]])
                rng = sm.StreamAt(oracle, seed, int(streams[alive[e]]), first)
                for l in range(nL):
                    for k in range(K):
                        ab[j, l, k] = (rng.f64(), rng.f64())
                for l in range(nS):
                    for k in range(K):
                        wu[j, l, k] = rng.unit_sphere()
                after[e] = rng.words()
            info["sphere_drawn"] += li.size * nS * K
            # scatter and emitted, at the cursor behind the light points
            st = {}
            sc, cur2 = world.scatter_rays(rays[alive], hits, api.pack_cursors(streams[alive], after), seed, stats=st, allow_degenerate=True)
            add(st, ("flagged",))
            em = count_em[alive]
            for h in HEURISTICS:
                c[h][alive[em]] = c[h][alive[em]] + thr[alive[em]] * sc["emitted"][em]
            if li.size:  # the light strategy: the quads, then the spheres
                p, nrm, time = hits["p"][li], hits["normal"][li], rays["time"][alive[li]]
                dsum = {h: np.zeros((li.size, 3)) for h in HEURISTICS}
                every = np.arange(li.size)
                for l in range(nL):
                    Q, u, v, E = L[l, 0:3], L[l, 3:6], L[l, 6:9], L[l, 9:12]
                    for k in range(K):
                        a, b = ab[:, l, k, 0:1], ab[:, l, k, 1:2]
                        yl = (Q + u * a) + v * b
                        d = yl - p
                        cl = np.abs(_dot(normals[l][None, :], d))
                        connect(p, nrm, time, every, d, cl, cl > 0.0, E, "quad", "light", dsum)
                for l in range(nS):
                    C, r, E = Sp[l, 0:3], Sp[l, 3], Sp[l, 4:7]
                    for k in range(K):
                        w = wu[:, l, k, :]
                        yl = C + w * r
                        d = yl - p
                        co = -_dot(w, d)
                        info["sphere_skipped"] += int((~((_dot(nrm, d) > 0.0) & (co > 0.0) & (_dot(d, d) > 0.0))).sum())
                        connect(p, nrm, time, every, d, co * areas[l], co > 0.0, E, "sphere", "light", dsum)
                tex = sc["attenuation"][li]  # the Lambertian's texture value
                for h in HEURISTICS:
                    c[h][alive[li]] = c[h][alive[li]] + ((thr[alive[li]] * tex) * dsum[h]) * kf
            wp[alive] = cur2["word_pos"]
            some = sc["scatter"] != 0
            go = alive[some]
            thr[go] = thr[go] * sc["attenuation"][some]
            bi = np.nonzero(lam & some)[0]
            if bi.size:  # the scattered-ray strategy, behind thr = thr * att
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
                    al = _dot(nl, _np_cross(hv, v[None, :])) / nn
                    be = _dot(nl, _np_cross(u[None, :], hv)) / nn
                    inside = (0.0 <= al) & (al <= 1.0) & (0.0 <= be) & (be <= 1.0)
                    ok, d = ok[inside], d[inside]
                    cl = np.abs(_dot(nl, d))
                    connect(x, nrm, time, ok, d, cl, cl > 0.0, E, "quad", "scatter", bsum)
                for l in range(nS):
                    C, r, E = Sp[l, 0:3], Sp[l, 3], Sp[l, 4:7]
                    oc = x - C[None, :]
                    a = _dot(w, w)
                    hb = _dot(oc, w)
                    cc = _dot(oc, oc) - r * r
                    disc = hb * hb - a * cc
                    ok = np.nonzero(disc > 0.0)[0]
                    sd = np.sqrt(disc[ok])
                    t = (-hb[ok] - sd) / a[ok]
                    ok, t = ok[(t > 0.0) & (t < np.inf)], t[(t > 0.0) & (t < np.inf)]
                    d = w[ok] * t[:, None]
                    y = x[ok] + d
                    wn = (y - C[None, :]) / r
                    co = -_dot(wn, d)
                    connect(x, nrm, time, ok, d, co * areas[l], co > 0.0, E, "sphere", "scatter", bsum)
                for h in HEURISTICS:
                    c[h][alive[bi]] = c[h][alive[bi]] + thr[alive[bi]] * bsum[h]
            rays[go] = sc["scattered"][some]
            count_em[go] = ~lam[some]
            alive = go
        for h in HEURISTICS:
            sums[h] = sums[h] + c[h]
            sq[h] = sq[h] + c[h] * c[h]
        tot["rng_words"] += int(wp.sum(dtype=np.uint64))
    tot["rays"] = info["path_rays"] + info["segments"]
    return {h: (sums[h], sq[h]) for h in HEURISTICS}, tot, info


def _np_cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


_frames = {}


def _yardstick(rl, oracle, name):
    """The composition's W0 x H0 frames of input `name`, computed once and shared -> ({heuristic: (sums, sq)}, counters, info)."""
    if name not in _frames:
        world, quads, balls, (S, K, D) = _input(rl, name)
        cam = _camera(rl, world, S, D)
        out, tot, info = _compose(rl, oracle, world, cam, *_pixels(cam), quads, balls, K, T)
        frames = {}
        for h, (su, sq) in out.items():
            su, sq = su.reshape(H0, W0, 3), sq.reshape(H0, W0, 3)
            su.setflags(write=False), sq.setflags(write=False)
            frames[h] = (su, sq)
        _frames[name] = (frames, tot, info)
    return _frames[name]


def _free_frame(rl, world, cam, quads, balls, K, heuristic, F=0, want=None):
    """The whole frame through a counter-free call (the host list form without stats) -> (PathNEE [H, W, 3], last_query())."""
    x, y = _pixels(cam)
    r = rl.render_pixels_nee_mis(cam, world, x, y, quads, K, T, heuristic, first_sample=F, want=want, allow_degenerate=True, sphere_lights=balls)
    q = rl.api.last_query()
    H, W = cam.c.image_height, cam.c.image_width
    r3 = lambda a: None if a is None else a.reshape(H, W, 3)
    return rl.PathNEE(r3(r.sums), r3(r.sq), r.samples, K), q


# ----------------------------------------------------------------------------- 1. the yardstick
def test_the_yardstick_meets_all_eight_kinds_of_term(rl, oracle):
    """A condition on the inputs, asserted on the composition alone: (quad | sphere) x (light point | scattered ray) x (free | occluded)
    each occur; sphere points are skipped as back-facing; inside the enclosing sphere nothing arrives; beside the tangent point g is
    large."""
    total = sm.new_info()
    for name in INPUTS:
        frames, tot, info = _yardstick(rl, oracle, name)
        print(name, info, tot)
        for h in HEURISTICS:
            su, sq = frames[h]
            assert np.isfinite(su).all() and (su >= 0.0).all() and (sq >= 0.0).all(), (name, h)
        assert not _same(frames["balance"][0], frames["power"][0]), name
        assert 0 < info["sphere_skipped"] < info["sphere_drawn"], name
        for k in total:
            if k != "largest":
                total[k] += info[k]
    for kind in ("quad", "sphere"):
        for strategy in ("light", "scatter"):
            for o in ("free", "occluded"):
                assert total[f"{kind}_{strategy}_{o}"] > 0, (kind, strategy, o, total)
    info = _yardstick(rl, oracle, "lambertian_world")[2]
    assert info["sphere_light_occluded"] > 0 and info["sphere_scatter_free"] > 0  # the light that is not geometry, behind occluders
    print("tangent: largest g", _yardstick(rl, oracle, "tangent")[2]["g_max"], "candidates the g < inf skip took", _yardstick(rl, oracle, "tangent")[2]["g_not_finite"])
    assert _yardstick(rl, oracle, "tangent")[2]["g_max"] > 1e3


def test_inside_the_enclosing_sphere_the_floor_gets_nothing(rl):
    """The pixel looking at the origin of the `enclosing` input: every vertex there is inside the sphere light, so the sample is the
    background its scattered ray finds, thr * background <= background; outside the sphere the floor is lit."""
    world, quads, balls, (S, K, D) = _input(rl, "enclosing")
    cam = _camera(rl, world, S, 2)
    r = rl.render_nee_mis(cam, world, quads, K, T, sphere_lights=balls)
    centre = r.sums[H0 // 2, W0 // 2] / S
    assert (centre <= np.array(world.params.background) + 1e-15).all() and (r.sums[H0 - 1] / S > np.array(world.params.background)).any()


# ----------------------------------------------------------------------------- 2. composition, counters, routes
@pytest.mark.parametrize("name", INPUTS)
def test_frames_are_the_compositions_bytes_on_every_route(rl, oracle, name):
    api = rl.api
    world, quads, balls, (S, K, D) = _input(rl, name)
    cam = _camera(rl, world, S, D)
    frames, tot, info = _yardstick(rl, oracle, name)
    x, y = _pixels(cam)
    for h in HEURISTICS:
        su, sq = frames[h]
        st = {}
        counting = rl.render_nee_mis(cam, world, quads, K, T, h, stats=st, allow_degenerate=True, sphere_lights=balls)
        assert api.last_query() == {"kernel": "nee_spheres_reference", "retraced": 0}
        assert _same2(counting, su, sq), (name, h, np.argwhere(counting.sums != su)[:8], np.argwhere(counting.sq != sq)[:8])
        assert counting.samples == S and counting.light_samples == K
        assert {k: st[k] for k in COUNTERS} == tot, (name, h, st, tot)
        assert st["rays"] == info["path_rays"] + info["segments"]
        for on, route in ((True, "nee_spheres_fast"), (False, "nee_spheres_reference")):
            api.set_fast_traversal(on)
            try:
                free, q = _free_frame(rl, world, cam, quads, balls, K, h)
            finally:
                api.set_fast_traversal(True)
            assert q["kernel"] == route, (name, h, q)
            assert _same2(free, su, sq), (name, h, route, np.argwhere(free.sums != su)[:8])
            if not on:
                assert q["retraced"] == 0
        st2 = {}
        lst = rl.render_pixels_nee_mis(cam, world, x, y, quads, K, T, h, stats=st2, allow_degenerate=True, sphere_lights=balls)
        assert api.last_query()["kernel"] == "nee_spheres_reference"
        assert _same(lst.sums.reshape(H0, W0, 3), su) and _same(lst.sq.reshape(H0, W0, 3), sq)
        assert {k: st2[k] for k in COUNTERS} == tot


# ----------------------------------------------------------------------------- 3. the oracle
def test_frames_equal_the_definition_on_the_cpu_oracle(rl, oracle):
    world, quads, balls, _ = _input(rl, "lambertian_world")
    cam = _camera(rl, world, 2, 4, 9, 5)
    K = 2
    for code, h in enumerate(HEURISTICS):
        su, sq, words, rays, info = sm.frame(oracle, world.desc, world.materials(), cam.c, rl.pack_lights(quads), rl.pack_sphere_lights(balls), K, T, heuristic=code)
        assert (su > 0).any() and rays > 2 * 45 and info["sphere_light_free"] > 0 and info["sphere_skipped"] > 0
        st = {}
        got = rl.render_nee_mis(cam, world, quads, K, T, h, stats=st, sphere_lights=balls)
        assert _same2(got, su, sq), (h, got.sums, su)
        assert st["rng_words"] == words and st["rays"] == rays
        free, q = _free_frame(rl, world, cam, quads, balls, K, h)
        assert q["kernel"] == "nee_spheres_fast" and _same2(free, su, sq)


# ----------------------------------------------------------------------------- 4. no sphere: the MIS call
def test_no_sphere_is_render_nee_mis_and_a_sphere_is_not(rl):
    api = rl.api
    world, quads, balls, (S, K, D) = _input(rl, "simple_light")
    cam = _camera(rl, world, S, D)
    x, y = _pixels(cam)
    for h in HEURISTICS:
        st0, st1 = {}, {}
        mis = rl.render_nee_mis(cam, world, quads, K, T, h, stats=st0, allow_degenerate=True)
        assert api.last_query()["kernel"] == "nee_mis_reference"
        none = rl.render_nee_mis(cam, world, quads, K, T, h, stats=st1, allow_degenerate=True, sphere_lights=[])
        assert api.last_query()["kernel"] == "nee_mis_reference"
        assert _same2(none, mis.sums, mis.sq) and {k: st0[k] for k in COUNTERS} == {k: st1[k] for k in COUNTERS}
        lst = rl.render_pixels_nee_mis(cam, world, x, y, quads, K, T, h, allow_degenerate=True, sphere_lights=np.zeros((0, 7)))
        assert api.last_query()["kernel"] == "nee_mis_fast"
        assert _same(lst.sums.reshape(H0, W0, 3), mis.sums)
        with_ball = rl.render_pixels_nee_mis(cam, world, x, y, quads, K, T, h, allow_degenerate=True, sphere_lights=balls)
        assert api.last_query()["kernel"] == "nee_spheres_fast"
        assert not _same(with_ball.sums.reshape(H0, W0, 3), mis.sums)


# ----------------------------------------------------------------------------- 5.-8. launch forms
def test_row_shards_lists_and_each_output_alone(rl, oracle):
    name, h = "simple_light", "power"
    world, quads, balls, (S, K, D) = _input(rl, name)
    cam = _camera(rl, world, S, D)
    su, sq = _yardstick(rl, oracle, name)[0][h]
    kw = dict(allow_degenerate=True, sphere_lights=balls)
    for first, step in ((0, 1), (1, 3), (2, 3)):
        sh = rl.render_nee_mis(cam, world, quads, K, T, h, row_first=first, row_step=step, **kw)
        assert _same2(sh, su[first::step], sq[first::step]), (first, step)
    rng = np.random.default_rng(5)
    x, y = rng.integers(0, W0, 900), rng.integers(0, H0, 900)
    assert np.unique(x * 100 + y).size < 900
    for st in (None, {}):
        lst = rl.render_pixels_nee_mis(cam, world, x, y, quads, K, T, h, stats=st, **kw)
        assert _same2(lst, su[y, x], sq[y, x])
    empty = rl.render_pixels_nee_mis(cam, world, [], [], quads, K, T, h, sphere_lights=balls)
    assert empty.sums.shape == (0, 3) and empty.sq.shape == (0, 3)
    with pytest.raises(rl.RLError) as e:  # the host form refuses a pixel outside the image
        rl.render_pixels_nee_mis(cam, world, [0, W0], [0, 0], quads, K, T, h, sphere_lights=balls)
    assert e.value.code == rl.api.RL_E_INVALID
    full = {"sums": su, "sq": sq}
    for want in (("sums",), ("sq",)):
        part = rl.render_nee_mis(cam, world, quads, K, T, h, want=want, **kw)
        lpart = rl.render_pixels_nee_mis(cam, world, x, y, quads, K, T, h, want=want, **kw)
        for k in full:
            if k in want:
                assert _same(getattr(part, k), full[k]) and _same(getattr(lpart, k), full[k][y, x]), (want, k)
            else:
                assert getattr(part, k) is None and getattr(lpart, k) is None, (want, k)


def test_a_list_longer_than_one_launchs_lanes(rl):
    """More slots than the launch has lanes: the grid-stride loop runs more than once, and every repeat of the 703 pixels equals the first."""
    world, quads, balls, _ = _input(rl, "simple_light")
    cam = _camera(rl, world, 1, 3)
    lanes = rl.api.features_max_lanes()
    reps = lanes // (W0 * H0) + 2
    x, y = _pixels(cam)
    xs, ys = np.tile(x, reps), np.tile(y, reps)
    assert xs.size > lanes
    r = rl.render_pixels_nee_mis(cam, world, xs, ys, quads, 1, T, "balance", allow_degenerate=True, sphere_lights=balls)
    assert rl.api.last_query()["kernel"] == "nee_spheres_fast"
    a, b = r.sums.reshape(reps, -1, 3), r.sq.reshape(reps, -1, 3)
    assert (a[0] > 0).any()
    for v in (a.view(np.uint64), b.view(np.uint64)):  # bits, not values
        assert (v == v[0:1]).all()
    frame = rl.render_nee_mis(cam, world, quads, 1, T, "balance", allow_degenerate=True, sphere_lights=balls)
    assert _same(frame.sums.reshape(-1, 3), a[0]) and _same(frame.sq.reshape(-1, 3), b[0])


def test_first_sample_continuation_is_moments_merge(rl):
    world, quads, balls, _ = _input(rl, "simple_light")
    K, D, h = 2, 4, "balance"
    three, two, one = (_camera(rl, world, s, D, 12, 8) for s in (3, 2, 1))
    kw = dict(sphere_lights=balls)
    whole = rl.render_nee_mis(three, world, quads, K, T, h, **kw).moments()
    a = rl.render_nee_mis(two, world, quads, K, T, h, first_sample=0, **kw)
    b = rl.render_nee_mis(one, world, quads, K, T, h, first_sample=2, **kw)
    m = a.moments().merge(b.moments())
    assert m.samples == 3 == whole.samples and (whole.sums > 0).any()
    assert _same(m.sums, a.sums + b.sums) and _same(m.sq, a.sq + b.sq)
    assert _same(b.sq, b.sums * b.sums)
    assert _same(whole.sums, a.sums + b.sums) and _same(whole.sq, a.sq + b.sums * b.sums)
    fb = _free_frame(rl, world, one, quads, balls, K, h, F=2)[0]
    assert _same2(fb, b.sums, b.sq)


def test_device_forms_an_outside_pixel_and_an_untouched_buffer(rl, oracle):
    import torch
    name, h = "simple_light", "balance"
    world, quads, balls, (S, K, D) = _input(rl, name)
    cam = _camera(rl, world, S, D)
    frames, tot, info = _yardstick(rl, oracle, name)
    su, sq = frames[h]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)).to("cuda:0")
    host_f = lambda t: t.cpu().numpy().view(np.float64)
    n = W0 * H0
    stream = torch.cuda.Stream()
    d_su, d_sq = dev(np.full(n * 3, 77.0)), dev(np.full(n * 3, 77.0))
    rl.render_nee_mis_device(cam, world, quads, K, T, h, stream=stream.cuda_stream, d_sums=d_su.data_ptr(), d_sq=d_sq.data_ptr(), sphere_lights=balls)
    stream.synchronize()
    status = rl.api.render_status(world, allow_degenerate=True)
    assert _same(host_f(d_su).reshape(H0, W0, 3), su) and _same(host_f(d_sq).reshape(H0, W0, 3), sq)
    assert status["rays"] == tot["rays"]
    # one output: the other buffer is untouched
    d_su.copy_(dev(np.full(n * 3, 77.0))), d_sq.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_nee_mis_device(cam, world, quads, K, T, h, d_sq=d_sq.data_ptr(), stats={}, allow_degenerate=True, sphere_lights=balls)
    assert _same(host_f(d_sq).reshape(H0, W0, 3), sq) and (host_f(d_su) == 77.0).all()
    d_sq.copy_(dev(np.full(n * 3, 77.0)))
    rl.render_nee_mis_device(cam, world, quads, K, T, h, row_first=1, row_step=3, d_sums=d_su.data_ptr(), stats={}, allow_degenerate=True, sphere_lights=balls)
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
        rl.render_pixels_nee_mis_device(cam, world, d_x.data_ptr(), d_y.data_ptr(), 300, quads, K, T, h, d_sums=d_a.data_ptr(), d_sq=d_b.data_ptr(), stats=st,
                                        allow_degenerate=True, sphere_lights=balls)
        torch.cuda.synchronize()
        if st is None:
            rl.api.render_status(world, allow_degenerate=True)
        ga, gb = host_f(d_a).reshape(302, 3), host_f(d_b).reshape(302, 3)
        assert _same(ga[:300][inside], su[y[inside], x[inside]]) and _same(gb[:300][inside], sq[y[inside], x[inside]])
        assert not ga[150].any() and not gb[150].any()
        assert (ga[300:] == 77.0).all() and (gb[300:] == 77.0).all()


# ----------------------------------------------------------------------------- 9. errors
def test_errors_with_a_device(rl):
    api = rl.api
    world, quads, balls, _ = _input(rl, "simple_light")
    cam = _camera(rl, world, 2, 4)
    smoke = rl.World.example_scene("cornell_smoke")
    scam = _camera(rl, smoke, 1, 4)
    for call in (lambda: rl.render_nee_mis(scam, smoke, quads, 2, sphere_lights=balls),
                 lambda: rl.render_pixels_nee_mis(scam, smoke, [0], [0], [], 2, heuristic="power", sphere_lights=balls),
                 lambda: rl.render_pixels_nee_mis(scam, smoke, [0], [0], quads, 2, stats={}, sphere_lights=balls)):
        with pytest.raises(rl.RLError) as e:  # a scene with ConstantMedium objects: there is no seeded any-hit
            call()
        assert e.value.code == api.RL_E_UNSUPPORTED and "ConstantMedium" in str(e.value)
    bad = [dict(lights=[], sphere_lights=[]), dict(lights=[QUAD] * 16, sphere_lights=balls), dict(lights=[], sphere_lights=[BALL] * 17),
           dict(lights=quads, sphere_lights=[((0.0, 7.0, 0.0), 0.0, 4.0)]), dict(lights=quads, sphere_lights=[((0.0, 7.0, 0.0), -1.0, 4.0)]),
           dict(lights=quads, sphere_lights=[((0.0, float("nan"), 0.0), 2.0, 4.0)]), dict(lights=quads, sphere_lights=[((0.0, 7.0, 0.0), 2.0, float("inf"))]),
           dict(lights=quads, sphere_lights=[((0.0, 7.0, 0.0), 1e160, 4.0)]), dict(lights=quads, sphere_lights=balls, light_samples=0),
           dict(lights=quads, sphere_lights=balls, seg_tmax=1.5), dict(lights=quads, sphere_lights=balls, light_samples=1 << 30)]  # S (L + Ls) K = 2^32
    for kw in bad:
        with pytest.raises(rl.RLError) as e:
            rl.render_nee_mis(cam, world, **kw)
        assert e.value.code == api.RL_E_INVALID, kw
    with pytest.raises(rl.RLError) as e:
        rl.render_nee_mis(_camera(rl, world, 2, 0), world, quads, 2, T, sphere_lights=balls)
    assert e.value.code == api.RL_E_INVALID
    st = {"rays": 5}
    past = rl.render_nee_mis(cam, world, quads, 2, T, row_first=H0, stats=st, sphere_lights=balls)  # a row past the frame: no rows, zeroed stats
    assert past.sums.shape == (0, W0, 3) and past.sq.shape == (0, W0, 3) and st["rays"] == 0
    ok = rl.render_nee_mis(cam, world, [], 2, T, sphere_lights=balls)  # no quad at all
    assert (ok.sums > 0).any()


# ----------------------------------------------------------------------------- 10. the C++ mirror
def test_cpp_mirror_renders_with_sphere_lights(rl):
    world = rl.World.simple_light()
    cam = rl.Camera(dataclasses.replace(world.params, image_width=20, samples_per_pixel=2, max_depth=6))
    seen = []
    for h in HEURISTICS:
        got = rl.nee.cpp_mirror_probe_spheres(20, 2, 1, [QUAD], [BALL], 3, 0.75, h)
        want = rl.render_nee_mis(cam, world, [QUAD], 3, 0.75, h, first_sample=1, allow_degenerate=True, sphere_lights=[BALL])
        assert _same2(got, want.sums, want.sq) and (want.sums > 0).any() and got.samples == 2
        seen.append(want.sums)
    assert not _same(seen[0], seen[1])
    only = rl.nee.cpp_mirror_probe_spheres(20, 2, 1, [], [BALL], 3, 0.75, "balance")  # the mirror hands an empty quad list on
    want = rl.render_nee_mis(cam, world, [], 3, 0.75, "balance", first_sample=1, allow_degenerate=True, sphere_lights=[BALL])
    assert _same2(only, want.sums, want.sq) and not _same(only.sums, seen[0])


# ----------------------------------------------------------------------------- 11. the expectation
GROUND_VIEW = dict(lookat=(2.0, 0.0, 4.0), vfov=15.0)  # simple_light: the ground beside the Perlin sphere, under the sphere light
_stat = {}


def _ground(rl, what, S=64, D=6):
    """Moments of simple_light's ground view at W0 x H0, S samples, max_depth D: "path" (render_moments), or (heuristic, with the sphere?)."""
    key = (what, S, D)
    if key not in _stat:
        world = _input(rl, "simple_light")[0]
        p = dataclasses.replace(world.params, image_width=W0, aspect_ratio=W0 / (H0 + 0.5), samples_per_pixel=S, max_depth=D, **GROUND_VIEW)
        cam = rl.Camera(p)
        assert (cam.c.image_width, cam.c.image_height) == (W0, H0)
        if what == "path":
            _stat[key] = cam.render_moments(world, allow_degenerate=True)
        else:
            h, ball = what
            _stat[key] = _free_frame(rl, world, cam, [QUAD], [BALL] if ball else [], 1, h)[0].moments()
    return _stat[key]


def _frame_mean(m):
    P = m.sums.shape[0] * m.sums.shape[1]
    return (m.sums / m.samples).reshape(-1, 3).sum(0) / P, m.variance_of_mean().reshape(-1, 3).sum(0) / (P * P)


@pytest.mark.parametrize("heuristic", HEURISTICS)
def test_the_expectation_is_ray_colors_with_both_emitters_listed_and_not_without_the_sphere(rl, heuristic):
    """simple_light, the ground under the sphere light, 37 x 19, S = 64, K = 1, max_depth 6: with the quad AND the sphere listed the frame
    mean agrees with render_moments of the same camera within 6 sigma of the two renders' own variance (pixels have independent streams:
    V = sum of variance_of_mean / P^2 each, added); with the sphere left out of the list the same render lies OUTSIDE 6 sigma: what the
    sphere casts on the ground is what was missing.  Seeds are fixed, so the outcome is fixed."""
    a, va = _frame_mean(_ground(rl, (heuristic, True)))
    b, vb = _frame_mean(_ground(rl, "path"))
    c, vc = _frame_mean(_ground(rl, (heuristic, False)))
    print(heuristic, "both listed", a, "render_moments", b, "quad alone", c, "6 sigma", 6.0 * np.sqrt(va + vb), 6.0 * np.sqrt(vc + vb))
    assert (b > 0).all()
    assert (np.abs(a - b) <= 6.0 * np.sqrt(va + vb)).all(), (a, b, 6.0 * np.sqrt(va + vb))
    assert (np.abs(c - b) > 6.0 * np.sqrt(vc + vb)).all() and (c < b).all(), (c, b, 6.0 * np.sqrt(vc + vb))


@pytest.mark.parametrize("heuristic", HEURISTICS)
def test_the_floor_under_a_sphere_has_its_analytic_value(rl, heuristic):
    """nee_spheres_model.under_a_sphere at 37 x 19, S = 64: rho E (r / h)^2 = 0.5 within 6 sigma of the render's own sq."""
    world, cam = sm.under_a_sphere(rl, 64, width=W0)
    r = rl.render_nee_mis(cam, world, [], 1, T, heuristic, sphere_lights=[sm.UNDER])
    mean, v = _frame_mean(r.moments())
    print(heuristic, "mean", mean, "6 sigma", 6.0 * np.sqrt(v), "analytic", sm.UNDER_ANSWER)
    assert (v > 0).all() and (np.abs(mean - sm.UNDER_ANSWER) <= 6.0 * np.sqrt(v)).all(), (mean, 6.0 * np.sqrt(v))


# ----------------------------------------------------------------------------- 12. the cap
@pytest.mark.parametrize("name", INPUTS)
def test_no_sample_exceeds_what_the_lights_emit(rl, name):
    """S = 1: sq is the square of one sample, at most B = max(background) + Emax (1 + (D - 1) (L + Ls) (K + 1)) (the MIS suite's test says
    why; a sphere light's terms obey the same two bounds wl kf <= 1 and wb <= 1)."""
    world, quads, balls, _ = _input(rl, name)
    Emax = max([float(rl.pack_sphere_lights(balls)[:, 4:7].max())] + ([float(rl.pack_lights(quads)[:, 9:12].max())] if quads else []))
    for K, D in ((1, 6), (3, 50)):
        cam = _camera(rl, world, 1, D)
        B = max(float(v) for v in cam.c.background) + Emax * (1.0 + (D - 1) * (len(quads) + len(balls)) * (K + 1))
        for h in HEURISTICS:
            for F in (0, 1):
                r = _free_frame(rl, world, cam, quads, balls, K, h, F=F)[0]
                assert np.isfinite(r.sq).all() and (r.sq <= B * B).all(), (name, K, D, h, F, float(r.sq.max()), B * B)
                assert _same(r.sq, r.sums * r.sums)
