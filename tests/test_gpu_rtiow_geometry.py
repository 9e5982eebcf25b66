"""GPU tier: Hittable::hit (World.hit_rays) and Texture::value (World.texture_values) held to the geometric model and the NumPy texture
restatements of tests/test_rtiow_geometry_model.py, which share nothing with the oracle, the host mirror or the kernels.

Every scene of the CPU tier goes through hit_rays three ways: with `stats` (the reference-order kernel), without (the fast walk where it
applies) and with set_fast_traversal(False).  The three must be the same bytes; the record must meet the model under the same bounds,
margins and caps as the oracle did, the directed cases with ==; and, ray by ray, t, p and normal must equal oracle.rtiow_hit bit for
bit, the existing convention, so that the two comparisons cannot drift apart.  The model's results are computed once per scene and shared
by the three routes."""
import numpy as np
import pytest

import test_rtiow_geometry_model as M

pytestmark = pytest.mark.gpu
CHUNK = 8  # random scenes per case: the model's mpmath arithmetic is a third of a second per scene
WORST = {}  # field -> largest observed / bound over the cases that have run


@pytest.fixture(autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


@pytest.fixture(scope="module", autouse=True)
def _release_the_worlds():
    """the worlds and model results are built once per module; their device scenes go when the module is done"""
    yield
    M._scene_cache.clear()
    M._directed_cache.clear()


def three_routes(rl, world, o, d, times, tmin, tmax):
    """-> the RTIOW_HIT records, after asserting that the three routes return the same bytes, count every ray, draw nothing and flag nothing"""
    o, d = np.ascontiguousarray(o, dtype=np.float64), np.ascontiguousarray(d, dtype=np.float64)
    st = {}
    counted = world.hit_rays(o, d, times=times, tmin=tmin, tmax=tmax, stats=st)
    assert st["rays"] == o.shape[0] and st["rng_words"] == 0 and st["flagged"] == 0, st
    free = world.hit_rays(o, d, times=times, tmin=tmin, tmax=tmax)
    rl.api.set_fast_traversal(False)
    try:
        off = world.hit_rays(o, d, times=times, tmin=tmin, tmax=tmax)
        assert rl.api.last_query()["kernel"] == "reference"
    finally:
        rl.api.set_fast_traversal(True)
    assert counted.tobytes() == free.tobytes() and counted.tobytes() == off.tobytes()
    return counted


def equal_the_oracle(oracle, world, h, o, d, time, tmin, tmax, where):
    ref = oracle.rtiow_hit(world.desc, o, d, time, tmin, tmax)
    if ref is None:
        assert h["hit"] == 0, where
        return
    assert h["hit"] == 1 and h["material"] == ref["mat"] and bool(h["front_face"]) == ref["front"], (where, h, ref)
    assert h["t"] == ref["t"] and np.array_equal(h["p"], ref["p"]) and np.array_equal(h["normal"], ref["normal"]), (where, h, ref)


def meet_the_model(rl, oracle, case, with_bvh, where):
    """one scene: -> (rays left out, hits compared)"""
    world, model, tags, (o, d, times), (tmin, tmax), results = case
    hits = three_routes(rl, world, o, d, times, tmin, tmax)
    left = n_hit = 0
    for i, res in enumerate(results):
        equal_the_oracle(oracle, world, hits[i], o[i], d[i], times[i], tmin, tmax, (where, i))
        if not M.use_ray(res, with_bvh):
            left += 1
            continue
        M.compare(res, M.gpu_record(hits[i], tags), WORST, (where, i))
        n_hit += res["hit"]
    return left, n_hit


def _report(what):
    print(what + "; worst observed / bound so far " + " ".join(f"{f} {WORST.get(f, 0.0):.3f}" for f in M.FIELDS))


@pytest.mark.parametrize("with_bvh", [False, True], ids=["list", "bvh"])
@pytest.mark.parametrize("chunk", range(M.N_SCENES // CHUNK))
def test_random_scenes_meet_the_model(rl, oracle, with_bvh, chunk):
    """(a) and (b) of the CPU tier"""
    seeds = (M.SEEDS_B if with_bvh else M.SEEDS_A)[chunk * CHUNK:(chunk + 1) * CHUNK]
    per_scene = []
    for seed in seeds:
        left, n_hit = meet_the_model(rl, oracle, M.random_case(rl, seed, with_bvh), with_bvh, seed)
        assert n_hit >= M.MIN_HITS, (seed, n_hit)
        per_scene.append((seed, left, n_hit))
    _report(f"seeds {seeds[0]}..{seeds[-1]}: left out {sum(s[1] for s in per_scene)}, fewest compared hits {min(s[2] for s in per_scene)}")


@pytest.mark.parametrize("with_bvh", [False, True], ids=["list", "bvh"])
def test_the_seeds_keep_the_caps(rl, with_bvh):
    """the 2 % cap and the 100-hit floor are conditions on the seeds, decided by the model alone (cached from the cases above)"""
    seeds = M.SEEDS_B if with_bvh else M.SEEDS_A
    per_scene = []
    for seed in seeds:
        results = M.random_case(rl, seed, with_bvh)[5]
        used = [r for r in results if M.use_ray(r, with_bvh)]
        per_scene.append((seed, len(results) - len(used), sum(r["hit"] for r in used)))
    left_out = M.check_counts(per_scene, len(seeds) * M.N_RAYS)
    _report(f"{len(seeds) * M.N_RAYS} rays, {left_out} left out")


def test_thin_turned_and_moving_children_of_a_bvh(rl, oracle):
    case = M.box_case(rl)
    left, n_hit = meet_the_model(rl, oracle, case, True, "box")
    n = len(case[5])
    assert left <= M.MAX_LEFT_OUT * n and n_hit >= 0.6 * n, (left, n_hit, n)
    _report(f"box scene: {n} rays, {left} left out, {n_hit} hits")


@pytest.mark.parametrize("k", range(len(M.DIRECTED)), ids=[c["name"] for c in M.DIRECTED])
def test_directed_cases(rl, oracle, k):
    """(c): exact records, =="""
    case = M.DIRECTED[k]
    world, model, tags = M.directed_world(rl, k)
    o, d = np.array([r[0] for r in case["rays"]]), np.array([r[1] for r in case["rays"]])
    hits = three_routes(rl, world, o, d, None, case["tmin"], case["tmax"])
    for i in range(len(hits)):
        equal_the_oracle(oracle, world, hits[i], o[i], d[i], 0.0, case["tmin"], case["tmax"], (case["name"], i))
        if not hits[i]["hit"]:
            assert hits[i]["t"] == M.INF
    M.check_directed(case, model, [M.gpu_record(h, tags) for h in hits])


# ----------------------------------------------------------------------------- textures
@pytest.fixture(scope="module")
def texture_table(rl):
    """-> (world, texture ids [n], uv [n, 2], p [n, 3], expected rgb [n, 3]) over every image and checker of the CPU tier's tables"""
    world, images, checkers = M.texture_world(rl)
    tex, uv, p, want = [], [], [], []
    for tid, img in images:
        h, w = img.shape[:2]
        for u in M.image_coordinates(w):
            for v in M.image_coordinates(h):
                tex.append(tid), uv.append((u, v)), p.append((0.0, 0.0, 0.0)), want.append(M.image_value(img, u, v))
    for tid, tree in checkers:
        for q in M.checker_points(tree[0][0]):
            tex.append(tid), uv.append((0.25, 0.75)), p.append(tuple(q)), want.append(M.checker_leaf(tree, q))
    return world, np.array(tex, dtype=np.uint32), np.array(uv), np.array(p), np.array(want)


@pytest.mark.parametrize("batch", [1, 64, 65])
def test_texture_values_equal_the_restatements(rl, texture_table, batch):
    """(d): Image (texture.rs:63-81: clamp, v flipped, Rust's saturating `as u32` with NaN -> texel column / row 0, float32 texels widened)
    and Checker (texture.rs:42-54: floor, the sign-keeping %), nested two deep: array_equal, in batches of 1, 64 and 65"""
    world, tex, uv, p, want = texture_table
    assert not np.isnan(want).any() and np.isnan(uv).any()
    for a in range(0, tex.shape[0], batch):
        got = world.texture_values(tex[a:a + batch], uv[a:a + batch], p[a:a + batch])
        assert np.array_equal(got, want[a:a + batch]), (a, tex[a:a + batch], uv[a:a + batch], p[a:a + batch], got, want[a:a + batch])
