"""CPU tier: the NEE path definition (tests/nee_model.py) held on its own, before any render is compared with it
(tests/test_gpu_render_nee.py): scenes whose answer needs no path tracer, and the word count of a two-vertex path by hand."""
import math

import direct_model as dm
import nee_model as nm
import numpy as np
import pytest
from ao_model import Stream, get_ray

E = nm.CEILING[3]
BG = nm.BACKGROUND


def _frame(rl, oracle, name, max_depth, lights, K, spp=1):
    world, cam = nm.known_answer_cases(rl, max_depth, spp)[name]
    assert (cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel, cam.c.max_depth) == (12, 8, spp, max_depth)
    su, sq, words, rays = nm.frame(oracle, world.desc, world.materials(), cam.c, rl.pack_lights(lights), K, dm.SEG_TMAX)
    return world, cam, su, sq, words, rays


def _first_hits(oracle, world, cam):
    """-> per pixel the material kind the camera ray of sample 0 meets (-1: none), from the oracle alone."""
    kinds = np.full((8, 12), -1)
    mats = world.materials()
    for y in range(8):
        for x in range(12):
            rng = Stream(oracle, cam.c.seed, x * 12 + y)
            o, d, time = get_ray(cam.c, rng, x, y)
            hit = oracle.rtiow_hit(world.desc, o, d, time, 1e-10, nm.INF)
            if hit is not None:
                kinds[y, x] = int(mats[hit["mat"]]["kind"])
    return kinds


def test_max_depth_one_is_emission_or_background_and_draws_no_light_point(rl, oracle):
    """One vertex: the camera ray's emission or the background; rule 3 needs i < max_depth, so no light point is drawn whatever K is: the
    words are get_ray's 6 per sample and the floor's Lambertian scatter (drawn, as ray_color draws it, and unused)."""
    world, cam, su, sq, words, rays = _frame(rl, oracle, "ceiling", 1, [nm.CEILING], 1)
    _, _, su7, sq7, words7, rays7 = _frame(rl, oracle, "ceiling", 1, [nm.CEILING], 7)
    assert su.tobytes() == su7.tobytes() and sq.tobytes() == sq7.tobytes() and words == words7 and rays == rays7 == 96
    kinds = _first_hits(oracle, world, cam)
    floor, lamp, sky = kinds == nm.MAT_LAMBERTIAN, kinds == nm.MAT_DIFFUSE_LIGHT, kinds == -1
    assert floor.sum() > 0 and lamp.sum() > 0 and floor.sum() + lamp.sum() + sky.sum() == 96
    assert not su[floor].any() and (su[lamp] == np.array(E)).all() and (su[sky] == np.array(BG)).all()
    assert (sq[lamp] == np.array(E) ** 2).all()
    # the words, by hand: 6 per sample, and UnitSphere's pairs at the floor pixels from word 6 on
    by_hand = 0
    for y, x in np.argwhere(kinds >= -1):
        rng = Stream(oracle, cam.c.seed, int(x) * 12 + int(y))
        get_ray(cam.c, rng, int(x), int(y))
        assert rng.words() == 6
        if floor[y, x]:
            rng.unit_sphere()
        by_hand += rng.words()
    assert words == by_hand > 6 * 96


def test_a_light_facing_away_adds_nothing_and_the_words_of_a_two_vertex_path(rl, oracle):
    """The floor alone, a light under it (cs < 0 at every point), max_depth = 2.  By hand for every floor pixel: get_ray takes 6 words,
    the L K = 3 light points 12 more whether or not they count, the scatter draws UnitSphere from word 18 on, and the scattered ray, which
    leaves the only surface upwards, meets nothing: c = (1 * 0.5) * background, two path rays, no segment."""
    K = 3
    world, cam, su, sq, words, rays = _frame(rl, oracle, "open", 2, nm.LIGHT_BELOW, K)
    kinds = _first_hits(oracle, world, cam)
    floor = kinds == nm.MAT_LAMBERTIAN
    assert 0 < floor.sum() < 96 and (kinds[~floor] == -1).all()
    assert rays == 96 + int(floor.sum())
    want = np.array([(1.0 * nm.ALBEDO) * b for b in BG])
    assert (su[floor] == want).all() and (sq[floor] == want * want).all() and (su[~floor] == np.array(BG)).all()
    by_hand = 0
    for y, x in np.argwhere(kinds >= -1):
        rng = Stream(oracle, cam.c.seed, int(x) * 12 + int(y))
        get_ray(cam.c, rng, int(x), int(y))
        if floor[y, x]:
            rng.i += 2 * K  # a, b of every light point: one u64 each
            assert rng.words() == 6 + 4 * K
            rng.unit_sphere()
        by_hand += rng.words()
    assert words == by_hand
    # and without the light points in the stream the scatters differ: the draws are really taken
    _, _, su1, _, words1, _ = _frame(rl, oracle, "open", 2, nm.LIGHT_BELOW, 1)
    assert su1.tobytes() == su.tobytes() and words1 != words


def test_the_light_is_counted_once_directly_and_never_after_a_lambertian_vertex(rl, oracle):
    """The floor under a DiffuseLight ceiling that is also the one listed light, S = 1.  A camera ray that meets the ceiling gives E once
    and stops.  A floor pixel's path: vertex 1 samples the light, its scattered ray meets the ceiling at vertex 2, whose emission is NOT
    counted (the connection stood for it): c is the connection alone, ((1 * 0.5) * direct) * kf with `direct` the direct-lighting
    model's sum for the same pixel, sample and lights (tests/direct_model.py draws the same points from the same words).  max_depth 2 and
    3 agree: the path has ended on the light."""
    K = 2
    world, cam, su, sq, words, rays = _frame(rl, oracle, "ceiling", 3, [nm.CEILING], K)
    _, _, su2, _, _, _ = _frame(rl, oracle, "ceiling", 2, [nm.CEILING], K)
    assert su.tobytes() == su2.tobytes()
    kinds = _first_hits(oracle, world, cam)
    floor, lamp = kinds == nm.MAT_LAMBERTIAN, kinds == nm.MAT_DIFFUSE_LIGHT
    assert floor.sum() > 0 and lamp.sum() > 0
    assert (su[lamp] == np.array(E)).all()
    kf = 1.0 / (math.pi * K)
    lit = 0
    for y, x in np.argwhere(floor):
        direct, unshadowed, hits, _, traced = dm.pixel(oracle, world.desc, cam.c, int(x), int(y), rl.pack_lights([nm.CEILING]), K, dm.SEG_TMAX)
        assert hits == 1 and traced == K and direct == unshadowed  # nothing between floor and ceiling; T < 1 keeps the ceiling itself out
        want = [((1.0 * nm.ALBEDO) * direct[ch]) * kf for ch in range(3)]
        assert su[y, x].tolist() == want, (x, y, su[y, x], want)
        lit += want[0] > 0.0
        assert all(want[ch] < nm.ALBEDO * E[ch] for ch in range(3))  # far from what counting the ceiling at vertex 2 as well would give
    assert lit == floor.sum()


def test_other_material_kinds_are_refused(rl, oracle):
    world = rl.World.build(lambda b: b.list([b.sphere((0.0, 0.0, -3.0), 1.0, b.metal((0.8, 0.8, 0.8), 0.1))]))
    cam = rl.Camera(rl.CameraParams(aspect_ratio=1.0, image_width=3, samples_per_pixel=1, max_depth=3, vfov=30.0))
    with pytest.raises(ValueError):
        nm.pixel(oracle, world.desc, world.materials(), cam.c, 1, 1, rl.pack_lights(nm.LIGHT_BELOW), 1)
