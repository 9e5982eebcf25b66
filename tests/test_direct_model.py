"""CPU tier: the direct-lighting definition (tests/direct_model.py) held on its own, before any render is compared with it
(tests/test_gpu_render_direct.py): (a) its geometry term against the textbook form with normalised vectors, (b) the mean of that term
over a light against the analytic form factor of a rectangle, (c) three scenes whose answer needs no computation."""
import math

import direct_model as dm
import numpy as np

K = 3


# ----------------------------------------------------------------------------- (a) the geometry term, the long way
def test_the_geometry_term_is_cos_cos_area_over_distance_squared():
    """g = (cs * cl) / (d2 * d2) with cs = n.d, cl = |nl.d|, nl = u x v (|nl| = area) is cos(theta) cos(theta_l) area / |d|^2 of the
    normalised vectors.  Both sides are a dozen binary64 roundings from the exact value: a few 1e-15 relative at most (1.3e-15 seen on this
    256 x 256 grid of light points); the bound is 1e-13."""
    light = [0.3, 2.1, -0.7, 1.9, 0.2, -0.4, 0.1, -0.5, 2.6, 1.0, 1.0, 1.0]  # a tilted parallelogram, not axis-aligned
    nl = dm.cross(light[3:6], light[6:9])
    area = math.sqrt(nl[0] * nl[0] + nl[1] * nl[1] + nl[2] * nl[2])
    nlu = [c / area for c in nl]
    p = (0.2, -0.3, 0.4)
    n = (0.48, 0.6, 0.64)  # a unit vector
    assert abs(math.sqrt(sum(c * c for c in n)) - 1.0) < 1e-15
    worst, seen = 0.0, 0
    N = 256
    for i in range(N):
        for j in range(N):
            a, b = (i + 0.5) / N, (j + 0.5) / N
            d, g = dm.geometry(light, nl, p, n, a, b)
            if g is None:
                continue
            dist = math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
            w = [c / dist for c in d]
            cos_s = n[0] * w[0] + n[1] * w[1] + n[2] * w[2]
            cos_l = abs(nlu[0] * w[0] + nlu[1] * w[1] + nlu[2] * w[2])
            long_way = cos_s * cos_l * area / (dist * dist)
            worst = max(worst, abs(g - long_way) / long_way)
            seen += 1
    print("largest relative difference", worst, "over", seen, "light points")
    assert seen > N * N // 2
    assert worst < 1e-13, worst


# ----------------------------------------------------------------------------- (b) the analytic form factor
def _midpoint_mean(N):
    light = [0.0, 1.5, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 3.0, 1.0, 1.0, 1.0]  # Q = (0, 1.5, 0), u = (2, 0, 0), v = (0, 0, 3): a corner over the origin
    nl = dm.cross(light[3:6], light[6:9])
    total = 0.0
    for i in range(N):
        for j in range(N):
            _, g = dm.geometry(light, nl, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0), (i + 0.5) / N, (j + 0.5) / N)
            total += g
    return total / (N * N)


def test_the_mean_over_a_light_is_pi_times_the_analytic_form_factor():
    """A point at the origin with normal +y under the corner of a 2 x 3 rectangle at height 1.5: the mean of g over the light is the
    integral of cos cos_l / r^2 over it, pi times the differential-element-to-rectangle form factor
        F = 1/2pi [a/sqrt(a^2+c^2) atan(b/sqrt(a^2+c^2)) + b/sqrt(b^2+c^2) atan(a/sqrt(b^2+c^2))],  a = 2, b = 3, c = 1.5.
    The midpoint rule is second order: relative errors 4.6e-5, 1.16e-5, 2.9e-6, 7.2e-7 at N = 32, 64, 128, 256.  Asserted: below 2e-6 at
    256 (the observed value with the margin of one more halving step's factor) and a factor of 3.5 .. 4.5 per doubling."""
    a, b, c = 2.0, 3.0, 1.5
    ra, rb = math.sqrt(a * a + c * c), math.sqrt(b * b + c * c)
    F = (a / ra * math.atan(b / ra) + b / rb * math.atan(a / rb)) / (2.0 * math.pi)
    errs = [abs(_midpoint_mean(N) - math.pi * F) / (math.pi * F) for N in (32, 64, 128, 256)]
    print("relative errors at N = 32, 64, 128, 256:", errs)
    assert errs[3] < 2e-6, errs
    for coarse, fine in zip(errs, errs[1:]):
        assert 3.5 <= coarse / fine <= 4.5, errs


# ----------------------------------------------------------------------------- (c) known answers, 12 x 8, S = 2
def test_nothing_between_floor_and_light_direct_is_unshadowed(rl, oracle):
    world, cam = dm.known_answer_cases(rl)["open"]
    assert (cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel) == (12, 8, 2)
    di, un, hits, words, traced = dm.frame(oracle, world.desc, cam.c, dm.LIGHT_ABOVE, K)
    assert 0 < (hits > 0).sum() < 12 * 8, hits  # the floor is in the frame and does not fill it
    assert di.tobytes() == un.tobytes()
    assert (di[hits > 0] > 0.0).all() and not di[hits == 0].any()
    assert traced == K * int(hits.sum())  # every light point is above the floor: none skipped
    assert words == 6 * 2 * 12 * 8 + 4 * K * int(hits.sum())  # get_ray without defocus: 3 f64 = 6 words per sample


def test_a_blocker_between_floor_and_light_leaves_no_direct_light(rl, oracle):
    cases = dm.known_answer_cases(rl)
    world, cam = cases["blocked"]
    open_world, open_cam = cases["open"]
    _, open_un, open_hits, _, _ = dm.frame(oracle, open_world.desc, open_cam.c, dm.LIGHT_ABOVE, K)
    di, un, hits, words, traced = dm.frame(oracle, world.desc, cam.c, dm.LIGHT_ABOVE, K)
    floor = open_hits > 0
    assert floor.any() and (hits >= open_hits).all() and (hits > open_hits).any()  # the floor as before, and the blocker's underside
    assert not di.any()
    assert (un[floor] > 0.0).all() and un[floor].tobytes() == open_un[floor].tobytes()
    assert traced == K * int(open_hits.sum())  # underside hits face away from the light: drawn, skipped
    assert words == 6 * 2 * 12 * 8 + 4 * K * int(hits.sum())


def test_a_light_below_the_floor_adds_nothing_and_still_draws(rl, oracle):
    world, cam = dm.known_answer_cases(rl)["open"]
    _, _, above_hits, _, _ = dm.frame(oracle, world.desc, cam.c, dm.LIGHT_ABOVE, K)
    di, un, hits, words, traced = dm.frame(oracle, world.desc, cam.c, dm.LIGHT_BELOW, K)
    assert not di.any() and not un.any() and traced == 0
    assert np.array_equal(hits, above_hits) and hits.sum() > 0
    assert words == 6 * 2 * 12 * 8 + 4 * 1 * K * int(hits.sum())  # 4 L K words per hit, whatever the geometry term says
