"""CPU tier: the definition of the NEE path renders with sphere lights (tests/nee_spheres_model.py) held on its own, before any render is
compared with it (tests/test_gpu_render_nee_spheres.py): the two weights as a partition of one at crossings of a sphere, a vertex inside
a sphere, and a floor point whose answer needs no path tracer."""
import math

import nee_spheres_model as sm
import numpy as np
import pytest
from ao_model import Stream
from direct_model import SEG_TMAX

HEURISTICS = (sm.BALANCE, sm.POWER)


def test_the_weights_of_a_pair_sum_to_one_at_crossings_of_a_sphere():
    """Scattered rays from floor points that do cross a sphere light: the crossing's own g (co and A in it) gives wl / g + wb = 1 to one
    ulp of 1, as for a quad (nee_mis_model's test says why one ulp), and wl kf <= 1, wb <= 1.  A light point placed where the ray crosses
    (wu = the crossing's outward normal) has the crossing's geometry term up to the rounding of its few operations: the two strategies
    weigh the SAME pair of densities."""
    rng = np.random.default_rng(3)
    ulp = 2.0 ** -52
    n = (0.0, 1.0, 0.0)
    seen = 0
    for sphere in ((0.0, 4.0, 0.0, 2.0, 4.0, 4.0, 4.0), (1.0, 0.75, -2.0, 0.7, 1.0, 2.0, 3.0), (0.0, 1.0 + 1e-9, 0.0, 1.0, 9.0, 9.0, 9.0)):
        A = sm.area(sphere[3])
        assert A == (4.0 * math.pi) * (sphere[3] * sphere[3])
        for _ in range(4000):
            x = (float(rng.uniform(-3, 3)), 0.0, float(rng.uniform(-3, 3)))
            w = tuple(float(v) for v in rng.normal(size=3) * rng.uniform(0.1, 3.0))
            d, g = sm.sphere_crossing(sphere, A, x, n, w)
            if g is None:
                continue
            seen += 1
            assert g > 0.0 and w[1] > 0.0
            for K in (1, 3):
                kf = 1.0 / (math.pi * K)
                for h in HEURISTICS:
                    wl, wb = sm.light_weight(g, kf, h), sm.scatter_weight(g, kf, h)
                    assert abs(wl / g + wb - 1.0) <= ulp, (sphere, x, w, g, h)
                    assert 0.0 <= wb <= 1.0 and 0.0 <= wl * kf <= 1.0 + ulp
            # the same point as a light point
            y = tuple(x[i] + d[i] for i in range(3))
            wu = tuple((y[i] - sphere[i]) / sphere[3] for i in range(3))
            d2, g2 = sm.sphere_point(sphere, A, x, n, wu)
            assert g2 is not None and abs(g2 - g) <= 1e-9 * g
    assert seen > 400


def test_a_vertex_inside_a_sphere_gets_nothing_from_it():
    """Every point of the sphere faces away from a vertex inside it (co < 0), and the near root of any ray from inside lies behind the
    vertex (t < 0): neither strategy makes a candidate, so nothing is traced.  (The reference's DiffuseLight emits from both sides: the one
    configuration in which the definition's expectation is not ray_color's.)"""
    rng = np.random.default_rng(4)
    sphere = (0.5, 1.0, -0.5, 3.0, 2.0, 2.0, 2.0)
    A = sm.area(3.0)
    for _ in range(3000):
        v = rng.normal(size=3)
        x = tuple(float(sphere[i] + v[i] / np.linalg.norm(v) * rng.uniform(0.0, 2.999)) for i in range(3))
        nv = rng.normal(size=3)
        n = tuple(float(c) for c in nv / np.linalg.norm(nv))
        u = rng.normal(size=3)
        wu = tuple(float(c) for c in u / np.linalg.norm(u))
        assert sm.sphere_point(sphere, A, x, n, wu) == (None, None)
        w = tuple(float(c) for c in rng.normal(size=3) * rng.uniform(0.1, 3.0))
        assert sm.sphere_crossing(sphere, A, x, n, w) == (None, None)


def test_the_far_side_costs_draws_but_no_trace(rl, oracle):
    """A path's words with a sphere light: every sphere point is drawn (4 words per try) whether or not it counts, and about half of them
    face away from a vertex far from the sphere."""
    world, cam = sm.under_a_sphere(rl, 4, width=3)
    info = sm.new_info()
    a, b, words, rays = sm.pixel(oracle, world.desc, world.materials(), cam.c, 1, 1, np.zeros((0, 12)), rl.pack_sphere_lights([sm.UNDER]), 8, SEG_TMAX, info=info)
    assert info["sphere_drawn"] == 4 * 8 and 0 < info["sphere_skipped"] < info["sphere_drawn"]
    # 4 camera rays, the counted sphere points, 4 scattered rays and the connections made
    made = info["sphere_scatter_free"] + info["sphere_scatter_occluded"]
    assert rays == 4 + (info["sphere_drawn"] - info["sphere_skipped"]) + 4 + made
    assert words >= 4 * (6 + 8 * 4 + 4) and words % 2 == 0  # get_ray's 3 draws, 8 points and the scatter of at least one try each
    assert info["quad_light_free"] == info["quad_scatter_free"] == 0


@pytest.mark.parametrize("heuristic", HEURISTICS)
def test_the_floor_under_a_sphere_has_its_analytic_value(rl, oracle, heuristic):
    """sm.under_a_sphere: a grey floor (rho = 0.5) seen at the point 4 under the centre of an r = 2, E = 4 sphere light that is not
    geometry, max_depth 2, black background.  The radiance towards the camera is rho E (r / h)^2 = 0.5.  12 x 8 pixels x S = 16
    = 1536 samples of the model (a few seconds), K = 1.  Pixels have independent streams, so the mean over the P pixels has variance (sum of
    their variance_of_mean) / P^2, taken from the model's own sq; the bound is 6 sigma of that.  One sample is at most 2 rho E = 4: the light
    point's term is at most rho E (wl kf <= 1) and the scattered ray's, at another point of the sphere, at most rho E (wb <= 1)."""
    S = 16
    world, cam = sm.under_a_sphere(rl, S)
    su, sq, words, rays, info = sm.frame(oracle, world.desc, world.materials(), cam.c, np.zeros((0, 12)), rl.pack_sphere_lights([sm.UNDER]), 1, SEG_TMAX,
                                         heuristic=heuristic)
    P = su.shape[0] * su.shape[1]
    assert P * S == 1536 and info["sphere_drawn"] == P * S
    mean = (su / S).reshape(-1, 3).sum(0) / P
    v = ((sq - su * su / S) / (S - 1) / S).reshape(-1, 3).sum(0)
    six_sigma = 6.0 * np.sqrt(v) / P
    print("heuristic", heuristic, "mean", mean, "6 sigma", six_sigma, "analytic", sm.UNDER_ANSWER, "largest sample", info["largest"], info)
    assert sm.UNDER_ANSWER == 0.5
    assert (six_sigma > 0).all() and (np.abs(mean - sm.UNDER_ANSWER) <= six_sigma).all(), (mean, six_sigma)
    assert info["largest"] <= 2.0 * sm.ALBEDO * sm.UNDER[2] * (1.0 + 1e-12)
    assert info["sphere_light_free"] > 0 and info["sphere_scatter_free"] > 0 and info["sphere_light_occluded"] == info["sphere_scatter_occluded"] == 0


def test_unit_sphere_of_the_stream_is_a_unit_vector(oracle):
    """What the light points are made of: Stream.unit_sphere() (the AO model's, Marsaglia's draw) returns unit vectors and takes 4 words
    per try."""
    rng = Stream(oracle, 9, 5)
    for _ in range(50):
        before = rng.words()
        w = rng.unit_sphere()
        assert abs(float(np.dot(w, w)) - 1.0) <= 4e-16 and (rng.words() - before) % 4 == 0 and rng.words() > before
