"""CPU tier: the definition of the NEE path renders with multiple importance sampling (tests/nee_mis_model.py) held on its own, before any
render is compared with it (tests/test_gpu_render_nee_mis.py): scenes whose answer needs no path tracer, the relation to nee_model, and
the two weights as a partition of one."""
import math

import nee_mis_model as mm
import nee_model as nm
import numpy as np
import pytest
from direct_model import SEG_TMAX

E = np.array(nm.CEILING[3])
HEURISTICS = (mm.BALANCE, mm.POWER)
_cache = {}


def _mis(rl, oracle, name, max_depth, lights, K, spp, heuristic):
    key = ("mis", name, max_depth, repr(lights), K, spp, heuristic)
    if key not in _cache:
        world, cam = nm.known_answer_cases(rl, max_depth, spp)[name]
        _cache[key] = mm.frame(oracle, world.desc, world.materials(), cam.c, rl.pack_lights(lights), K, SEG_TMAX, heuristic=heuristic)
    return _cache[key]


def _nee(rl, oracle, name, max_depth, lights, K, spp):
    key = ("nee", name, max_depth, repr(lights), K, spp)
    if key not in _cache:
        world, cam = nm.known_answer_cases(rl, max_depth, spp)[name]
        _cache[key] = nm.frame(oracle, world.desc, world.materials(), cam.c, rl.pack_lights(lights), K, SEG_TMAX)
    return _cache[key]


def _first_hit_kinds(rl, oracle, name, spp):
    """-> [spp, 8, 12] the material kind every sample's camera ray meets (-1: none), from the oracle alone."""
    key = ("kinds", name, spp)
    if key not in _cache:
        world, cam = nm.known_answer_cases(rl, 2, spp)[name]
        _cache[key] = mm.first_hit_kinds(oracle, world, cam.c)
    return _cache[key]


def _variance_of_mean(su, sq, S):
    return (sq - su * su / S) / (S - 1) / S


@pytest.mark.parametrize("heuristic", HEURISTICS)
def test_a_light_no_ray_reaches_leaves_nee_models_bytes(rl, oracle, heuristic):
    """The floor alone with a light under it: cs < 0 at every light point, so none counts, and a scattered ray, which leaves the floor
    upwards, crosses the light's plane at t < 0.  Nothing is weighted and nothing is connected: nee_model's bytes, words and rays."""
    K, S = 3, 2
    su, sq, words, rays, info = _mis(rl, oracle, "open", 3, nm.LIGHT_BELOW, K, S, heuristic)
    su0, sq0, words0, rays0 = _nee(rl, oracle, "open", 3, nm.LIGHT_BELOW, K, S)
    assert su.tobytes() == su0.tobytes() and sq.tobytes() == sq0.tobytes() and (su > 0).any()
    assert words == words0 and rays == rays0
    assert info["counted"] == 0 and info["made"] == 0 and info["free"] == 0


@pytest.mark.parametrize("heuristic", HEURISTICS)
def test_under_a_ceiling_light_the_floor_has_its_analytic_value_and_less_variance_than_nee(rl, oracle, heuristic):
    """The floor under the DiffuseLight CEILING, which is also the one listed light; max_depth 2, S = 16, K = 1.  Every scattered ray of a
    floor vertex crosses the ceiling and nothing stands between.  The radiance a floor point sends to the camera is ALBEDO * E (the form
    factor of the 2000 x 2000 quad at height 4 falls short of 1 by about 1e-5, far inside sigma).  Pixels have independent streams, so the
    mean over P floor pixels has variance (sum of their variance_of_mean) / P^2, taken from the model's own sq.  Uniform area sampling
    alone (nee_model) draws points up to 1400 units away on this light: its variance over the same pixels is far larger (the margin
    measured is about 6e3)."""
    S = 16
    su, sq, words, rays, info = _mis(rl, oracle, "ceiling", 2, [nm.CEILING], 1, S, heuristic)
    su0, sq0, words0, rays0 = _nee(rl, oracle, "ceiling", 2, [nm.CEILING], 1, S)
    kinds = _first_hit_kinds(rl, oracle, "ceiling", S)
    assert words == words0  # the scattered-ray strategy draws nothing
    vertices = int((kinds == nm.MAT_LAMBERTIAN).sum())  # max_depth 2: the first vertex alone can sample
    assert vertices > 0 and info["made"] == vertices == info["free"]
    assert rays == rays0 + info["made"]
    floor = (kinds == nm.MAT_LAMBERTIAN).all(axis=0)  # pixels whose every sample starts on the floor
    P = int(floor.sum())
    assert P >= 36
    mean = (su[floor] / S).sum(0) / P
    v, v0 = _variance_of_mean(su, sq, S)[floor], _variance_of_mean(su0, sq0, S)[floor]
    six_sigma = 6.0 * np.sqrt(v.sum(0)) / P
    print("heuristic", heuristic, "floor pixels", P, "connections", info["made"], "mean", mean, "6 sigma", six_sigma, "analytic", nm.ALBEDO * E,
          "largest sample", info["largest"], "variance MIS", v.sum(), "NEE", v0.sum(), "NEE mean", (su0[floor] / S).sum(0) / P)
    assert (np.abs(mean - nm.ALBEDO * E) <= six_sigma).all(), (mean, six_sigma)
    assert 0.0 < v.sum() < v0.sum()
    assert info["largest"] <= E.max() * (1.0 + 1e-12)  # a light's own pixel, or one vertex: ALBEDO * E * (light share + scattered share)


def test_max_depth_two_and_three_agree_under_the_ceiling(rl, oracle):
    """The scattered ray of a floor vertex ends on the ceiling, whose emission is not counted a second time: the path is over."""
    for heuristic in HEURISTICS:
        a = _mis(rl, oracle, "ceiling", 2, [nm.CEILING], 2, 2, heuristic)
        b = _mis(rl, oracle, "ceiling", 3, [nm.CEILING], 2, 2, heuristic)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2:4] == b[2:4] and a[4] == b[4]
        assert a[4]["made"] > 0


def test_the_two_heuristics_differ_and_both_differ_from_nee(rl, oracle):
    bal = _mis(rl, oracle, "ceiling", 2, [nm.CEILING], 2, 2, mm.BALANCE)
    pw = _mis(rl, oracle, "ceiling", 2, [nm.CEILING], 2, 2, mm.POWER)
    nee = _nee(rl, oracle, "ceiling", 2, [nm.CEILING], 2, 2)
    assert bal[0].tobytes() != pw[0].tobytes() and bal[0].tobytes() != nee[0].tobytes() and pw[0].tobytes() != nee[0].tobytes()
    assert bal[2] == pw[2] == nee[2] and bal[3] == pw[3]  # words and rays do not depend on the weights


def test_the_weights_of_a_pair_sum_to_one():
    """A light point's term is E * wl * kf = E * g * kf * (the light strategy's weight), so that weight is wl / g; the scattered ray's is
    wb.  With q = g * kf they are 1 / (1 + q^b) and q^b / (1 + q^b), b = 1 or 2, over the SAME rounded denominator.  wl / g carries two
    roundings of relative size 2^-53 on a value <= 1, wb one, and the sum is rounded to a double next to 1: |wl / g + wb - 1| <= 2^-52,
    one ulp of 1.  (The unweighted terms themselves are equal by construction: (wl * kf) / wb is 1 for balance and 1 / q for power.)"""
    ulp = 2.0 ** -52
    for K in (1, 2, 3, 7):
        kf = 1.0 / (math.pi * K)
        for e in np.linspace(-40.0, 40.0, 321):
            for mant in (1.0, 1.1, 1.7320508, 1.9999999):
                g = mant * 10.0 ** float(e)
                for h in HEURISTICS:
                    wl, wb = mm.light_weight(g, kf, h), mm.scatter_weight(g, kf, h)
                    assert abs(wl / g + wb - 1.0) <= ulp, (K, g, h, wl, wb)
                    # one weighted light sample is at most thr tex E (up to the rounding of wl * kf), the scattered-ray term thr E per light
                    assert 0.0 <= wb <= 1.0 and 0.0 <= wl * kf <= 1.0 + ulp


def test_other_material_kinds_and_heuristics_are_refused(rl, oracle):
    world = rl.World.build(lambda b: b.list([b.sphere((0.0, 0.0, -3.0), 1.0, b.metal((0.8, 0.8, 0.8), 0.1))]))
    cam = rl.Camera(rl.CameraParams(aspect_ratio=1.0, image_width=3, samples_per_pixel=1, max_depth=3, vfov=30.0))
    with pytest.raises(ValueError):
        mm.pixel(oracle, world.desc, world.materials(), cam.c, 1, 1, rl.pack_lights(nm.LIGHT_BELOW), 1)
    floor, fcam = nm.known_answer_cases(rl, 2)["open"]
    with pytest.raises(ValueError):
        mm.pixel(oracle, floor.desc, floor.materials(), fcam.c, 6, 7, rl.pack_lights(nm.LIGHT_BELOW), 1, heuristic=2)
