"""CPU tier: known answers of the ambient-occlusion definition (tests/ao_model.py) on its own — the model the GPU tests compare the
renders with (tests/test_gpu_render_ao.py) is itself held to two scenes whose answer needs no computation."""
import ao_model
import numpy as np

K = 4
INF = float("inf")


def test_a_lone_convex_body_occludes_none_of_its_own_ambient_rays(rl, oracle):
    """One unit sphere, no ground, R = inf: open == K * hits on every pixel.  (The ambient ray's spurious near root on its own sphere is
    about 1e-16 / (2 cos theta), below tmin = 1e-10 unless cos theta < 1e-6.)"""
    world, cam = ao_model.known_answer_cases(rl)["lone_sphere"]
    assert (cam.c.image_width, cam.c.image_height, cam.c.samples_per_pixel) == (12, 8, 2)
    op, hits, words = ao_model.frame(oracle, world.desc, cam.c, K, INF)
    assert 0 < hits.sum() < 2 * 12 * 8, hits  # the sphere is in the frame and does not fill it
    assert np.array_equal(op, K * hits), (op, hits)
    # get_ray without defocus draws 3 f64 = 6 words per sample; every unit vector at least 2 uniforms = 4 words
    assert words >= 6 * 2 * 12 * 8 + 4 * K * int(hits.sum())


def test_from_inside_a_sphere_every_ambient_ray_is_occluded(rl, oracle):
    """The camera at the centre of one sphere of radius 5, R = inf: hits == S and open == 0 everywhere."""
    world, cam = ao_model.known_answer_cases(rl)["inside"]
    op, hits, _ = ao_model.frame(oracle, world.desc, cam.c, K, INF)
    assert np.array_equal(hits, np.full((8, 12), 2, dtype=np.uint32)), hits
    assert not op.any(), op


def test_a_radius_short_of_the_wall_opens_every_ray_and_calls_add(rl, oracle):
    """Inside the radius-5 sphere an ambient ray travels at most a diameter and, leaving the wall inwards, more than 0 — with R = 1e-3 only
    rays within 1e-4 of the tangent plane could end in the wall again: open == K * hits.  And (F = 0, S = 2) = (F = 0, S = 1) + (F = 1, S = 1)."""
    world, cam = ao_model.known_answer_cases(rl)["inside"]
    op, hits, words = ao_model.frame(oracle, world.desc, cam.c, K, 1e-3)
    assert np.array_equal(op, K * hits) and hits.min() == 2
    p = cam.params
    p.samples_per_pixel = 1
    one = rl.Camera(p)
    a = ao_model.frame(oracle, world.desc, one.c, K, 1e-3, first_sample=0)
    b = ao_model.frame(oracle, world.desc, one.c, K, 1e-3, first_sample=1)
    assert np.array_equal(a[0] + b[0], op) and np.array_equal(a[1] + b[1], hits) and a[2] + b[2] == words
