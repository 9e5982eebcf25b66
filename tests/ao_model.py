"""The definition of the ambient-occlusion renders (include/rl_render.h "Ambient-occlusion renders") in Python, on the CPU oracle alone:
draws from oracle.chacha_script, both hits from oracle.rtiow_hit, Camera::get_ray restated from camera.rs:203-230, UnitSphere / UnitDisc as
rand_distr 0.4.3 states them.  Nothing of the library computes here: `desc` and `cam` are the scene description and the derived camera
(rl_rtiow_scene_desc, rl_rtiow_camera) as data.  Not a test module."""
import math

import numpy as np

INF = float("inf")


class Stream:
    """ChaCha8Rng::seed_from_u64(seed) after set_stream(stream), word position 0.  Every draw used here takes one u64 (two words), so draw i
    read as gen::<f64>() and as Uniform::new(-1.0, 1.0) are element i of two scripts of the oracle over the same stream."""

    def __init__(self, oracle, seed, stream):
        self.oracle, self.seed, self.stream, self.i = oracle, seed, stream, 0
        self.f, self.u = np.zeros(0), np.zeros(0)

    def _at(self, kind):
        if self.i >= self.f.size:
            n = max(32, 2 * self.f.size)
            self.f = self.oracle.chacha_script(self.seed, [("set_stream", self.stream)] + [("f64",)] * n)[0][1:]
            self.u = self.oracle.chacha_script(self.seed, [("set_stream", self.stream)] + [("uniform",)] * n)[0][1:]
        v = float((self.f if kind == "f64" else self.u)[self.i])
        self.i += 1
        return v

    def f64(self):
        return self._at("f64")

    def uniform(self):
        return self._at("uniform")

    def words(self):
        return 2 * self.i

    def unit_sphere(self):  # rand_distr 0.4.3 UnitSphere
        while True:
            x1, x2 = self.uniform(), self.uniform()
            s = x1 * x1 + x2 * x2
            if s >= 1.0:
                continue
            f = 2.0 * math.sqrt(1.0 - s)
            return np.array([x1 * f, x2 * f, 1.0 - 2.0 * s])

    def unit_disc(self):  # rand_distr 0.4.3 UnitDisc
        while True:
            x1, x2 = self.uniform(), self.uniform()
            if x1 * x1 + x2 * x2 <= 1.0:
                return x1, x2


def get_ray(cam, rng, x, y):  # camera.rs:203-230
    v = lambda a: np.array(list(a), dtype=np.float64)
    p00, du, dv = v(cam.pixel_00), v(cam.pixel_du), v(cam.pixel_dv)
    center = (p00 + float(x) * du) + float(y) * dv
    px = -0.5 + rng.f64()
    py = -0.5 + rng.f64()
    sample = center + (px * du + py * dv)
    if cam.defocus_angle <= 0.0:
        origin = v(cam.lookfrom)
    else:
        a, b = rng.unit_disc()
        origin = (v(cam.lookfrom) + a * v(cam.defocus_disk_u)) + b * v(cam.defocus_disk_v)
    return origin, sample - origin, rng.f64()


def _near_zero(d):  # vec3.rs:60-65: approx_eq(0.0, F64Margin::zero().epsilon(1e-8)) on every component
    return all(c == 0.0 or abs(c) <= 1e-8 for c in d)


def pixel(oracle, desc, cam, x, y, ao_rays, radius, first_sample=0):
    """-> (open_count, hit_count, rng words consumed) of pixel (x, y)."""
    W, H, S = cam.image_width, cam.image_height, cam.samples_per_pixel
    open_count = hit_count = words = 0
    for s in range(first_sample, first_sample + S):
        rng = Stream(oracle, cam.seed, s * W * H + x * W + y)
        o, d, time = get_ray(cam, rng, x, y)
        hit = oracle.rtiow_hit(desc, o, d, time, 1e-10, INF)
        if hit is not None:
            hit_count += 1
            for _ in range(ao_rays):
                d2 = hit["normal"] + rng.unit_sphere()
                if _near_zero(d2):
                    d2 = hit["normal"]
                dx, dy, dz = float(d2[0]), float(d2[1]), float(d2[2])
                inv = 1.0 / math.sqrt(dx * dx + dy * dy + dz * dz)  # vec3.rs:56 with vec3.rs:36-41, 177-179
                a = np.array([dx * inv, dy * inv, dz * inv])
                open_count += oracle.rtiow_hit(desc, hit["p"], a, time, 1e-10, radius) is None
        words += rng.words()
    return open_count, hit_count, words


def frame(oracle, desc, cam, ao_rays, radius, first_sample=0):
    """-> (open [H, W] uint32, hits [H, W] uint32, words) of the whole frame."""
    W, H = cam.image_width, cam.image_height
    op, hi, words = np.zeros((H, W), dtype=np.uint32), np.zeros((H, W), dtype=np.uint32), 0
    for y in range(H):
        for x in range(W):
            o, h, w = pixel(oracle, desc, cam, x, y, ao_rays, radius, first_sample)
            op[y, x], hi[y, x] = o, h
            words += w
    return op, hi, words


# ---- the two known-answer set-ups shared by tests/test_ao_model.py (on the model) and tests/test_gpu_render_ao.py (on the device)
def known_answer_cases(rl, seed=7):
    """-> {name: (world, camera)}, 12 x 8 frames, S = 2.
    lone_sphere: one unit sphere and no ground; the body is convex, so with R = inf no ambient ray is occluded: open == K * hits.
    inside: the camera at the centre of one sphere of radius 5: every camera ray hits and every ambient ray is occluded."""
    grey = lambda b: b.lambertian(b.solid((0.5, 0.5, 0.5)))
    lone = rl.World.build(lambda b: b.list([b.sphere((0.0, 0.0, -3.0), 1.0, grey(b))]))
    inside = rl.World.build(lambda b: b.list([b.sphere((0.0, 0.0, 0.0), 5.0, grey(b))]))
    params = lambda vfov: rl.CameraParams(aspect_ratio=1.5, image_width=12, samples_per_pixel=2, max_depth=5, vfov=vfov, lookfrom=(0.0, 0.0, 0.0),
                                          lookat=(0.0, 0.0, -1.0), seed=seed)
    return {"lone_sphere": (lone, rl.Camera(params(50.0))), "inside": (inside, rl.Camera(params(90.0)))}
