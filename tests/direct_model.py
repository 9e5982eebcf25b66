"""The definition of the direct-lighting renders (include/rl_render.h "Direct-lighting renders") in Python, on the CPU oracle alone: draws
from oracle.chacha_script (ao_model.Stream), Camera::get_ray as ao_model restates it, both hits from oracle.rtiow_hit.  Nothing of the
library computes here: `desc` and `cam` are the scene description and the derived camera (rl_rtiow_scene_desc, rl_rtiow_camera) as data,
`lights` is [L][12] (Q, u, v, E).  Python floats are binary64 and every line below is one rounded operation, or a sum written with the
parentheses of the definition.  Not a test module."""
import numpy as np
from ao_model import Stream, get_ray

INF = float("inf")
SEG_TMAX = 1.0 - 1e-6


def cross(u, v):  # vec3.rs:48-54, every product rounded
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


def light_point(light, a, b):
    """yl = (Q + u*a) + v*b, component by component."""
    Q, u, v = light[0:3], light[3:6], light[6:9]
    return tuple((float(Q[i]) + float(u[i]) * a) + float(v[i]) * b for i in range(3))


def geometry(light, nl, p, n, a, b):
    """-> (d, g) for the light point (a, b) seen from p with normal n; g is None where the definition skips the sample."""
    yl = light_point(light, a, b)
    d = (yl[0] - p[0], yl[1] - p[1], yl[2] - p[2])
    d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    cs = n[0] * d[0] + n[1] * d[1] + n[2] * d[2]
    cl = abs(nl[0] * d[0] + nl[1] * d[1] + nl[2] * d[2])
    if not (cs > 0.0) or not (cl > 0.0) or not (d2 > 0.0):
        return d, None
    return d, (cs * cl) / (d2 * d2)


def pixel(oracle, desc, cam, x, y, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0):
    """-> (direct [3], unshadowed [3], hit_count, rng words consumed, segments traced) of pixel (x, y)."""
    W, H, S = cam.image_width, cam.image_height, cam.samples_per_pixel
    lights = [[float(c) for c in row] for row in np.asarray(lights, dtype=np.float64).reshape(-1, 12)]
    normals = [cross(row[3:6], row[6:9]) for row in lights]
    direct, unshadowed = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    hit_count = words = traced = 0
    for s in range(first_sample, first_sample + S):
        rng = Stream(oracle, cam.seed, s * W * H + x * W + y)
        o, d, time = get_ray(cam, rng, x, y)
        hit = oracle.rtiow_hit(desc, o, d, time, 1e-10, INF)
        if hit is not None:
            hit_count += 1
            p, n = [float(c) for c in hit["p"]], [float(c) for c in hit["normal"]]
            for light, nl in zip(lights, normals):
                for _ in range(light_samples):
                    a = rng.f64()
                    b = rng.f64()
                    seg, g = geometry(light, nl, p, n, a, b)
                    if g is None:
                        continue
                    traced += 1
                    occluded = oracle.rtiow_hit(desc, p, seg, time, 1e-10, seg_tmax) is not None
                    for c in range(3):
                        e = light[9 + c] * g
                        unshadowed[c] = unshadowed[c] + e
                        if not occluded:
                            direct[c] = direct[c] + e
        words += rng.words()
    return direct, unshadowed, hit_count, words, traced


def frame(oracle, desc, cam, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0):
    """-> (direct [H, W, 3], unshadowed [H, W, 3], hits [H, W] uint32, words, segments traced) of the whole frame."""
    W, H = cam.image_width, cam.image_height
    di, un, hi = np.zeros((H, W, 3)), np.zeros((H, W, 3)), np.zeros((H, W), dtype=np.uint32)
    words = traced = 0
    for y in range(H):
        for x in range(W):
            d, u, h, w, t = pixel(oracle, desc, cam, x, y, lights, light_samples, seg_tmax, first_sample)
            di[y, x], un[y, x], hi[y, x] = d, u, h
            words += w
            traced += t
    return di, un, hi, words, traced


# ---- the known-answer set-ups shared by tests/test_direct_model.py (on the model) and tests/test_gpu_render_direct.py (on the device)
FLOOR_Y = 0.0
LIGHT_ABOVE = [((-1.0, 4.0, -4.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (5.0, 4.0, 3.0))]   # a 2 x 2 light at y = 4, over the floor
LIGHT_BELOW = [((-1.0, -2.0, -4.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (5.0, 4.0, 3.0))]  # the same light at y = -2, under it


def known_answer_cases(rl, seed=7):
    """-> {name: (world, camera)}, 12 x 8 frames, S = 2, a camera at (0, 1, 6) looking at the origin over a floor quad at y = 0,
    x in [-10, 10], z in [-10, 8]; the upper rows look past the floor's far edge: pixels without a hit.
    open:    the floor alone.  With LIGHT_ABOVE nothing shadows: direct == unshadowed in bytes, > 0 wherever hits > 0.
    blocked: the floor and a blocker quad at y = 2, x in [-8, 8], z in [-12, 6].  A segment from a floor point (px, 0, pz) to a light point
             (lx, 4, lz) crosses y = 2 at its midpoint ((px + lx) / 2, 2, (pz + lz) / 2): |px + lx| <= 11 < 16 and -14 <= pz + lz <= 6,
             inside [-24, 12], so the blocker is between EVERY floor point and EVERY light point, at t = 0.5.  The camera is below the
             blocker, so it sees the same floor points as in `open`; camera rays that climb meet the blocker's underside, whose record
             normal points down (cs < 0: nothing added).  On the floor pixels of `open`: direct == 0 and unshadowed has `open`'s bytes.
    With LIGHT_BELOW on `open`: cs < 0 everywhere, both sums 0, hits unchanged, 4 L K words per hit still drawn."""
    grey = lambda b: b.lambertian(b.solid((0.5, 0.5, 0.5)))
    floor = lambda b: b.quad((-10.0, FLOOR_Y, -10.0), (20.0, 0.0, 0.0), (0.0, 0.0, 18.0), grey(b))
    blocker = lambda b: b.quad((-8.0, 2.0, -12.0), (16.0, 0.0, 0.0), (0.0, 0.0, 18.0), grey(b))
    open_w = rl.World.build(lambda b: b.list([floor(b)]))
    blocked_w = rl.World.build(lambda b: b.list([floor(b), blocker(b)]))
    cam = lambda: rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=12, samples_per_pixel=2, max_depth=5, vfov=60.0, lookfrom=(0.0, 1.0, 6.0),
                                            lookat=(0.0, 0.0, 0.0), seed=seed))
    return {"open": (open_w, cam()), "blocked": (blocked_w, cam())}
