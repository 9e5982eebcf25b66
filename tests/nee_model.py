"""The definition of the NEE path renders (include/rl_render.h "NEE path renders") in Python, on the CPU oracle alone: draws from
oracle.chacha_script (ao_model.Stream), Camera::get_ray and the Lambertian direction as ao_model restates them, the light points and the
geometry term of direct_model, every hit from oracle.rtiow_hit, every texture value from oracle.texture_value.  Nothing of the library
computes here: `desc`, `materials` and `cam` are the scene description, its material table (api.MATERIAL records) and the derived camera as
data, `lights` is [L][12] (Q, u, v, E).  Python floats are binary64 and every line below is one rounded operation, or a product or sum
written with the parentheses of the definition.  For scenes of Lambertian, DiffuseLight and Flat materials; other kinds are refused.
Not a test module."""
import math

import numpy as np
from ao_model import Stream, _near_zero, get_ray
from direct_model import SEG_TMAX, cross, geometry

INF = float("inf")
MAT_FLAT, MAT_LAMBERTIAN, MAT_DIFFUSE_LIGHT = 0, 1, 4  # RL_MAT_*


def path(oracle, desc, materials, cam, rng, o, d, time, lights, normals, light_samples, seg_tmax):
    """One sample's path from the camera ray (o, d, time), drawing from `rng` -> (c [3], rays traced: path rays + segments)."""
    K = light_samples
    kf = 1.0 / (math.pi * K)
    bg = [float(v) for v in cam.background]
    c, thr = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    count_emission = True
    rays = 0
    for i in range(1, cam.max_depth + 1):
        rays += 1
        hit = oracle.rtiow_hit(desc, o, d, time, 1e-10, INF)
        if hit is None:
            c = [c[ch] + thr[ch] * bg[ch] for ch in range(3)]
            break
        m = materials[hit["mat"]]
        kind = int(m["kind"])
        if kind not in (MAT_FLAT, MAT_LAMBERTIAN, MAT_DIFFUSE_LIGHT):
            raise ValueError(f"material kind {kind}: the model states Lambertian, DiffuseLight and Flat only")
        p, n = [float(v) for v in hit["p"]], [float(v) for v in hit["normal"]]
        tex = [0.0, 0.0, 0.0]
        if kind != MAT_FLAT:
            tex = [float(v) for v in oracle.texture_value(desc, int(m["texture"]), hit["u"], hit["v"], hit["p"])]
        em = tex if kind == MAT_DIFFUSE_LIGHT else [0.0, 0.0, 0.0]
        if count_emission:
            c = [c[ch] + thr[ch] * em[ch] for ch in range(3)]
        sampled = kind == MAT_LAMBERTIAN and i < cam.max_depth
        if sampled:
            dsum = [0.0, 0.0, 0.0]
            for light, nl in zip(lights, normals):
                for _ in range(K):
                    a = rng.f64()
                    b = rng.f64()
                    seg, g = geometry(light, nl, p, n, a, b)
                    if g is None:
                        continue
                    rays += 1
                    if oracle.rtiow_hit(desc, p, seg, time, 1e-10, seg_tmax) is None:
                        dsum = [dsum[ch] + light[9 + ch] * g for ch in range(3)]
            c = [c[ch] + ((thr[ch] * tex[ch]) * dsum[ch]) * kf for ch in range(3)]
        if kind != MAT_LAMBERTIAN:  # DiffuseLight and Flat: scatter returns None
            break
        nd = hit["normal"] + rng.unit_sphere()  # material.rs:76-84
        if _near_zero(nd):
            nd = hit["normal"]
        thr = [thr[ch] * tex[ch] for ch in range(3)]
        o, d = hit["p"], nd
        count_emission = not sampled
    return c, rays


def pixel(oracle, desc, materials, cam, x, y, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0):
    """-> (sums [3], sq [3], rng words consumed, rays traced) of pixel (x, y)."""
    W, H, S = cam.image_width, cam.image_height, cam.samples_per_pixel
    lights = [[float(v) for v in row] for row in np.asarray(lights, dtype=np.float64).reshape(-1, 12)]
    normals = [cross(row[3:6], row[6:9]) for row in lights]
    sums, sq = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    words = rays = 0
    for s in range(first_sample, first_sample + S):
        rng = Stream(oracle, cam.seed, s * W * H + x * W + y)
        o, d, time = get_ray(cam, rng, x, y)
        c, r = path(oracle, desc, materials, cam, rng, o, d, time, lights, normals, light_samples, seg_tmax)
        sums = [sums[ch] + c[ch] for ch in range(3)]
        sq = [sq[ch] + c[ch] * c[ch] for ch in range(3)]
        words += rng.words()
        rays += r
    return sums, sq, words, rays


def frame(oracle, desc, materials, cam, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0):
    """-> (sums [H, W, 3], sq [H, W, 3], words, rays traced) of the whole frame."""
    W, H = cam.image_width, cam.image_height
    su, sq = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    words = rays = 0
    for y in range(H):
        for x in range(W):
            a, b, w, r = pixel(oracle, desc, materials, cam, x, y, lights, light_samples, seg_tmax, first_sample)
            su[y, x], sq[y, x] = a, b
            words += w
            rays += r
    return su, sq, words, rays


# ---- the known-answer set-up of tests/test_nee_model.py
BACKGROUND = (0.125, 0.25, 0.5)
ALBEDO = 0.5
CEILING = ((-1000.0, 4.0, -1000.0), (2000.0, 0.0, 0.0), (0.0, 0.0, 2000.0), (5.0, 4.0, 3.0))  # a DiffuseLight quad over everything
LIGHT_BELOW = [((-1.0, -2.0, -4.0), (2.0, 0.0, 0.0), (0.0, 0.0, 2.0), (5.0, 4.0, 3.0))]         # direct_model's: under the floor, not geometry


def known_answer_cases(rl, max_depth, spp=1, seed=7):
    """-> {name: (world, camera)}, 12 x 8 frames, direct_model's camera at (0, 1, 6) over its floor quad at y = 0 (Lambertian, grey 0.5), a
    background of BACKGROUND; the upper rows look past the floor's far edge.
    open:    the floor alone: what is not floor is background.
    ceiling: the floor under the DiffuseLight quad CEILING: the upper rows see the light itself."""
    grey = lambda b: b.lambertian(b.solid((ALBEDO, ALBEDO, ALBEDO)))
    floor = lambda b: b.quad((-10.0, 0.0, -10.0), (20.0, 0.0, 0.0), (0.0, 0.0, 18.0), grey(b))
    lamp = lambda b: b.quad(*CEILING[:3], b.diffuse_light(b.solid(CEILING[3])))
    open_w = rl.World.build(lambda b: b.list([floor(b)]))
    ceil_w = rl.World.build(lambda b: b.list([floor(b), lamp(b)]))
    cam = lambda: rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=12, samples_per_pixel=spp, max_depth=max_depth, vfov=60.0,
                                            lookfrom=(0.0, 1.0, 6.0), lookat=(0.0, 0.0, 0.0), background=BACKGROUND, seed=seed))
    return {"open": (open_w, cam()), "ceiling": (ceil_w, cam())}
