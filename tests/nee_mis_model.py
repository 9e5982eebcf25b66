"""The definition of the NEE path renders with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance
sampling") in Python, on the CPU oracle alone.  It is nee_model.path with two additions: every light point that counts is weighted against
the scattered ray's density, and the scattered ray of a vertex that sampled the lights is intersected with every light's parallelogram
and, where it crosses one, connected with the light points' own segment test and the complementary weight.  Draws, hits and texture values
come from where nee_model takes them; the light points and their geometry term are direct_model's.  Python floats are binary64 and every
line below is one rounded operation, or a product or sum written with the parentheses of the definition.  For scenes of Lambertian,
DiffuseLight and Flat materials; other kinds are refused.  Not a test module."""
import math

import numpy as np
from ao_model import Stream, _near_zero, get_ray
from direct_model import SEG_TMAX, cross, geometry
from nee_model import INF, MAT_DIFFUSE_LIGHT, MAT_FLAT, MAT_LAMBERTIAN

BALANCE, POWER = 0, 1  # RL_MIS_BALANCE, RL_MIS_POWER
HEURISTICS = {"balance": BALANCE, "power": POWER}


def dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def light_weight(g, kf, heuristic):
    """wl: what a light point's g becomes (wl * kf is the light strategy's share of the pair)."""
    q = g * kf
    return g / (1.0 + q) if heuristic == BALANCE else g / (1.0 + q * q)


def scatter_weight(g, kf, heuristic):
    """wb: the scattered ray's share of the pair at the point where it crosses the light."""
    q = g * kf
    return q / (1.0 + q) if heuristic == BALANCE else (q * q) / (1.0 + q * q)


def crossing(light, nl, x, n, w):
    """The scattered ray x + t w against the light's parallelogram -> (d, g): the segment to the crossing point and its geometry term;
    (None, None) where the definition skips the light."""
    Q, u, v = light[0:3], light[3:6], light[6:9]
    den = dot(nl, w)
    if not (abs(den) > 0.0):
        return None, None
    r = (Q[0] - x[0], Q[1] - x[1], Q[2] - x[2])
    t = dot(nl, r) / den
    if not (t > 0.0) or not (t < INF):
        return None, None
    d = (w[0] * t, w[1] * t, w[2] * t)
    y = (x[0] + d[0], x[1] + d[1], x[2] + d[2])
    h = (y[0] - Q[0], y[1] - Q[1], y[2] - Q[2])
    nn = dot(nl, nl)
    al = dot(nl, cross(h, v)) / nn
    be = dot(nl, cross(u, h)) / nn
    if not (0.0 <= al <= 1.0) or not (0.0 <= be <= 1.0):
        return None, None
    d2 = dot(d, d)
    cs = dot(n, d)
    cl = abs(dot(nl, d))
    if not (cs > 0.0) or not (cl > 0.0) or not (d2 > 0.0):
        return None, None
    g = (cs * cl) / (d2 * d2)
    if not (g < INF):
        return None, None
    return d, g


def path(oracle, desc, materials, cam, rng, o, d, time, lights, normals, light_samples, seg_tmax, heuristic):
    """One sample's path from the camera ray (o, d, time), drawing from `rng`
    -> (c [3], rays traced: path rays + segments, light points that counted, scattered-ray connections made, of them free)."""
    if heuristic not in (BALANCE, POWER):
        raise ValueError("heuristic is BALANCE or POWER")
    K = light_samples
    kf = 1.0 / (math.pi * K)
    bg = [float(v) for v in cam.background]
    c, thr = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    count_emission = True
    rays = counted = made = free = 0
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
        if sampled:  # the light strategy
            dsum = [0.0, 0.0, 0.0]
            for light, nl in zip(lights, normals):
                for _ in range(K):
                    a = rng.f64()
                    b = rng.f64()
                    seg, g = geometry(light, nl, p, n, a, b)
                    if g is None or not (g < INF):
                        continue
                    wl = light_weight(g, kf, heuristic)
                    rays += 1
                    if oracle.rtiow_hit(desc, p, seg, time, 1e-10, seg_tmax) is None:
                        counted += 1
                        dsum = [dsum[ch] + light[9 + ch] * wl for ch in range(3)]
            c = [c[ch] + ((thr[ch] * tex[ch]) * dsum[ch]) * kf for ch in range(3)]
        if kind != MAT_LAMBERTIAN:  # DiffuseLight and Flat: scatter returns None
            break
        nd = hit["normal"] + rng.unit_sphere()  # material.rs:76-84
        if _near_zero(nd):
            nd = hit["normal"]
        thr = [thr[ch] * tex[ch] for ch in range(3)]
        if sampled:  # the scattered-ray strategy: no draw
            w = [float(v) for v in nd]
            bsum = [0.0, 0.0, 0.0]
            for light, nl in zip(lights, normals):
                seg, g = crossing(light, nl, p, n, w)
                if g is None:
                    continue
                wb = scatter_weight(g, kf, heuristic)
                rays += 1
                made += 1
                if oracle.rtiow_hit(desc, p, seg, time, 1e-10, seg_tmax) is None:
                    free += 1
                    bsum = [bsum[ch] + light[9 + ch] * wb for ch in range(3)]
            c = [c[ch] + thr[ch] * bsum[ch] for ch in range(3)]
        o, d = hit["p"], nd
        count_emission = not sampled
    return c, rays, counted, made, free


def first_hit_kinds(oracle, world, cam, first_sample=0):
    """-> [S, H, W]: the material kind the camera ray of every sample of every pixel meets (-1: none), from the oracle alone."""
    W, H, S = cam.image_width, cam.image_height, cam.samples_per_pixel
    mats = world.materials()
    kinds = np.full((S, H, W), -1)
    for s in range(S):
        for y in range(H):
            for x in range(W):
                rng = Stream(oracle, cam.seed, (first_sample + s) * W * H + x * W + y)
                o, d, time = get_ray(cam, rng, x, y)
                hit = oracle.rtiow_hit(world.desc, o, d, time, 1e-10, INF)
                if hit is not None:
                    kinds[s, y, x] = int(mats[hit["mat"]]["kind"])
    return kinds


def pixel(oracle, desc, materials, cam, x, y, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0, heuristic=BALANCE):
    """-> (sums [3], sq [3], rng words consumed, rays traced, light points that counted, scattered-ray connections made, of them free,
    the largest channel of a sample) of pixel (x, y)."""
    W, H, S = cam.image_width, cam.image_height, cam.samples_per_pixel
    lights = [[float(v) for v in row] for row in np.asarray(lights, dtype=np.float64).reshape(-1, 12)]
    normals = [cross(row[3:6], row[6:9]) for row in lights]
    sums, sq = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    words = rays = counted = made = free = 0
    largest = 0.0
    for s in range(first_sample, first_sample + S):
        rng = Stream(oracle, cam.seed, s * W * H + x * W + y)
        o, d, time = get_ray(cam, rng, x, y)
        c, r, k, m, f = path(oracle, desc, materials, cam, rng, o, d, time, lights, normals, light_samples, seg_tmax, heuristic)
        sums = [sums[ch] + c[ch] for ch in range(3)]
        sq = [sq[ch] + c[ch] * c[ch] for ch in range(3)]
        words += rng.words()
        rays, counted, made, free = rays + r, counted + k, made + m, free + f
        largest = max(largest, max(c))
    return sums, sq, words, rays, counted, made, free, largest


def frame(oracle, desc, materials, cam, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0, heuristic=BALANCE):
    """-> (sums [H, W, 3], sq [H, W, 3], words, rays traced, info) of the whole frame; info = {"counted": light points that counted,
    "made": scattered-ray connections made, "free": of them free, "largest": the largest channel of a sample}."""
    W, H = cam.image_width, cam.image_height
    su, sq = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    words = rays = 0
    info = {"counted": 0, "made": 0, "free": 0, "largest": 0.0}
    for y in range(H):
        for x in range(W):
            a, b, w, r, k, m, f, big = pixel(oracle, desc, materials, cam, x, y, lights, light_samples, seg_tmax, first_sample, heuristic)
            su[y, x], sq[y, x] = a, b
            words += w
            rays += r
            info["counted"] += k
            info["made"] += m
            info["free"] += f
            info["largest"] = max(info["largest"], big)
    return su, sq, words, rays, info
