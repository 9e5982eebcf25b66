"""The definition of the NEE path renders with sphere lights (include/rl_render.h "NEE path renders with sphere lights") in Python, on the
CPU oracle alone.  It is nee_mis_model.path with the two sphere statements: behind the quads' light points, K points per sphere light
drawn with UnitSphere from the sample's stream, and behind the quads' candidates of the scattered ray, its near root on every sphere
light.  What it shares with nee_mis_model (the weights, the quads' crossing, the stream, the camera) is imported.  Python floats are
binary64 and every line below is one rounded operation, or a product or sum written with the parentheses of the definition.  For scenes
of Lambertian, DiffuseLight and Flat materials; other kinds are refused.  Not a test module."""
import math

import numpy as np
from ao_model import Stream, _near_zero, get_ray
from direct_model import SEG_TMAX, cross, geometry
from nee_mis_model import BALANCE, POWER, crossing, dot, light_weight, scatter_weight
from nee_model import INF, MAT_DIFFUSE_LIGHT, MAT_FLAT, MAT_LAMBERTIAN


class StreamAt(Stream):
    """ao_model.Stream continued at an even word position of the stream: what a host composition draws a vertex's light points from."""

    def __init__(self, oracle, seed, stream, word_pos):
        super().__init__(oracle, seed, stream)
        assert word_pos % 2 == 0
        self.i = word_pos // 2

    def _at(self, kind):
        if self.i >= self.f.size:
            n = max(32, 2 * self.f.size, 2 * (self.i + 1))
            self.f = self.oracle.chacha_script(self.seed, [("set_stream", self.stream)] + [("f64",)] * n)[0][1:]
            self.u = self.oracle.chacha_script(self.seed, [("set_stream", self.stream)] + [("uniform",)] * n)[0][1:]
        return super()._at(kind)


def area(r):
    """A of a sphere light, the host's double."""
    return (4.0 * math.pi) * (r * r)


def _term(n, d, co, A):
    """d2, cs, cl, the skips and g of a candidate (d, co) -> g, or None where the definition skips it."""
    d2 = dot(d, d)
    cs = dot(n, d)
    cl = co * A
    if not (cs > 0.0) or not (co > 0.0) or not (d2 > 0.0):
        return None
    g = (cs * cl) / (d2 * d2)
    if not (g < INF):
        return None
    return g


def sphere_point(sphere, A, x, n, wu):
    """The light strategy's candidate for the unit vector wu = UnitSphere.sample(rng) -> (d, g), or (None, None) where it is skipped."""
    C, r = sphere[0:3], sphere[3]
    yl = (C[0] + wu[0] * r, C[1] + wu[1] * r, C[2] + wu[2] * r)
    d = (yl[0] - x[0], yl[1] - x[1], yl[2] - x[2])
    co = -dot(wu, d)
    g = _term(n, d, co, A)
    return (None, None) if g is None else (d, g)


def sphere_crossing(sphere, A, x, n, w):
    """The scattered ray x + t w against the sphere, Sphere::hit's order, the near root only -> (d, g), or (None, None)."""
    C, r = sphere[0:3], sphere[3]
    oc = (x[0] - C[0], x[1] - C[1], x[2] - C[2])
    a = dot(w, w)
    hb = dot(oc, w)
    cc = dot(oc, oc) - r * r
    disc = hb * hb - a * cc
    if not (disc > 0.0):
        return None, None
    sd = math.sqrt(disc)
    t = (-hb - sd) / a
    if not (t > 0.0) or not (t < INF):
        return None, None
    d = (w[0] * t, w[1] * t, w[2] * t)
    y = (x[0] + d[0], x[1] + d[1], x[2] + d[2])
    wn = ((y[0] - C[0]) / r, (y[1] - C[1]) / r, (y[2] - C[2]) / r)
    co = -dot(wn, d)
    g = _term(n, d, co, A)
    return (None, None) if g is None else (d, g)


def new_info():
    """The eight kinds of term a path can meet, counted: (quad | sphere) x (light point | scattered ray) x (free | occluded), and the sphere
    points drawn and skipped."""
    info = {f"{k}_{s}_{o}": 0 for k in ("quad", "sphere") for s in ("light", "scatter") for o in ("free", "occluded")}
    info.update(sphere_drawn=0, sphere_skipped=0, largest=0.0)
    return info


def path(oracle, desc, materials, cam, rng, o, d, time, lights, normals, spheres, areas, light_samples, seg_tmax, heuristic, info):
    """One sample's path from the camera ray (o, d, time), drawing from `rng` -> (c [3], rays traced: path rays + segments); the kinds of
    term are counted into `info`."""
    if heuristic not in (BALANCE, POWER):
        raise ValueError("heuristic is BALANCE or POWER")
    K = light_samples
    kf = 1.0 / (math.pi * K)
    bg = [float(v) for v in cam.background]
    c, thr = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    count_emission = True
    rays = 0

    def segment(p, seg, kind, strategy):
        free = oracle.rtiow_hit(desc, p, seg, time, 1e-10, seg_tmax) is None
        info[f"{kind}_{strategy}_{'free' if free else 'occluded'}"] += 1
        return free
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
        if sampled:  # the light strategy: the quads, then the spheres
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
                    if segment(p, seg, "quad", "light"):
                        dsum = [dsum[ch] + light[9 + ch] * wl for ch in range(3)]
            for sph, A in zip(spheres, areas):
                for _ in range(K):
                    wu = [float(v) for v in rng.unit_sphere()]
                    info["sphere_drawn"] += 1
                    seg, g = sphere_point(sph, A, p, n, wu)
                    if g is None:
                        info["sphere_skipped"] += 1
                        continue
                    wl = light_weight(g, kf, heuristic)
                    rays += 1
                    if segment(p, seg, "sphere", "light"):
                        dsum = [dsum[ch] + sph[4 + ch] * wl for ch in range(3)]
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
                if segment(p, seg, "quad", "scatter"):
                    bsum = [bsum[ch] + light[9 + ch] * wb for ch in range(3)]
            for sph, A in zip(spheres, areas):
                seg, g = sphere_crossing(sph, A, p, n, w)
                if g is None:
                    continue
                wb = scatter_weight(g, kf, heuristic)
                rays += 1
                if segment(p, seg, "sphere", "scatter"):
                    bsum = [bsum[ch] + sph[4 + ch] * wb for ch in range(3)]
            c = [c[ch] + thr[ch] * bsum[ch] for ch in range(3)]
        o, d = hit["p"], nd
        count_emission = not sampled
    return c, rays


def _rows(a, width):
    return [[float(v) for v in row] for row in np.asarray(a, dtype=np.float64).reshape(-1, width)]


def pixel(oracle, desc, materials, cam, x, y, lights, spheres, light_samples, seg_tmax=SEG_TMAX, first_sample=0, heuristic=BALANCE, info=None):
    """-> (sums [3], sq [3], rng words consumed, rays traced) of pixel (x, y); lights [L, 12] (may be empty), spheres [Ls, 7]."""
    W, H, S = cam.image_width, cam.image_height, cam.samples_per_pixel
    lights, spheres = _rows(lights, 12), _rows(spheres, 7)
    normals = [cross(row[3:6], row[6:9]) for row in lights]
    areas = [area(row[3]) for row in spheres]
    info = new_info() if info is None else info
    sums, sq = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    words = rays = 0
    for s in range(first_sample, first_sample + S):
        rng = Stream(oracle, cam.seed, s * W * H + x * W + y)
        o, d, time = get_ray(cam, rng, x, y)
        c, r = path(oracle, desc, materials, cam, rng, o, d, time, lights, normals, spheres, areas, light_samples, seg_tmax, heuristic, info)
        sums = [sums[ch] + c[ch] for ch in range(3)]
        sq = [sq[ch] + c[ch] * c[ch] for ch in range(3)]
        words += rng.words()
        rays += r
        info["largest"] = max(info["largest"], max(c))
    return sums, sq, words, rays


def frame(oracle, desc, materials, cam, lights, spheres, light_samples, seg_tmax=SEG_TMAX, first_sample=0, heuristic=BALANCE):
    """-> (sums [H, W, 3], sq [H, W, 3], words, rays traced, info) of the whole frame; info is new_info()'s counts."""
    W, H = cam.image_width, cam.image_height
    su, sq = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    words = rays = 0
    info = new_info()
    for y in range(H):
        for x in range(W):
            a, b, w, r = pixel(oracle, desc, materials, cam, x, y, lights, spheres, light_samples, seg_tmax, first_sample, heuristic, info)
            su[y, x], sq[y, x] = a, b
            words += w
            rays += r
    return su, sq, words, rays, info


# ---- the known-answer set-up of tests/test_nee_spheres_model.py and of the GPU suite
ALBEDO = 0.5
UNDER = ((0.0, 4.0, 0.0), 2.0, 4.0)  # the sphere light over the floor point (0, 0, 0): rho E (r / h)^2 = 0.5 * 4 * (2 / 4)^2 = 0.5 there
UNDER_ANSWER = ALBEDO * UNDER[2] * (UNDER[1] / UNDER[0][1]) ** 2


def under_a_sphere(rl, spp, width=12, seed=11):
    """-> (world, camera): a grey Lambertian floor quad at y = 0 alone (the sphere light UNDER is NOT geometry), black background,
    max_depth 2, looked at straight down from (0, 3, 0) through a 0.2 degree lens: every pixel sees a floor point within 0.006 of the
    point under the centre, where the irradiance of the sphere is pi E (r / h)^2 (it changes with the square of the offset over h: below
    1e-5 relative here)."""
    world = rl.World.build(lambda b: b.list([b.quad((-10.0, 0.0, -10.0), (20.0, 0.0, 0.0), (0.0, 0.0, 20.0), b.lambertian(b.solid((ALBEDO,) * 3)))]))
    cam = rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=width, samples_per_pixel=spp, max_depth=2, vfov=0.2, lookfrom=(0.0, 3.0, 0.0),
                                    lookat=(0.0, 0.0, 0.0), vup=(0.0, 0.0, -1.0), background=(0.0, 0.0, 0.0), seed=seed))
    return world, cam
