#!/usr/bin/env python3
"""Where do the largest NEE samples of cornell_box come from?  Renders the 1920x1080 frame at S = 1, K = 1, max_depth 50
with render_pixels_nee, lists the largest sample values and their share of the sum of squares, and replays the paths of the three
largest with the host composition (get_rays, hit_rays, the light point's draws from the oracle's ChaCha script, occluded_rays,
scatter_rays), printing every vertex: position, normal, throughput, geometry term, distance to the light point and what it adds.
usage: tools/render_nee_fireflies.py > profiles/render_nee_fireflies.txt        (GPU, one process, a few seconds)"""
import importlib
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
rl = importlib.import_module("rendering-learning_amd")
oracle = importlib.import_module("rl_oracle")
api = rl.api
rl.init(0)
LIGHT = [((343.0, 554.0, 332.0), (-130.0, 0.0, 0.0), (0.0, 0.0, -105.0), 15.0)]
T = 1.0 - 1e-6
world = rl.World.example_scene("cornell_box")
p = world.params
p.aspect_ratio, p.image_width, p.samples_per_pixel, p.max_depth = 16.0 / 9.0, 1920, 1, 50
cam = rl.Camera(p)
W, H = cam.c.image_width, cam.c.image_height
y, x = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
r = rl.render_pixels_nee(cam, world, x, y, LIGHT, 1, T)
c = r.sums
order = np.argsort(c.max(axis=1))[::-1]
print("samples", W * H, "mean", c.mean(), "sum of squares", float((c * c).sum()))
top = c.max(axis=1)[order]
print("largest 10 sample values", top[:10])
print("share of the sum of squares held by the largest 10 / 100 / 1000 samples", [float((c[order[:k]] ** 2).sum() / (c * c).sum()) for k in (10, 100, 1000)])
L = rl.pack_lights(LIGHT)[0]
Q, u, v, E = L[0:3], L[3:6], L[6:9], L[9:12]
nl = np.cross(u, v)
kinds = world.materials()["kind"]
for idx in order[:3]:
    px, py = np.array([x[idx]], dtype=np.uint64), np.array([y[idx]], dtype=np.uint64)
    stream = px * np.uint64(W) + py
    rays, cur = cam.get_rays(px, py, api.pack_cursors(stream, 0))
    wp = int(cur["word_pos"][0])
    thr = np.ones(3)
    print("pixel", int(px[0]), int(py[0]), "sample value", c[idx])
    for i in range(1, 51):
        hit = world.hit_rays(rays["origin"], rays["dir"], times=rays["time"], tmin=1e-10)
        if not hit["hit"][0]:
            print("  vertex", i, "miss")
            break
        kind = int(kinds[hit["material"][0]])
        lam = kind == api.MAT_LAMBERTIAN and i < 50
        term = None
        if lam:
            ab = oracle.chacha_script(cam.params.seed, [("set_stream", int(stream[0]))] + [("f64",)] * (wp // 2 + 2))[0][1:][wp // 2:]
            yl = (Q + u * ab[0]) + v * ab[1]
            d = yl - hit["p"][0]
            d2 = float(d @ d)
            cs, cl = float(hit["normal"][0] @ d), abs(float(nl @ d))
            if cs > 0 and cl > 0 and d2 > 0:
                g = cs * cl / (d2 * d2)
                occ = rl.occluded_rays(world, hit["p"], d[None, :], times=rays["time"], tmin=1e-10, tmax=T)[0]
                term = (g, bool(occ), math.sqrt(d2))
            wp += 4
        sc, cur2 = world.scatter_rays(rays, hit, api.pack_cursors(stream, wp), cam.params.seed)
        contrib = None if term is None or term[1] else (thr * sc["attenuation"][0]) * E * term[0] / math.pi
        print("  vertex", i, "kind", kind, "p", hit["p"][0], "normal", hit["normal"][0], "thr", thr, "g, occluded, |d|", term, "adds", contrib)
        wp = int(cur2["word_pos"][0])
        if not sc["scatter"][0]:
            break
        thr = thr * sc["attenuation"][0]
        rays = sc["scattered"].copy()
