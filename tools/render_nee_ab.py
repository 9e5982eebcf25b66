#!/usr/bin/env python3
"""The NEE path render next to the plain path tracer on the same 1920x1080 frame, S = 4, max_depth 50: ms of render_nee_device and of
render_independent_device, the frame-summed variance of the pixel means of each (from sums and sq: render_nee_device's own, and
render_moments_device's for the plain path), and the efficiency ratio (variance x time of the plain render) / (variance x time of the
NEE render).  Reported, not a gate.  HIP events on the launch stream, 3 warm-up + --reps timed repetitions, median [min, max].
The parent process never opens the GPU: every step runs in a child of its own under a time limit, and the first failing step ends the
run.  Results: profiles/render_nee.json (merged per step) and one JSON line per step on stdout.

usage: tools/render_nee_ab.py [--reps 20] [--steps cornell_k1,cornell_k4,built] [--width 1920] [--out profiles/render_nee.json]        (GPU)
steps: cornell_k1 / cornell_k4 = cornell_box with its own light, K = 1 / 4; built = the test suite's built world (a Lambertian ground, 30
spheres of four materials, every third one moving, under two DiffuseLight quads), K = 1."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"cornell_k1": 400, "cornell_k4": 400, "built": 400}
S, MAX_DEPTH = 4, 50
CORNELL_LIGHT = [((343.0, 554.0, 332.0), (-130.0, 0.0, 0.0), (0.0, 0.0, -105.0), 15.0)]
BUILT_LIGHTS = [((-1.5, 4.0, -1.5), (3.0, 0.0, 0.0), (0.0, 0.0, 3.0), (6.0, 6.0, 6.0)), ((4.0, 2.0, -1.0), (0.0, 0.0, 2.0), (1.0, 1.5, 0.0), (5.0, 3.5, 2.0))]


def built_world(rl):
    """tests/test_gpu_render_nee.py's _built_world."""
    import numpy as np
    rng = np.random.default_rng(2027)

    def build(b):
        mats = [b.lambertian(b.solid((0.6, 0.5, 0.4))), b.metal((0.8, 0.8, 0.7), 0.3), b.dielectric(1.5), b.flat()]
        objs = [b.sphere((0.0, -100.0, 0.0), 100.0, b.lambertian(b.solid((0.5, 0.6, 0.5))))]
        for i in range(30):
            c = np.array([rng.uniform(-3.0, 3.0), rng.uniform(0.2, 1.4), rng.uniform(-3.0, 3.0)])
            c2 = c + (0.0, rng.uniform(0.1, 0.4), 0.0) if i % 3 == 0 else None
            objs.append(b.sphere(c, rng.uniform(0.15, 0.5), mats[i % len(mats)], center2=c2))
        for q, u, v, e in BUILT_LIGHTS:
            objs.append(b.quad(q, u, v, b.diffuse_light(b.solid(e))))
        return b.bvh(objs)
    w = rl.World.build(build)
    w.params = rl.CameraParams(vfov=40.0, lookfrom=(6.0, 2.5, 5.0), lookat=(0.0, 0.5, 0.0), defocus_angle=0.6, focus_dist=8.0, background=(0.05, 0.06, 0.08),
                               seed=11)
    return w


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "reps": int(a.size)}


def _time(fn, reps, torch):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return _stats(ms)


def _variance(torch, sums, sq, n):
    """The frame sum of Moments.variance_of_mean: (sq - sums^2 / n) / (n - 1) / n, clipped at 0."""
    return float(torch.clamp((sq - sums * sums / n) / (n - 1) / n, min=0.0).sum().item())


def step(name, reps, width):
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    api = rl.api
    if name == "built":
        world, lights, K = built_world(rl), BUILT_LIGHTS, 1
    else:
        world, lights, K = rl.World.example_scene("cornell_box"), CORNELL_LIGHT, (1 if name == "cornell_k1" else 4)
    p = world.params
    p.aspect_ratio, p.image_width, p.samples_per_pixel, p.max_depth = 16.0 / 9.0, width, S, MAX_DEPTH
    cam = rl.Camera(p)
    n = cam.c.image_width * cam.c.image_height
    s0 = torch.cuda.current_stream().cuda_stream
    dev = "cuda:0"
    d_su, d_sq, p_su, p_sq, d_ind = (torch.zeros(n * 3, dtype=torch.float64, device=dev) for _ in range(5))
    nee = lambda: rl.render_nee_device(cam, world, lights, K, stream=s0, d_sums=d_su.data_ptr(), d_sq=d_sq.data_ptr())
    plain = lambda: cam.render_independent_device(world, d_ind.data_ptr(), stream=s0)
    out = {"step": name, "width": cam.c.image_width, "height": cam.c.image_height, "pixels": n, "samples": S, "max_depth": MAX_DEPTH, "lights": len(lights),
           "light_samples": K, "seg_tmax": rl.direct.SEG_TMAX, "render_lib": os.path.basename(api.RENDER_LIB)}
    for label, fn in (("render_nee_device", nee), ("render_independent_device", plain)):
        row = _time(fn, reps, torch)
        api.render_status(world, allow_degenerate=True)
        fn()
        torch.cuda.synchronize()
        st = api.render_status(world, allow_degenerate=True)
        row["rays"] = int(st["rays"])
        if label == "render_nee_device":
            row["served_by"], row["retraced"] = api.last_query()["kernel"], int(st["slow_traces"])
        out[label] = row
    cam.render_moments_device(world, p_su.data_ptr(), p_sq.data_ptr(), stream=s0)
    torch.cuda.synchronize()
    api.render_status(world, allow_degenerate=True)
    # (render_moments is the CHAINED render: a pixel's samples continue one stream; render_independent restarts the stream per sample.  Two
    # estimates of the same image, not the same bytes; recorded so that nobody reads the variance as that of the timed call's own samples.)
    out["plain_sums_are_render_independents"] = bool(torch.equal(p_su.view(torch.int64), d_ind.view(torch.int64)))
    out["variance_nee"], out["variance_plain"] = _variance(torch, d_su, d_sq, S), _variance(torch, p_su, p_sq, S)
    out["mean_nee"], out["mean_plain"] = float(d_su.sum().item()) / (S * n * 3), float(p_su.sum().item()) / (S * n * 3)
    # the counter-free render against the counting one (the reference-order fold for every ray), byte for byte
    fast_su, fast_sq = d_su.clone(), d_sq.clone()
    rl.render_nee_device(cam, world, lights, K, stream=s0, d_sums=d_su.data_ptr(), d_sq=d_sq.data_ptr(), stats={}, allow_degenerate=True)
    out["same_bytes_as_counting"] = bool(torch.equal(fast_su.view(torch.int64), d_su.view(torch.int64)) and torch.equal(fast_sq.view(torch.int64), d_sq.view(torch.int64)))
    tn, tp = out["render_nee_device"]["median_ms"], out["render_independent_device"]["median_ms"]
    out["ratio_nee_over_plain_ms"] = tn / tp
    out["efficiency_ratio"] = (out["variance_plain"] * tp) / (out["variance_nee"] * tn) if out["variance_nee"] > 0.0 else None
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="cornell_k1,cornell_k4,built")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_nee.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.width)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for name in a.steps.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--width", str(a.width)], stdout=subprocess.PIPE,
                               text=True, timeout=LIMITS[name])
        except subprocess.TimeoutExpired:
            print(f"step {name}: time limit of {LIMITS[name]} s reached; stopping", file=sys.stderr)
            return 1
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
            return 1
        results[name] = json.loads(line[-1][7:])
        print(line[-1][7:], flush=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
