#!/usr/bin/env python3
"""The NEE-MIS render with sphere lights on the reference scene that needs them: simple_light at 1920x1080, S = 4,
max_depth 50, K = 1.  Time, rays, frame mean and frame-summed variance of the pixel means of
  - render_independent_device / render_moments_device: the plain path tracer (the expectation every other row should have),
  - render_nee_mis_device with the quad alone: what the library offered before (the sphere's light on the ground is missing),
  - render_nee_mis_device with the quad and sphere_lights = the sphere: this change;
the share of sphere points skipped as back-facing (at the first vertices of a 240x135 grid of camera rays, numpy draws: a geometric
statistic, not the render's stream) and the re-traced count.  Reported, not a gate.  HIP events on the launch stream, device-resident
buffers, 3 warm-up + --reps timed repetitions, median [min, max] (tools/render_nee_ab.py's clock).

--parent-lib PATH: a build of the parent commit's library.  The first two rows are then measured in a child that loads that library
(RL_RENDER_LIB): the reference of a measurement is never the code under test alone.  This build's quad-alone render is measured too and
its bytes are compared with the parent's through a digest.

The parent process never opens the GPU: every step runs in a child of its own under a time limit, and the first failing step ends the
run.  Results: profiles/render_nee_spheres.json and one JSON line on stdout.

usage: tools/render_nee_spheres_ab.py [--reps 20] [--width 1920] [--parent-lib PATH] [--out profiles/render_nee_spheres.json]   (GPU)"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import render_nee_ab as nab  # noqa: E402  (the clock and the variance of the NEE measurement)

LIMIT = 500
S, MAX_DEPTH, K = nab.S, nab.MAX_DEPTH, 1
QUAD = [((3.0, 1.0, -2.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), 4.0)]  # examples/simple_light.rs
BALL = [((0.0, 7.0, 0.0), 2.0, 4.0)]
HEURISTICS = ("balance", "power")


def _digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.cpu().numpy().tobytes())
    return h.hexdigest()[:16]


def _back_facing_share(rl, world, p):
    """Of sphere points drawn uniformly on BALL from the first vertices of a 240 x 135 grid of camera rays: the share the definition skips
    (cs <= 0 or co <= 0), and the share with co <= 0 alone."""
    import dataclasses

    import numpy as np
    cam = rl.Camera(dataclasses.replace(p, image_width=240, samples_per_pixel=1))
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
    rays, _ = cam.get_rays(x, y, rl.api.pack_cursors(x * np.uint64(W) + y, 0))
    hits = world.hit_rays(rays["origin"], rays["dir"], times=rays["time"], tmin=1e-10, allow_degenerate=True)
    lam = (hits["hit"] != 0) & (world.materials()["kind"][hits["material"]] == rl.api.MAT_LAMBERTIAN)
    pts, nrm = hits["p"][lam], hits["normal"][lam]
    w = np.random.default_rng(1).normal(size=pts.shape)
    w /= np.linalg.norm(w, axis=1, keepdims=True)
    C, r = np.array(BALL[0][0]), BALL[0][1]
    d = (C + w * r) - pts
    co, cs = -(w * d).sum(1), (nrm * d).sum(1)
    return {"first_vertices": int(lam.sum()), "skipped": float(((co <= 0) | (cs <= 0)).mean()), "back_facing": float((co <= 0).mean())}


def step(reps, width, parent_only):
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    api = rl.api
    world = rl.World.simple_light()
    p = world.params
    p.aspect_ratio, p.image_width, p.samples_per_pixel, p.max_depth = 16.0 / 9.0, width, S, MAX_DEPTH
    cam = rl.Camera(p)
    n = cam.c.image_width * cam.c.image_height
    s0 = torch.cuda.current_stream().cuda_stream
    d_su, d_sq, d_ind = (torch.zeros(n * 3, dtype=torch.float64, device="cuda:0") for _ in range(3))
    out = {"scene": "simple_light", "width": cam.c.image_width, "height": cam.c.image_height, "pixels": n, "samples": S, "max_depth": MAX_DEPTH, "light_samples": K,
           "seg_tmax": rl.direct.SEG_TMAX, "render_lib": os.path.basename(os.path.dirname(api.RENDER_LIB)) + "/" + os.path.basename(api.RENDER_LIB)}
    calls = {"render_independent_device": lambda: cam.render_independent_device(world, d_ind.data_ptr(), stream=s0),
             "render_moments_device": lambda: cam.render_moments_device(world, d_su.data_ptr(), d_sq.data_ptr(), stream=s0)}
    for h in HEURISTICS:
        calls["render_nee_mis_device:quad alone:" + h] = lambda h=h: rl.render_nee_mis_device(cam, world, QUAD, K, heuristic=h, stream=s0, d_sums=d_su.data_ptr(),
                                                                                             d_sq=d_sq.data_ptr())
        if not parent_only:
            calls["render_nee_mis_device:quad and sphere:" + h] = lambda h=h: rl.render_nee_mis_device(cam, world, QUAD, K, heuristic=h, stream=s0, d_sums=d_su.data_ptr(),
                                                                                                      d_sq=d_sq.data_ptr(), sphere_lights=BALL)
    for label, fn in calls.items():
        row = nab._time(fn, reps, torch)
        api.render_status(world, allow_degenerate=True)
        fn()
        torch.cuda.synchronize()
        st = api.render_status(world, allow_degenerate=True)
        row["rays"] = int(st["rays"])
        if label != "render_independent_device":
            row["variance"] = nab._variance(torch, d_su, d_sq, S)
            row["mean"] = float(d_su.sum().item()) / (S * n * 3)
            row["digest"] = _digest(d_su, d_sq)
        if label.startswith("render_nee_mis"):
            row["served_by"], row["retraced"] = api.last_query()["kernel"], int(st["slow_traces"])
        out[label] = row
    if not parent_only:
        out["sphere_points"] = _back_facing_share(rl, world, p)
    print("RESULT " + json.dumps(out), flush=True)


def _child(reps, width, lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(reps), "--width", str(width)]
    env = dict(os.environ)
    if lib:
        cmd.append("--parent-only")
        env["RL_RENDER_LIB"] = os.path.abspath(lib)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=LIMIT, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        raise RuntimeError(f"exit status {r.returncode}\n{r.stdout[-2000:]}")
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_nee_spheres.json"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-only", action="store_true")
    a = ap.parse_args()
    if a.child:
        step(a.reps, a.width, a.parent_only)
        return 0
    try:
        r = _child(a.reps, a.width, None)
        ref = r
        if a.parent_lib:  # the references from the parent's build, taken right behind this build's in the same job
            ref = _child(a.reps, a.width, a.parent_lib)
            r["parent"] = ref
            r["quad_alone_bytes_equal_the_parents"] = all(r["render_nee_mis_device:quad alone:" + h]["digest"] == ref["render_nee_mis_device:quad alone:" + h]["digest"]
                                                          for h in HEURISTICS)
    except (subprocess.TimeoutExpired, RuntimeError) as e:
        print(f"{e}; stopping", file=sys.stderr)
        return 1
    r["references_from"] = "parent" if a.parent_lib else "this build"
    plain = ref["render_moments_device"]
    for h in HEURISTICS:
        row, old = r["render_nee_mis_device:quad and sphere:" + h], ref["render_nee_mis_device:quad alone:" + h]
        row["ratio_ms_over_quad_alone"] = row["median_ms"] / old["median_ms"]
        row["ratio_ms_over_plain"] = row["median_ms"] / ref["render_independent_device"]["median_ms"]
        row["mean_over_plain_mean"] = row["mean"] / plain["mean"]
        row["quad_alone_mean_over_plain_mean"] = old["mean"] / plain["mean"]
        row["efficiency_vs_plain"] = (plain["variance"] * ref["render_independent_device"]["median_ms"]) / (row["variance"] * row["median_ms"])
    print(json.dumps(r), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(r, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
