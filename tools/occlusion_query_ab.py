#!/usr/bin/env python3
"""Occlusion queries against the hit query on the same buffers: ms of occluded_rays_device next to hit_rays_device (the existing query is
the yardstick) for two workloads per scene — the pixel-centre rays of a 1920x1080 frame, tmax = inf, and the shadow segments from those
rays' hit points to one point above the scene, dir = L - p, tmax = 1.  Device-resident buffers, HIP events on the launch stream, 3
warm-up + --reps timed repetitions, median [min, max]; the rays each fast kernel re-traced in the reference's order are recorded too.
The parent process never opens the GPU: every step runs in a child of its own under a time limit, and the first failing step ends the
run.  Results: profiles/occlusion_query.json (merged per step) and one JSON line per step on stdout.

usage: tools/occlusion_query_ab.py [--reps 20] [--steps bouncing,stress60] [--out profiles/occlusion_query.json]        (GPU)
steps: bouncing = bouncing_spheres(1); stress60 = stress_scene(60, 1): 3,600 spheres and the cow mesh subdivided once."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"bouncing": 300, "stress60": 300}


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


def _pixel_centre_rays(np, cam):  # camera.rs:232-262 without the sample offset and the defocus disc: lookfrom -> pixel centre
    c = cam.c
    W, H = c.image_width, c.image_height
    x, y = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    p00, du, dv, eye = (np.array(list(v)) for v in (c.pixel_00, c.pixel_du, c.pixel_dv, c.lookfrom))
    centre = (p00 + x.reshape(-1, 1) * du) + y.reshape(-1, 1) * dv
    return np.tile(eye, (W * H, 1)), centre - eye


def _workload(rl, world, o, d, tmax, reps, np, torch):
    """Both queries on one device-resident batch: timings, re-traced rays, and whether the bytes agree."""
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    n = o.shape[0]
    rays = api.pack_rays(o, d)
    d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 56).copy()).to("cuda:0")
    d_hits = torch.zeros((n, 88), dtype=torch.uint8, device="cuda:0")
    d_occ = torch.zeros((n,), dtype=torch.uint8, device="cuda:0")
    out = {"rays": n, "tmax": "inf" if tmax == float("inf") else tmax}
    calls = {"hit_rays_device": lambda: world.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, tmax=tmax, stream=s0),
             "occluded_rays_device": lambda: rl.occluded_rays_device(world, d_rays.data_ptr(), d_occ.data_ptr(), n, tmax=tmax, stream=s0)}
    for name, fn in calls.items():
        out[name] = _time(fn, reps, torch)
        out[name]["served_by"] = api.last_query()["kernel"]
        api.render_status(world)
        fn()
        out[name]["retraced"] = int(api.render_status(world)["slow_traces"])
    hits = d_hits.cpu().numpy().reshape(-1).view(api.RTIOW_HIT)
    occ = d_occ.cpu().numpy()
    out["occluded"] = int(occ.sum())
    out["same_bytes"] = bool(np.array_equal(occ, hits["hit"].astype(np.uint8)))
    out["ratio_occluded_over_hit"] = out["occluded_rays_device"]["median_ms"] / out["hit_rays_device"]["median_ms"]
    return out, hits


def step(name, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    if name == "bouncing":
        world = rl.World.bouncing_spheres(1)
    else:
        from PIL import Image
        import gzip
        G = os.path.join(ROOT, "tests", "golden")
        tex = np.asarray(Image.open(os.path.join(G, "spot_texture.png")).convert("RGB"))
        world = rl.World.stress_scene(60, 1, gzip.open(os.path.join(G, "spot_triangulated.obj.gz"), "rb").read(), tex)
    p = world.params
    p.aspect_ratio, p.image_width = 16.0 / 9.0, 1920
    cam = rl.Camera(p)
    o, d = _pixel_centre_rays(np, cam)
    frame, hits = _workload(rl, world, o, d, float("inf"), reps, np, torch)
    eye, target = np.array(p.lookfrom, dtype=np.float64), np.array(p.lookat, dtype=np.float64)
    L = target + float(np.linalg.norm(target - eye)) * np.array([0.3, 1.5, 0.2])  # above the scene, off every axis and plane of symmetry
    hit = hits["hit"] == 1
    pts = hits["p"][hit]
    shadow, _ = _workload(rl, world, pts, L - pts, 1.0, reps, np, torch)
    out = {"step": name, "width": cam.c.image_width, "height": cam.c.image_height, "light": [float(v) for v in L], "frame_rays": frame, "shadow_segments": shadow,
           "render_lib": os.path.basename(rl.api.RENDER_LIB)}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="bouncing,stress60")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "occlusion_query.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for name in a.steps.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps)], stdout=subprocess.PIPE, text=True,
                               timeout=LIMITS[name])
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
