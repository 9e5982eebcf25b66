#!/usr/bin/env python3
"""Seeded hit queries, measured.  Per step, on the 1920x1080 frame's camera rays (one per pixel):

  cornell_smoke     hit_rays_seeded_device (counter-free, the reference-order fold with media) next to the counter-free
                    ray_color_rays_device of the same rays and cursors at max_depth = 1: the nearest thing a library without the seeded
                    hit can do with a media scene (one Hittable::hit per path, then the material's scatter and a colour instead of a hit
                    record).  That side is to be run on a build of the PARENT commit: RL_RENDER_LIB=<its librl_render.so> with --only color
                    and RL_SEEDED_HIT_QUERY_TAG=_parent (this change also corrects Ring::low for cursors at odd positions, which rebuilds
                    the kernels behind ray_color_rays).  The product library's own ray_color_rays is timed too, in the seeded call's process.
  cornell_smoke_odd the same two calls from cursors at word 7 (word 13 behind get_rays): the positions at which Ring::low changed, so the
                    product / parent pair of this step is the cost of that correction on ray_color_rays.
  bouncing_spheres  hit_rays_seeded_device next to the bare hit_rays_device of the same rays.  No media: both run the same kernel, so the
                    difference is the cursor pass-through (a device-to-device copy of 16 B per ray; none when the output cursors are the
                    input's buffer).  The records are compared (same bits).

Device-resident buffers, HIP events on the launch stream, 3 warm-up and --reps timed repetitions, median [min, max], both sides of a step
in one process.  The parent process never opens the GPU: every step runs in a child of its own under `timeout -k 10`, and the first
failing step ends the run.  Results: profiles/seeded_hit_query.json (merged per step) and one JSON line per step on stdout.

usage: tools/seeded_hit_query_ab.py [--reps 20] [--steps cornell_smoke,cornell_smoke_odd,bouncing_spheres] [--only all|color] [--out FILE]   (GPU)"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300


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


def step(name, reps, only):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    api = rl.api
    rl.init(0)
    dev = "cuda:0"
    s0 = torch.cuda.current_stream().cuda_stream
    odd = name.endswith("_odd")
    world = rl.World.bouncing_spheres(1) if name == "bouncing_spheres" else rl.World.example_scene(name[:-4] if odd else name)
    p = world.params
    p.aspect_ratio, p.image_width, p.samples_per_pixel = 16.0 / 9.0, 1920, 1
    cam = rl.Camera(p)
    W, H = cam.c.image_width, cam.c.image_height
    n = W * H
    y, x = np.divmod(np.arange(n, dtype=np.uint64), W)
    cur0 = api.pack_cursors(x * np.uint64(W) + y, 7 if odd else 0)
    d_px = torch.from_numpy(x.astype(np.uint32).view(np.int32)).to(dev)
    d_py = torch.from_numpy(y.astype(np.uint32).view(np.int32)).to(dev)
    d_cur0 = torch.from_numpy(cur0.view(np.int64).reshape(n, 2).copy()).to(dev)
    d_cur = torch.zeros_like(d_cur0)
    d_rays = torch.zeros((n, 7), dtype=torch.float64, device=dev)
    cam.get_rays_device(d_px.data_ptr(), d_py.data_ptr(), d_cur0.data_ptr(), d_rays.data_ptr(), d_cur.data_ptr(), n, stream=s0)
    torch.cuda.synchronize()
    media = world.counts()["media"]
    out = {"step": name, "library": os.environ.get("RL_RENDER_LIB", "product"), "rays": n, "width": W, "height": H, "media": int(media)}
    d_hits = torch.zeros((n, 11), dtype=torch.float64, device=dev)
    d_end = torch.zeros_like(d_cur)
    if media:
        d_rgb = torch.zeros((n, 3), dtype=torch.float64, device=dev)

        def color():
            world.ray_color_rays_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, 1, p.background, d_rgb.data_ptr(), d_end.data_ptr(), stream=s0)
        out["ray_color_rays_device_depth1"] = _time(color, reps, torch)
        api.render_status(world, allow_degenerate=True)
        out["ray_color_rays_kernel"] = api.last_query()["kernel"]
        depth = min(p.max_depth, 20)  # whole paths: many shades per cursor, which is where Ring::low decides between FILL and the inline refill

        def paths():
            world.ray_color_rays_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, depth, p.background, d_rgb.data_ptr(), d_end.data_ptr(), stream=s0)
        out["ray_color_rays_device_depth%d" % depth] = _time(paths, reps, torch)
        out["paths_rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
    else:
        def bare():
            world.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s0)
        out["hit_rays_device"] = _time(bare, reps, torch)
        api.render_status(world, allow_degenerate=True)
        out["hit_rays_kernel"] = api.last_query()["kernel"]
    if only == "all":
        d_seeded = torch.zeros_like(d_hits)

        def seeded():
            world.hit_rays_seeded_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, d_seeded.data_ptr(), d_end.data_ptr(), stream=s0)
        out["hit_rays_seeded_device"] = _time(seeded, reps, torch)
        st = api.render_status(world, allow_degenerate=True)
        out["hit_rays_seeded_kernel"] = api.last_query()["kernel"]
        out["seeded_status_rays"] = int(st["rays"])
        out["hits"] = int(((d_seeded.view(torch.int64)[:, 9] & 0xFFFFFFFF) != 0).sum())
        out["rays_that_drew"] = int((d_end[:, 1] != d_cur[:, 1]).sum())
        if media:
            out["ratio_seeded_hit_over_ray_color_depth1"] = out["hit_rays_seeded_device"]["median_ms"] / out["ray_color_rays_device_depth1"]["median_ms"]
        else:
            d_alias = d_cur.clone()

            def in_place():
                world.hit_rays_seeded_device(d_rays.data_ptr(), d_alias.data_ptr(), n, p.seed, d_seeded.data_ptr(), d_alias.data_ptr(), stream=s0)
            out["hit_rays_seeded_device_cursors_in_place"] = _time(in_place, reps, torch)
            api.render_status(world, allow_degenerate=True)
            out["same_bits"] = bool(torch.equal(d_seeded.view(torch.int64), d_hits.view(torch.int64)) and torch.equal(d_end, d_cur) and torch.equal(d_alias, d_cur))
            out["ratio_seeded_over_bare"] = out["hit_rays_seeded_device"]["median_ms"] / out["hit_rays_device"]["median_ms"]
            out["ratio_seeded_in_place_over_bare"] = out["hit_rays_seeded_device_cursors_in_place"]["median_ms"] / out["hit_rays_device"]["median_ms"]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="cornell_smoke,cornell_smoke_odd,bouncing_spheres")
    ap.add_argument("--only", default="all", choices=("all", "color"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seeded_hit_query.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.only)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    tag = os.environ.get("RL_SEEDED_HIT_QUERY_TAG", "")
    for name in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--only", a.only]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
            return 1
        results[name + tag] = json.loads(line[-1][7:])
        print(line[-1][7:], flush=True)
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
