#!/usr/bin/env python3
"""Seeded path queries against the render that traces the same paths: get_rays_device + ray_color_rays_device of one sample per pixel
(and of 8 samples per pixel submitted as ONE batch) next to render_independent_device at 1 spp (8 spp) of the same 1920x1080 frame —
the same work through the camera.  Device-resident buffers, HIP events on the launch stream, 3 warm-up and --reps timed repetitions,
median [min, max]; the query's colours folded per pixel are checked against the render's frame (same bits).  The parent process never
opens the GPU: every step runs in a child of its own under `timeout -k 10`, and the first failing step ends the run.  RL_RENDER_LIB
selects the library of the render side's --only render run (a build of the parent commit gives the comparison DESIGN.md §3.9 reports).
Results: profiles/path_query.json (merged per step) and one JSON line per step on stdout.

usage: tools/path_query_ab.py [--reps 20] [--steps bouncing_spheres,cow_scene,cornell_smoke] [--only both|query|render] [--out FILE]   (GPU)"""
import argparse
import gzip
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 400


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


def _world(rl, np, name):
    G = os.path.join(ROOT, "tests", "golden")
    if name == "bouncing_spheres":
        w = rl.World.bouncing_spheres(1)
    elif name == "cow_scene":
        from PIL import Image
        tex = np.asarray(Image.open(os.path.join(G, "spot_texture.png")).convert("RGB"))
        w = rl.World.cow_scene(gzip.open(os.path.join(G, "spot_triangulated.obj.gz"), "rb").read(), tex)
    else:
        w = rl.World.example_scene(name)
    p = w.params
    p.aspect_ratio, p.image_width = 16.0 / 9.0, 1920
    return w, p


def step(name, reps, only):
    import dataclasses
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    api = rl.api
    rl.init(0)
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name)
    out = {"step": name, "library": os.environ.get("RL_RENDER_LIB", "product")}
    for S in (1, 8):
        cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=S))
        W, H = cam.c.image_width, cam.c.image_height
        n = W * H * S
        frame = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        key = f"{S}spp"
        out[key] = {"paths": n, "width": W, "height": H}
        if only in ("both", "render"):
            r = _time(lambda: cam.render_independent_device(world, frame.data_ptr(), stream=s0), reps, torch)
            out[key].update(render_independent_device=r, render_rays=int(api.render_status(world)["rays"]))
        if only in ("both", "query"):
            s, y, x = np.meshgrid(np.arange(S, dtype=np.uint64), np.arange(H, dtype=np.uint64), np.arange(W, dtype=np.uint64), indexing="ij")
            cur0 = api.pack_cursors((s * np.uint64(W * H) + x * np.uint64(W) + y).reshape(-1))
            d_px = torch.from_numpy(x.reshape(-1).astype(np.uint32)).to("cuda:0")
            d_py = torch.from_numpy(y.reshape(-1).astype(np.uint32)).to("cuda:0")
            d_cur0 = torch.from_numpy(cur0.view(np.uint8).reshape(n, 16).copy()).to("cuda:0")
            d_cur = torch.zeros_like(d_cur0)
            d_rays = torch.zeros((n, 56), dtype=torch.uint8, device="cuda:0")
            d_rgb = torch.zeros((S, H, W, 3), dtype=torch.float64, device="cuda:0")
            d_cnt = torch.zeros(n, dtype=torch.int32, device="cuda:0")

            def query():
                cam.get_rays_device(d_px.data_ptr(), d_py.data_ptr(), d_cur0.data_ptr(), d_rays.data_ptr(), d_cur.data_ptr(), n, stream=s0)
                world.ray_color_rays_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, p.max_depth, p.background, d_rgb.data_ptr(), d_cur.data_ptr(),
                                            d_cnt.data_ptr(), stream=s0)
            q = _time(query, reps, torch)
            st = api.render_status(world)
            g = _time(lambda: cam.get_rays_device(d_px.data_ptr(), d_py.data_ptr(), d_cur0.data_ptr(), d_rays.data_ptr(), d_cur.data_ptr(), n, stream=s0),
                      reps, torch)
            out[key].update(get_rays_plus_ray_color_rays_device=q, get_rays_device=g, query_rays=int(st["rays"]), retraced=int(st["slow_traces"]),
                            served_by=api.last_query()["kernel"], query_mrays_per_s=st["rays"] / q["median_ms"] / 1e3)
            if only == "both":
                acc = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
                for k in range(S):
                    acc = acc + d_rgb[k]
                cam.render_independent_device(world, frame.data_ptr(), stream=s0)
                api.render_status(world)
                out[key].update(same_bits=bool(torch.equal(acc, frame)),
                                ratio_query_over_render=q["median_ms"] / out[key]["render_independent_device"]["median_ms"])
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="bouncing_spheres,cow_scene,cornell_smoke")
    ap.add_argument("--only", default="both", choices=("both", "query", "render"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "path_query.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.only)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    tag = os.environ.get("RL_PATH_QUERY_TAG", "")
    for name in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--only", a.only]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {name}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
            return 1
        results[name + tag] = json.loads(line[-1][7:])
        print(line[-1][7:], flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
