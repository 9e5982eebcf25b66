#!/usr/bin/env python3
"""A/B of the chained render (rl_rtiow_render_device) against the sample-parallel mode with independent sample streams
(rl_rtiow_render_independent_device), alternately in one process: per case and per repetition one chained and one independent frame
(for every claim size K of --k), HIP events on the launch stream, rays from rl_render_status.  One JSON line per timed frame.

usage: tools/indep_ab.py [--reps 2] [--k 1,2,4] [--only name,...] [--out file.jsonl]        (GPU)
cases: final_scene 400x400, teapot, cornell_smoke, checkered_spheres (the examples' own settings), configs[1] (bouncing_spheres
1920x1080, 1024 spp, depth 50) whole and its 1/4 and 1/8 row shards (row_first 0, row_step 4 / 8)."""
import argparse
import importlib
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
G = os.path.join(ROOT, "tests", "golden")


def cases(rl):
    from PIL import Image
    tex = np.asarray(Image.open(os.path.join(G, "spot_texture.png")).convert("RGB"))
    out = []
    for name, kw in (("final_scene", dict(rgb8=tex)), ("teapot", dict(obj_text=open(os.path.join(G, "teapot-low.obj"), "rb").read())),
                     ("cornell_smoke", {}), ("checkered_spheres", {})):
        w = rl.World.example_scene(name, **kw)
        out.append((f"{name} {w.params.image_width}x{int(w.params.image_width / w.params.aspect_ratio)}", w, w.params, 0, 1))
    w = rl.World.bouncing_spheres(1)
    p = w.params
    p.image_width, p.samples_per_pixel, p.max_depth = 1920, 1024, 50
    for step, label in ((1, "configs[1] 1920x1080"), (4, "configs[1] 1/4 shard"), (8, "configs[1] 1/8 shard")):
        out.append((label, w, p, 0, step))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--k", default="1")
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev)
    ks = [int(k) for k in a.k.split(",")]
    sink = open(a.out, "a") if a.out else None

    def timed(fn, world):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        st = rl.api.render_status(world)
        torch.cuda.synchronize(dev)
        return e0.elapsed_time(e1), st["rays"]

    for label, w, p, row_first, row_step in cases(rl):
        if a.only and not any(o in label for o in a.only.split(",")):
            continue
        cam = rl.Camera(p)
        nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
        buf = torch.zeros((nrows, cam.c.image_width, 3), dtype=torch.float64, device=dev)
        warm = rl.Camera(rl.CameraParams(**{**p.__dict__, "samples_per_pixel": 1}))
        warm.render_device(w, buf.data_ptr(), stream=stream.cuda_stream, row_first=row_first, row_step=row_step)
        warm.render_independent_device(w, buf.data_ptr(), stream=stream.cuda_stream, row_first=row_first, row_step=row_step)
        rl.api.render_status(w)
        legs = [("chained", None)] + [("independent", k) for k in ks]
        for rep in range(a.reps):
            for mode, k in legs:
                if mode == "chained":
                    fn = lambda: cam.render_device(w, buf.data_ptr(), stream=stream.cuda_stream, row_first=row_first, row_step=row_step)  # noqa: E731
                else:
                    rl.api.set_indep_k(k)
                    fn = lambda: cam.render_independent_device(w, buf.data_ptr(), stream=stream.cuda_stream, row_first=row_first, row_step=row_step)  # noqa: E731
                ms, rays = timed(fn, w)
                rec = {"case": label, "mode": mode, "k": k, "rep": rep, "spp": p.samples_per_pixel, "depth": p.max_depth,
                       "pixels": nrows * cam.c.image_width, "ms": round(ms, 2), "rays": rays, "Mrays_s": round(rays / ms / 1e3, 1)}
                print(json.dumps(rec), flush=True)
                if sink:
                    sink.write(json.dumps(rec) + "\n")
                    sink.flush()
        rl.api.set_indep_k(1)


if __name__ == "__main__":
    main()
