#!/usr/bin/env python3
"""Pixel-list renders (rl_rtiow_render_pixels_device) against the two ways a host got single pixels before them:

  small   lists of 1, 64, 1 k and 16 k pixels of a 1920x1080 frame at the scene's own samples per pixel: render_pixels_device next to
          (a) render_device of the whole frame and (b) the S-launch composition get_rays_device + ray_color_rays_device per sample,
          cursors carried from sample to sample (what tests/test_gpu_path_query.py builds); the list's sums are checked against the
          composition's (same bits) wherever both ran
  full    the whole 1920x1080 frame as a list, row-major and in a random permutation, at --full-spp samples, next to render_device; the
          list's output is checked against the frame (same bits)
  cross   sphere scenes: lists of 4 k ... the whole frame (a prefix of a random permutation, --full-spp samples) through the cooperative
          one-wave-per-pixel kernel (its length bound lifted) and through the reference-order kernel (rl_debug_set_coop(0)): where the
          automatic choice of choose_rtiow_pixels_kernel has to change sides
  headline  `bench.py --gpus 1 --steps 5 --warmup 2` on the library --parent-lib names and on the product library, alternating,
          --headline-rounds rounds: the headline figure of each run and the spread of each pair

Device-resident buffers, HIP events on the launch stream, --warm warm-up and --reps timed repetitions (2 / 3 for the steps that render
whole frames at full spp), median [min, max].  The parent process never opens the GPU: every step runs in a child of its own under
`timeout -k 10`, and the first failing step ends the run.  --only baseline times (a) and (b) alone: with RL_RENDER_LIB pointing at a
build of the parent commit that is the comparison DESIGN.md §3.13 reports; RL_RENDER_PIXELS_TAG (e.g. "@parent") is appended to the step's
key and names the library in the record.
Results: profiles/render_pixels.json (merged per step) and one JSON line per step on stdout.

usage: tools/render_pixels_ab.py [--reps 10] [--steps small:bouncing_spheres,small:cornell_smoke,full:cow_scene,full:bouncing_spheres,cross:bouncing_spheres]
                                 [--only all|list|baseline] [--full-spp 16] [--parent-lib FILE (adds the headline step)] [--out FILE]   (GPU)"""
import argparse
import gzip
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420
SIZES = (1, 64, 1024, 16384)


def _stats(ms):
    import numpy as np
    a = np.sort(np.asarray(ms))
    return {"median_ms": float(np.median(a)), "min_ms": float(a[0]), "max_ms": float(a[-1]), "reps": int(a.size)}


def _time(fn, reps, warm, torch):
    for _ in range(warm):
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


def _dev_u32(torch, np, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to("cuda:0")


def step_small(rl, name, reps, warm, only, out):
    import numpy as np
    import torch
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name)
    cam = rl.Camera(p)
    W, H, S = cam.c.image_width, cam.c.image_height, p.samples_per_pixel
    out.update(width=W, height=H, samples_per_pixel=S, max_depth=p.max_depth)
    if only in ("all", "baseline"):
        frame = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
        out["render_device_full_frame"] = _time(lambda: cam.render_device(world, frame.data_ptr(), stream=s0), min(reps, 3), 1, torch)
        api.render_status(world, allow_degenerate=True)
    idx = np.random.default_rng(1).permutation(W * H)
    for n in SIZES:
        ys, xs = np.divmod(idx[:n].astype(np.uint64), np.uint64(W))
        d_xs, d_ys = _dev_u32(torch, np, xs), _dev_u32(torch, np, ys)
        r = out.setdefault(f"n{n}", {"pixels": n})
        d_list = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
        if only in ("all", "list"):
            r["render_pixels_device"] = _time(lambda: cam.render_pixels_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, d_list.data_ptr(), stream=s0),
                                              reps, warm, torch)
            r["list_rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
        if only in ("all", "baseline"):
            cur0 = api.pack_cursors(xs * np.uint64(W) + ys)  # sample 0's stream; sample s adds s * W * H below
            d_cur0 = torch.from_numpy(cur0.view(np.uint8).reshape(n, 16).copy()).to("cuda:0")
            d_cur = torch.zeros_like(d_cur0)
            d_rays = torch.zeros((n, 56), dtype=torch.uint8, device="cuda:0")
            d_rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
            d_acc = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
            step_words = torch.zeros((n, 2), dtype=torch.int64, device="cuda:0")
            step_words[:, 0] = W * H  # cursor = {stream u64, word_pos u64}: the next sample's stream, the word position kept

            def compose():
                d_cur.copy_(d_cur0)
                d_acc.zero_()
                for _ in range(S):
                    cam.get_rays_device(d_xs.data_ptr(), d_ys.data_ptr(), d_cur.data_ptr(), d_rays.data_ptr(), d_cur.data_ptr(), n, stream=s0)
                    world.ray_color_rays_device(d_rays.data_ptr(), d_cur.data_ptr(), n, p.seed, p.max_depth, p.background, d_rgb.data_ptr(), d_cur.data_ptr(),
                                                0, stream=s0)
                    d_acc.add_(d_rgb)
                    d_cur.view(torch.int64).add_(step_words)
            r["camera_rays_plus_ray_color_rays_S_launches"] = _time(compose, min(reps, 5), 1, torch)
            api.render_status(world, allow_degenerate=True)
            if only == "all":
                r["same_bits_as_composition"] = bool(torch.equal(d_acc, d_list))
        if only == "all":
            lst = r["render_pixels_device"]["median_ms"]
            r["full_frame_over_list"] = out["render_device_full_frame"]["median_ms"] / lst
            r["composition_over_list"] = r["camera_rays_plus_ray_color_rays_S_launches"]["median_ms"] / lst


def step_full(rl, name, reps, warm, only, out, spp):
    import dataclasses
    import numpy as np
    import torch
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name)
    cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=spp))
    W, H = cam.c.image_width, cam.c.image_height
    n = W * H
    out.update(width=W, height=H, samples_per_pixel=spp, max_depth=p.max_depth, pixels=n)
    frame = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    if only in ("all", "baseline"):
        out["render_device"] = _time(lambda: cam.render_device(world, frame.data_ptr(), stream=s0), reps, warm, torch)
        out["render_rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
    if only in ("all", "list"):
        orders = {"row_major": np.arange(n), "permutation": np.random.default_rng(2).permutation(n)}
        for key, idx in orders.items():
            ys, xs = np.divmod(idx, W)
            d_xs, d_ys = _dev_u32(torch, np, xs), _dev_u32(torch, np, ys)
            d_list = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
            r = _time(lambda: cam.render_pixels_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, d_list.data_ptr(), stream=s0), reps, warm, torch)
            out[f"render_pixels_device_{key}"] = r
            out["list_rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
            if only == "all":
                d_idx = torch.from_numpy(idx).to("cuda:0")
                out[f"same_bits_{key}"] = bool(torch.equal(frame.reshape(n, 3)[d_idx], d_list))
                out[f"list_over_frame_{key}"] = r["median_ms"] / out["render_device"]["median_ms"]


def step_cross(rl, name, reps, warm, out, spp):
    import dataclasses
    import numpy as np
    import torch
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name)
    cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=spp))
    W, H = cam.c.image_width, cam.c.image_height
    idx = np.random.default_rng(2).permutation(W * H)
    name_buf = __import__("ctypes").create_string_buffer(64)
    cus = api.render_lib().rl_device_info(name_buf, 64)
    out.update(width=W, height=H, samples_per_pixel=spp, max_depth=p.max_depth, compute_units=cus)
    for n in (4096, 16384, cus * 160, 65536, 262144, W * H):
        ys, xs = np.divmod(idx[:n], W)
        d_xs, d_ys = _dev_u32(torch, np, xs), _dev_u32(torch, np, ys)
        d_a = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
        d_b = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
        r = out.setdefault(f"n{n}", {"pixels": n})
        api.set_coop(True), api.set_coop_pixels_max(1 << 40)
        r["cooperative"] = _time(lambda: cam.render_pixels_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, d_a.data_ptr(), stream=s0), reps, warm, torch)
        api.set_coop(False)
        r["reference_order"] = _time(lambda: cam.render_pixels_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, d_b.data_ptr(), stream=s0), reps, warm, torch)
        api.set_coop(True), api.set_coop_pixels_max(0)
        r["rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
        r["same_bits"] = bool(torch.equal(d_a, d_b))
        r["cooperative_over_reference_order"] = r["cooperative"]["median_ms"] / r["reference_order"]["median_ms"]


def headline(parent_lib, results, out_path, rounds):
    """bench.py on the parent's library and on the product library, alternating; every run a child process under its own time limit."""
    runs = {"parent": [], "branch": []}
    for _ in range(rounds):
        for which in ("parent", "branch"):
            env = dict(os.environ)
            env.pop("RL_RENDER_LIB", None)
            if which == "parent":
                env["RL_RENDER_LIB"] = parent_lib
            cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                print(f"headline ({which}): exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
                return 1
            d = json.loads(line[-1])
            runs[which].append({"Mrays_s": d["value"], "ms_per_step": d["ms_per_step"], "check": d.get("check", {}).get("timed_frame_equals_counting_frame")})
    rec = {"step": "headline", "cmd": "bench.py --gpus 1 --steps 5 --warmup 2", "runs": runs}
    for which in runs:
        v = [x["Mrays_s"] for x in runs[which]]
        rec[which + "_mean_Mrays_s"], rec[which + "_spread_Mrays_s"] = sum(v) / len(v), max(v) - min(v)
    rec["branch_over_parent"] = rec["branch_mean_Mrays_s"] / rec["parent_mean_Mrays_s"]
    results["headline"] = rec
    print(json.dumps(rec), flush=True)
    with open(out_path, "w") as f:
        json.dump(results, f, indent=1, sort_keys=True)
        f.write("\n")
    return 0


def step(what, reps, warm, only, full_spp):
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    kind, name = what.split(":")
    tag = os.environ.get("RL_RENDER_PIXELS_TAG", "").lstrip("@")
    out = {"step": what, "library": (tag or "RL_RENDER_LIB") if os.environ.get("RL_RENDER_LIB") else "product", "only": only}
    if kind == "cross":
        step_cross(rl, name, reps, warm, out, full_spp)
    elif kind == "small":
        step_small(rl, name, reps, warm, only, out)
    else:
        step_full(rl, name, reps, warm, only, out, full_spp)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--steps", default="small:bouncing_spheres,small:cornell_smoke,full:cow_scene,full:bouncing_spheres,cross:bouncing_spheres")
    ap.add_argument("--headline-rounds", type=int, default=4)
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit: adds the headline step (bench.py on both libraries)")
    ap.add_argument("--only", default="all", choices=("all", "list", "baseline"))
    ap.add_argument("--full-spp", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_pixels.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.warm, a.only, a.full_spp)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    tag = os.environ.get("RL_RENDER_PIXELS_TAG", "")
    for what in [w for w in a.steps.split(",") if w]:
        if what.startswith("cross:") and a.only == "baseline":
            continue  # the parent commit has no list render
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps), "--warm", str(a.warm),
               "--only", a.only, "--full-spp", str(a.full_spp)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {what}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
            return 1
        results[what + tag] = json.loads(line[-1][7:])
        print(line[-1][7:], flush=True)
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
    if a.parent_lib:
        return headline(os.path.abspath(a.parent_lib), results, a.out, a.headline_rounds)
    return 0


if __name__ == "__main__":
    sys.exit(main())
