#!/usr/bin/env python3
"""The a-trous denoiser (rl_denoise_atrous_pass_device): what one pass costs on each route, beside a copy of the same
bytes and beside the render it follows, and what it does to a noisy image.

  passes    1920x1080, G = 8 guides, seeded random images resident on the device: one pass at step 1, 2, 4, 8, 16 on either
            route (taps from the images; one lattice's tile and halo staged in LDS), the routes alternating repetition by
            repetition.  In the same run a device-to-device copy that moves the bytes a pass must move: a pass reads (6 + G) and writes 6
            doubles per pixel, a copy of n bytes reads n and writes n, so the copy is of (12 + G) * 4 bytes per pixel.  pass / copy is the
            fraction of the achievable bandwidth a pass reaches (achievable: what the copy reaches, not a nominal figure).
  render    the 16-spp render_moments_device + render_features_device of bouncing_spheres at 1920x1080 the filter would follow, and the
            five passes (step 1 .. 16) of the default routes after it
  quality   bouncing_spheres at 64x48: render_moments + render_features at 4 spp through denoise_render against a 1024-spp render; the
            mean squared errors and their ratio (what tests/test_gpu_denoise.py asserts to be below 1), also at 16 spp

HIP events on the launch stream, --warm warm-ups and --reps timed repetitions (passes and copies: ten calls per repetition), median
[min, max].  The parent process never opens the GPU:
every step runs in a child of its own under `timeout -k 10`, and the first failing step ends the run.
Results: profiles/denoise.json (merged per step) and one JSON line per step on stdout.

usage: tools/denoise_ab.py [--reps 20] [--warm 3] [--steps passes,render,quality] [--out FILE]"""
import argparse
import dataclasses
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from render_moments_ab import LIMIT_S, _stats, _time, _world  # noqa: E402  (the same timing and scenes)

W, H, G = 1920, 1080, 8
STEPS = (1, 2, 4, 8, 16)
INNER = 10


def step_passes(rl, reps, warm, out):
    import torch
    api = rl.api
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    color = torch.rand((H, W, 3), dtype=torch.float64, device=dev, generator=gen)
    variance = torch.rand((H, W, 3), dtype=torch.float64, device=dev, generator=gen) * 0.01
    guides = torch.rand((H, W, G), dtype=torch.float64, device=dev, generator=gen)
    out_c, out_v = torch.empty_like(color), torch.empty_like(color)
    p = api.atrous_params(G)
    s0 = torch.cuda.current_stream().cuda_stream
    npix = W * H
    read_b, write_b = npix * (6 + G) * 8, npix * 6 * 8
    out.update(width=W, height=H, n_guides=G, pass_reads_bytes=read_b, pass_writes_bytes=write_b)
    src = torch.empty((read_b + write_b) // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    out["copy_bytes_each_way"] = int(src.numel())

    def one(step, route):
        api.set_denoise_route(route)
        api.denoise_atrous_pass_device(W, H, step, p, color.data_ptr(), variance.data_ptr(), guides.data_ptr(), out_c.data_ptr(), out_v.data_ptr(), stream=s0)

    def timed(fn):  # INNER back-to-back calls between two events: a single pass is too short a window
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(INNER):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / INNER

    def copy_time():
        for _ in range(warm):
            dst.copy_(src)
        return _stats([timed(lambda: dst.copy_(src)) for _ in range(reps)])

    out["calls_per_timed_window"] = INNER
    out["copy_before"] = copy_time()
    results = {}
    for step in STEPS:
        routes = [("images", 0), ("lds", 1)]
        ref = None
        for name, r in routes:  # warm-up; and the routes' outputs are the same bytes at the size that is timed
            for _ in range(warm):
                one(step, r)
            torch.cuda.synchronize()
            assert api.last_denoise_route() == name
            got = (out_c.clone(), out_v.clone())
            assert ref is None or (torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])), f"routes differ at step {step}"
            ref = got
        ms = {name: [] for name, _ in routes}
        for _ in range(reps):
            for name, r in routes:
                ms[name].append(timed(lambda: one(step, r)))
        results[str(step)] = {name: _stats(v) for name, v in ms.items()}
    api.set_denoise_route(-1)
    out["copy_after"] = copy_time()
    copy_ms = min(out["copy_before"]["median_ms"], out["copy_after"]["median_ms"])
    out["copy_GBps_moved"] = (read_b + write_b) / copy_ms / 1e6
    for step, rec in results.items():
        for name in ("images", "lds"):
            if name in rec:
                rec[name]["copy_over_pass"] = copy_ms / rec[name]["median_ms"]  # the fraction of the copy's bandwidth the pass reaches
        one(int(step), -1)
        torch.cuda.synchronize()
        rec["default_route"] = api.last_denoise_route()
    out["step"] = results


def step_render(rl, reps, warm, out):
    import numpy as np
    import torch
    api = rl.api
    dev = "cuda:0"
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, "bouncing_spheres", 16)
    p = dataclasses.replace(p, samples_per_pixel=16)
    cam = rl.Camera(p)
    w, h = cam.c.image_width, cam.c.image_height
    n = w * h
    out.update(width=w, height=h, samples_per_pixel=16)
    sums, sq = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    albedo, normal = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 3), dtype=torch.float64, device=dev)
    depth, count = torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)

    def render():
        cam.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0)
        cam.render_features_device(world, stream=s0, d_albedo_sum=albedo.data_ptr(), d_normal_sum=normal.data_ptr(), d_depth_sum=depth.data_ptr(),
                                   d_hit_count=count.data_ptr(), allow_degenerate=True)

    out["render_moments_plus_features"] = _time(render, max(3, reps // 4), 1, torch)
    api.render_status(world, allow_degenerate=True)
    guides = torch.rand((n, G), dtype=torch.float64, device=dev)
    var = sq * 1e-3
    work = [[torch.empty_like(sums), torch.empty_like(sums)] for _ in range(2)]
    prm = api.atrous_params(G)

    def denoise():
        src = [sums, var]
        for it, step in enumerate(STEPS):
            dst = work[it & 1]
            api.denoise_atrous_pass_device(w, h, step, prm, src[0].data_ptr(), src[1].data_ptr(), guides.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), stream=s0)
            src = dst

    out["five_passes_default_routes"] = _time(denoise, reps, warm, torch)
    out["denoise_over_render"] = out["five_passes_default_routes"]["median_ms"] / out["render_moments_plus_features"]["median_ms"]


def step_quality(rl, out):
    import numpy as np
    api = rl.api
    world = rl.World.bouncing_spheres(1)
    base = dataclasses.replace(world.params, image_width=64, aspect_ratio=64 / 48.5)
    truth = rl.Camera(dataclasses.replace(base, samples_per_pixel=1024)).render(world).pixel_data()
    for spp in (4, 16):
        cam = rl.Camera(dataclasses.replace(base, samples_per_pixel=spp))
        moments, features = cam.render_moments(world), cam.render_features(world)
        noisy = moments.sums * (1.0 / spp)
        color, _ = api.denoise_render(moments, features)
        before, after = float(np.mean((noisy - truth) ** 2)), float(np.mean((color - truth) ** 2))
        out[f"{spp}spp"] = {"width": 64, "height": 48, "mse_noisy": before, "mse_denoised": after, "ratio": after / before}
    out["defaults"] = {"iterations": 5, "color_sigma": api.DENOISE_COLOR_SIGMA, "variance_floor": api.DENOISE_VARIANCE_FLOOR, "guide_sigma": api.DENOISE_GUIDE_SIGMA}


def step(what, reps, warm):
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    out = {}
    if what == "passes":
        step_passes(rl, reps, warm, out)
    elif what == "render":
        step_render(rl, reps, warm, out)
    elif what == "quality":
        step_quality(rl, out)
    else:
        raise SystemExit(f"unknown step {what}")
    print("RESULT " + json.dumps(out), flush=True)


def _child(what, a):
    env = dict(os.environ)
    env.pop("RL_RENDER_LIB", None)
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps), "--warm", str(a.warm)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"step {what}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
        return None
    print(line[-1][7:], flush=True)
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--steps", default="passes,render,quality")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.warm)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for what in [w for w in a.steps.split(",") if w]:
        rec = _child(what, a)
        if rec is None:
            return 1
        results[what] = rec
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
