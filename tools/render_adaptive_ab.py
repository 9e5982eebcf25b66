#!/usr/bin/env python3
"""Adaptive renders (rl_rtiow_render_adaptive_device): what stopping pixels inside the launch buys, and what the rule costs.

  loop      one scene at S = first + more samples: a uniform render_device at S; the two-pass loop of tools/render_moments_ab.py (a `first`
            spp moments pass, the noisiest tenth of the pixels selected on the device, a list render of `more` further samples of those, a
            merge); ONE render_adaptive_device with min_samples = check_every = first and abs_variance = the 90th percentile over pixels of
            the `first` spp variance of the mean (largest channel).  Times, samples traced and rays of all three.
            bouncing_spheres at 1920x1080 (first 16, S 80), cornell_smoke at 600x600 and cow_scene at 1920x1080 (S = the sample counts of
            the moments cost step, first = S / 5)
  rule      render_moments_device, and render_adaptive_device with min_samples >= S (the rule never fires: the moments call's bytes, checked),
            in one child per library, --parent-lib and the product library alternating: the cost of the rule's presence in the MOMENTS
            kernels (moments, branch over parent) and of the mode itself (adaptive over moments, branch)
  regs      (CPU only) tools/kernel_regs.py on --parent-lib and on the product library: every kernel name without `moments` in it must show
            identical figures; the MOMENTS kernels' figures of both
  headline  `bench.py --gpus 1 --steps 5 --warmup 2 --configs ""` on --parent-lib and on the product library, alternating, three runs each

Device-resident buffers, HIP events on the launch stream, --warm warm-ups and --reps timed repetitions, median [min, max].  The parent
process never opens the GPU: every GPU step runs in a child of its own under `timeout -k 10`, and the first failing step ends the run.
Results: profiles/render_adaptive.json (merged per step) and one JSON line per step on stdout.

usage: tools/render_adaptive_ab.py [--reps 5] [--warm 1] [--spp 1024] [--steps loop:bouncing_spheres,loop:cornell_smoke,loop:cow_scene,rule:bouncing_spheres,...]
                                   [--parent-lib FILE (needed by rule, regs and headline)] [--out FILE]"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from render_moments_ab import LIMIT_S, _regs, _time, _world, headline  # noqa: E402  (the same timing, scenes and bench runs)

PRODUCT = os.path.join(ROOT, "rendering-learning_amd", "csrc", "librl_render.so")


def step_loop(rl, name, reps, warm, out):
    import dataclasses
    import numpy as np
    import torch
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name, 80)
    S = p.samples_per_pixel
    first = 16 if name == "bouncing_spheres" else max(2, S // 5)
    more = S - first
    cam1 = rl.Camera(dataclasses.replace(p, samples_per_pixel=first))
    cam2 = rl.Camera(dataclasses.replace(p, samples_per_pixel=more))
    camu = rl.Camera(dataclasses.replace(p, samples_per_pixel=S))
    W, H = cam1.c.image_width, cam1.c.image_height
    n = (W * H) // 10
    out.update(width=W, height=H, first_pass_spp=first, second_pass_spp=more, second_pass_pixels=n, uniform_spp=S, max_depth=p.max_depth)
    sums, sq = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    lsums, lsq = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
    counts = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")

    def rays():
        return int(api.render_status(world, allow_degenerate=True)["rays"])

    # uniform
    out["uniform_render_device"] = _time(lambda: camu.render_device(world, sums.data_ptr(), stream=s0), reps, warm, torch)
    out["uniform_rays"], out["uniform_samples"] = rays(), W * H * S

    # the two-pass loop
    def select():
        v = ((sq - sums * sums / first) / (first - 1) / first).clamp_(min=0.0).sum(dim=2).reshape(-1)
        idx = torch.topk(v, n).indices
        return (idx % W).to(torch.int32), (idx // W).to(torch.int32), idx

    def loop():
        cam1.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0)
        d_xs, d_ys, idx = select()
        cam2.render_pixels_moments_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, lsums.data_ptr(), lsq.data_ptr(), stream=s0, first_sample=first)
        sums.reshape(-1, 3).index_add_(0, idx, lsums)
        sq.reshape(-1, 3).index_add_(0, idx, lsq)

    out["two_pass_loop"] = _time(loop, reps, warm, torch)
    rays()
    out["two_pass_samples"] = W * H * first + n * more

    # one adaptive launch; the bound from a first-pass render of its own
    cam1.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0)
    rays()
    var = ((sq - sums * sums / first) / (first - 1) / first).clamp_(min=0.0).max(dim=2).values.reshape(-1)
    bound = float(torch.quantile(var, 0.9))
    out["abs_variance"] = bound
    out["render_adaptive_device"] = _time(lambda: camu.render_adaptive_device(world, first, first, sums.data_ptr(), sq.data_ptr(), counts.data_ptr(), abs_variance=bound,
                                                                              stream=s0), reps, warm, torch)
    out["adaptive_rays"] = rays()
    c = counts.to(torch.int64)
    out["adaptive_samples"] = int(c.sum())
    out["adaptive_count_histogram"] = {str(int(k)): int(v) for k, v in zip(*torch.unique(c, return_counts=True))}
    u, t, a = (out[k]["median_ms"] for k in ("uniform_render_device", "two_pass_loop", "render_adaptive_device"))
    out["two_pass_over_uniform"], out["adaptive_over_uniform"], out["adaptive_over_two_pass"] = t / u, a / u, a / t
    out["adaptive_samples_over_uniform"] = out["adaptive_samples"] / out["uniform_samples"]
    out["one_launch_beats_both"] = bool(a < u and a < t)


def step_rule(rl, name, reps, warm, spp, out):
    import numpy as np
    import torch
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name, spp)
    cam = rl.Camera(p)
    W, H = cam.c.image_width, cam.c.image_height
    S = p.samples_per_pixel
    out.update(width=W, height=H, samples_per_pixel=S, max_depth=p.max_depth, lib=os.environ.get("RL_RENDER_LIB", "product"))
    sums, sq = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    out["render_moments_device"] = _time(lambda: cam.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0), reps, warm, torch)
    rl.api.render_status(world, allow_degenerate=True)
    if hasattr(rl.api.render_lib(), "rl_rtiow_render_adaptive_device"):
        a_sums, a_sq = torch.zeros_like(sums), torch.zeros_like(sq)
        counts = torch.zeros((H, W), dtype=torch.int32, device="cuda:0")
        out["render_adaptive_device_no_checkpoint"] = _time(lambda: cam.render_adaptive_device(world, S, 1, a_sums.data_ptr(), a_sq.data_ptr(), counts.data_ptr(),
                                                                                                abs_variance=1.0, stream=s0), reps, warm, torch)
        rl.api.render_status(world, allow_degenerate=True)
        out["same_bits_as_moments"] = bool(torch.equal(sums, a_sums) and torch.equal(sq, a_sq) and bool((counts == S).all()))
        out["moments_again"] = _time(lambda: cam.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0), reps, 0, torch)  # drift of the session
        rl.api.render_status(world, allow_degenerate=True)


def regs(parent_lib):
    a, b = _regs(parent_lib), _regs(PRODUCT)
    plain = [k for k in a if "moments" not in k]
    diff = {k: {"parent": a[k], "branch": b.get(k)} for k in plain if a[k] != b.get(k)}
    return {"step": "regs", "kernel_names_without_moments": len(plain), "missing_from_branch": sorted(k for k in a if k not in b),
            "new_in_branch": sorted(k for k in b if k not in a), "kernels_without_moments": diff if diff else "no differences",
            "moments_kernels": {k: {"parent": a.get(k), "branch": v} for k, v in b.items() if "moments" in k}}


def step(what, reps, warm, spp):
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    kind, name = what.split(":")
    out = {"step": what}
    if kind == "loop":
        step_loop(rl, name, reps, warm, out)
    else:
        step_rule(rl, name, reps, warm, spp, out)
    print("RESULT " + json.dumps(out), flush=True)


def _child(what, a, lib=None):
    env = dict(os.environ)
    env.pop("RL_RENDER_LIB", None)
    if lib:
        env["RL_RENDER_LIB"] = lib
    cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps), "--warm", str(a.warm), "--spp", str(a.spp)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
    line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        print(f"step {what}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
        return None
    print(line[-1][7:], flush=True)
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--spp", type=int, default=1024, help="bouncing_spheres' samples per pixel in the rule step (the bench's)")
    ap.add_argument("--steps", default="loop:bouncing_spheres,loop:cornell_smoke,loop:cow_scene,rule:bouncing_spheres,rule:cornell_smoke,rule:cow_scene")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit: needed by the rule steps, adds regs and headline")
    ap.add_argument("--rule-rounds", type=int, default=2)
    ap.add_argument("--headline-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_adaptive.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.warm, a.spp)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    parent = os.path.abspath(a.parent_lib) if a.parent_lib else None

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")

    if parent:
        results["regs"] = regs(parent)
        print(json.dumps({"regs": results["regs"]["kernels_without_moments"]}), flush=True)
        save()
    for what in [w for w in a.steps.split(",") if w]:
        if what.startswith("loop:"):
            rec = _child(what, a)
            if rec is None:
                return 1
            results[what] = rec
        else:
            if not parent:
                print(f"step {what} needs --parent-lib", file=sys.stderr)
                return 1
            runs = {"parent": [], "branch": []}
            for _ in range(a.rule_rounds):
                for which in ("parent", "branch"):
                    rec = _child(what, a, parent if which == "parent" else None)
                    if rec is None:
                        return 1
                    runs[which].append(rec)
            pm = [r["render_moments_device"] for r in runs["parent"]]
            bm = sorted(r["render_moments_device"]["median_ms"] for r in runs["branch"])
            ba = sorted(r["render_adaptive_device_no_checkpoint"]["median_ms"] for r in runs["branch"])
            lo, hi = min(r["min_ms"] for r in pm), max(r["max_ms"] for r in pm)
            med = lambda v: (v[(len(v) - 1) // 2] + v[len(v) // 2]) / 2  # noqa: E731
            pmed = med(sorted(r["median_ms"] for r in pm))
            results[what] = {"step": what, "runs": runs, "parent_moments_min_max_ms": [lo, hi], "parent_moments_median_ms": pmed,
                             "branch_moments_median_ms": med(bm), "branch_adaptive_no_checkpoint_median_ms": med(ba),
                             "moments_branch_over_parent": med(bm) / pmed, "adaptive_no_checkpoint_over_parent_moments": med(ba) / pmed,
                             "branch_moments_within_parent_spread": bool(lo <= med(bm) <= hi),
                             "adaptive_no_checkpoint_within_parent_spread": bool(lo <= med(ba) <= hi),
                             "same_bits_as_moments": all(r["same_bits_as_moments"] for r in runs["branch"])}
        save()
    if parent and a.headline_rounds > 0:
        rec = headline(parent, a.headline_rounds)
        if rec is None:
            return 1
        results["headline"] = rec
        print(json.dumps(rec), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
