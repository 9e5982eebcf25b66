#!/usr/bin/env python3
"""Renders with second moments (rl_rtiow_render_moments_device / rl_rtiow_render_pixels_moments_device): what the flavour
costs, and a worked adaptive pass.

  cost      render_device next to render_moments_device, same process, same buffers' sizes, alternating warm-ups: bouncing_spheres at
            1920x1080 at the bench's sample count (--spp), cornell_smoke at 600x600 at the scene's own samples, cow_scene at 1920x1080 at
            32 spp; the moments call's sums are checked against the plain frame (same bits)
  adaptive  bouncing_spheres at 1920x1080: render_moments_device at 16 spp; the tenth of the pixels with the largest variance_of_mean
            (summed over the channels); render_pixels_moments_device for 64 further samples of those at first_sample = 16; the merge —
            timed as a whole (device-side selection included) next to a uniform 80 spp render_device
  regs      (CPU only) tools/kernel_regs.py on --parent-lib and on the product library: the figures of every kernel name both have
            ("no differences" or the list), and the MOMENTS instantiations' own figures
  headline  `bench.py --gpus 1 --steps 5 --warmup 2 --configs ""` on --parent-lib and on the product library, alternating, three runs each

Device-resident buffers, HIP events on the launch stream, --warm warm-ups and --reps timed repetitions, median [min, max].  The parent
process never opens the GPU: every GPU step runs in a child of its own under `timeout -k 10`, and the first failing step ends the run.
Results: profiles/render_moments.json (merged per step) and one JSON line per step on stdout.

usage: tools/render_moments_ab.py [--reps 5] [--warm 1] [--spp 1024] [--steps cost:bouncing_spheres,cost:cornell_smoke,cost:cow_scene,adaptive:bouncing_spheres]
                                  [--parent-lib FILE (adds regs and headline)] [--out FILE]"""
import argparse
import gzip
import importlib
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 420


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


def _world(rl, np, name, spp):
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
    if name == "cornell_smoke":
        p.aspect_ratio, p.image_width = 1.0, 600
    else:
        p.aspect_ratio, p.image_width = 16.0 / 9.0, 1920
        p.samples_per_pixel = 32 if name == "cow_scene" else spp
    return w, p


def step_cost(rl, name, reps, warm, spp, out):
    import numpy as np
    import torch
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name, spp)
    cam = rl.Camera(p)
    W, H = cam.c.image_width, cam.c.image_height
    out.update(width=W, height=H, samples_per_pixel=p.samples_per_pixel, max_depth=p.max_depth)
    plain = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    sums, sq = torch.zeros_like(plain), torch.zeros_like(plain)
    out["render_device"] = _time(lambda: cam.render_device(world, plain.data_ptr(), stream=s0), reps, warm, torch)
    out["rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
    out["render_moments_device"] = _time(lambda: cam.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0), reps, warm, torch)
    out["moments_rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
    out["plain_again"] = _time(lambda: cam.render_device(world, plain.data_ptr(), stream=s0), reps, 0, torch)  # drift of the session
    api.render_status(world, allow_degenerate=True)
    out["sums_same_bits"] = bool(torch.equal(plain, sums))
    out["moments_over_plain"] = out["render_moments_device"]["median_ms"] / out["render_device"]["median_ms"]


def step_adaptive(rl, name, reps, warm, out):
    import dataclasses
    import numpy as np
    import torch
    api = rl.api
    s0 = torch.cuda.current_stream().cuda_stream
    world, p = _world(rl, np, name, 16)
    first, more = 16, 64
    cam1 = rl.Camera(dataclasses.replace(p, samples_per_pixel=first))
    cam2 = rl.Camera(dataclasses.replace(p, samples_per_pixel=more))
    camu = rl.Camera(dataclasses.replace(p, samples_per_pixel=first + more))
    W, H = cam1.c.image_width, cam1.c.image_height
    n = (W * H) // 10
    out.update(width=W, height=H, first_pass_spp=first, second_pass_spp=more, second_pass_pixels=n, uniform_spp=first + more, max_depth=p.max_depth)
    sums, sq = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    lsums, lsq = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0"), torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
    uniform = torch.zeros((H, W, 3), dtype=torch.float64, device="cuda:0")
    parts = {}

    def timed(key, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        parts.setdefault(key, []).append((e0, e1))
        return r

    def select():  # Moments.variance_of_mean on the device, summed over the channels; the n largest
        v = ((sq - sums * sums / first) / (first - 1) / first).clamp_(min=0.0).sum(dim=2).reshape(-1)
        idx = torch.topk(v, n).indices
        return (idx % W).to(torch.int32), (idx // W).to(torch.int32), idx

    def merge(idx):
        sums.reshape(-1, 3).index_add_(0, idx, lsums)
        sq.reshape(-1, 3).index_add_(0, idx, lsq)

    def loop():
        timed("first_pass", lambda: cam1.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=s0))
        d_xs, d_ys, idx = timed("select", select)
        timed("second_pass", lambda: cam2.render_pixels_moments_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, lsums.data_ptr(), lsq.data_ptr(), stream=s0,
                                                                       first_sample=first))
        timed("merge", lambda: merge(idx))

    out["adaptive_loop"] = _time(loop, reps, warm, torch)
    api.render_status(world, allow_degenerate=True)
    torch.cuda.synchronize()
    for key, evs in parts.items():
        out[key] = _stats([a.elapsed_time(b) for a, b in evs[warm:]])
    out["uniform_render_device"] = _time(lambda: camu.render_device(world, uniform.data_ptr(), stream=s0), reps, warm, torch)
    out["uniform_rays"] = int(api.render_status(world, allow_degenerate=True)["rays"])
    # (the refined pixels are NOT the uniform render's: their second pass starts a fresh chain at sample 16, word position 0)
    out["adaptive_over_uniform"] = out["adaptive_loop"]["median_ms"] / out["uniform_render_device"]["median_ms"]


def _regs(lib):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), lib], stdout=subprocess.PIPE, text=True, check=True)
    rows = {}
    for line in r.stdout.splitlines()[1:]:
        f = line.split(None, 7)
        rows.setdefault(f[7] if len(f) > 7 else "", []).append(dict(zip(("vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_bytes", "lds_bytes"), map(int, f[:7]))))
    return {k: sorted(v, key=lambda d: sorted(d.items())) for k, v in rows.items()}  # (names are cut at 110 characters: a name may stand for several kernels)


def regs(parent_lib):
    a, b = _regs(parent_lib), _regs(os.path.join(ROOT, "rendering-learning_amd", "csrc", "librl_render.so"))
    diff = {k: {"parent": a[k], "branch": b[k]} for k in a if k in b and a[k] != b[k]}
    return {"step": "regs", "kernel_names_in_both": len([k for k in a if k in b]), "missing_from_branch": sorted(k for k in a if k not in b),
            "existing_kernels": diff if diff else "no differences",
            "moments_instantiations": {k: v[0] for k, v in b.items() if re.search(r"moments_kernel", k)}}


def headline(parent_lib, rounds):
    """bench.py on the parent's library and on the product library, alternating; every run a child process under its own time limit."""
    runs = {"parent": [], "branch": []}
    for _ in range(rounds):
        for which in ("parent", "branch"):
            env = dict(os.environ)
            env.pop("RL_RENDER_LIB", None)
            if which == "parent":
                env["RL_RENDER_LIB"] = parent_lib
            cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--configs", ""]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, env=env)
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                print(f"headline ({which}): exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
                return None
            d = json.loads(line[-1])
            runs[which].append({"Mrays_s": d["value"], "ms_per_step": d["ms_per_step"], "check": d.get("check", {}).get("timed_frame_equals_counting_frame")})
            print(json.dumps({which: runs[which][-1]}), flush=True)
    rec = {"step": "headline", "cmd": 'bench.py --gpus 1 --steps 5 --warmup 2 --configs ""', "runs": runs}
    pv, bv = sorted(x["Mrays_s"] for x in runs["parent"]), sorted(x["Mrays_s"] for x in runs["branch"])
    rec["parent_min_max_Mrays_s"], rec["branch_median_Mrays_s"] = [pv[0], pv[-1]], bv[len(bv) // 2]
    rec["branch_median_within_parent_spread"] = bool(pv[0] <= rec["branch_median_Mrays_s"] <= pv[-1])
    return rec


def step(what, reps, warm, spp):
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    kind, name = what.split(":")
    out = {"step": what}
    if kind == "cost":
        step_cost(rl, name, reps, warm, spp, out)
    else:
        step_adaptive(rl, name, reps, warm, out)
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm", type=int, default=1)
    ap.add_argument("--spp", type=int, default=1024, help="bouncing_spheres' samples per pixel in the cost step (the bench's)")
    ap.add_argument("--steps", default="cost:bouncing_spheres,cost:cornell_smoke,cost:cow_scene,adaptive:bouncing_spheres")
    ap.add_argument("--parent-lib", default=None, help="a build of the parent commit: adds the regs and headline steps")
    ap.add_argument("--headline-rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_moments.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.warm, a.spp)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1, sort_keys=True)
            f.write("\n")

    if a.parent_lib:
        results["regs"] = regs(os.path.abspath(a.parent_lib))
        print(json.dumps({"regs": results["regs"]["existing_kernels"]}), flush=True)
        save()
    for what in [w for w in a.steps.split(",") if w]:
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", what, "--reps", str(a.reps), "--warm", str(a.warm),
               "--spp", str(a.spp)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if r.returncode != 0 or not line:
            print(f"step {what}: exit status {r.returncode}; stopping\n{r.stdout[-2000:]}", file=sys.stderr)
            return 1
        results[what] = json.loads(line[-1][7:])
        print(line[-1][7:], flush=True)
        save()
    if a.parent_lib and a.headline_rounds > 0:
        rec = headline(os.path.abspath(a.parent_lib), a.headline_rounds)
        if rec is None:
            return 1
        results["headline"] = rec
        print(json.dumps(rec), flush=True)
        save()
    return 0


if __name__ == "__main__":
    sys.exit(main())
