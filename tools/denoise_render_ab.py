#!/usr/bin/env python3
"""denoise_render on the device (rl_denoise_prepare_device, rl_denoise_finish_device, rl_denoise_render_device): what the
two elementwise kernels cost beside a copy of the bytes they must move, what the whole chain costs beside the sum of its parts, and what the
host path it replaces costs.

  kernels   1920x1080, G = 8, an adaptive estimate and features of seeded random sums resident on the device.  prepare reads 13 doubles and
            two words and writes 14 doubles per pixel; finish reads 9 doubles and writes 6 doubles and 3 bytes (also timed without the
            bytes, which cost one binary64 pow per value).  In the same run a
            device-to-device copy that moves the same bytes (a copy of n bytes reads n and writes n, so it is of half the kernel's
            traffic).  copy / kernel is the fraction of the achievable bandwidth the kernel reaches.
  whole     rl_denoise_render_device with five passes and all three outputs, beside prepare + the five passes + finish timed one by one
  host      api.denoise_render (numpy around the staged filter) on the same frame brought to the host: wall clock, staging included; and
            api.denoise_render_gpu (rl_denoise_render: staging, the chain, three copies back), whose bytes are asserted to be the same

HIP events on the launch stream, --warm warm-ups and --reps timed repetitions (kernels and copies: ten calls per repetition), median
[min, max].  The parent process never opens the GPU: every step runs in a child of its own under `timeout -k 10`, and the first failing
step ends the run.  Results: profiles/denoise_render.json (merged per step) and one JSON line per step on stdout.

usage: tools/denoise_render_ab.py [--reps 20] [--warm 3] [--steps kernels,whole,host] [--out FILE]"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from render_moments_ab import LIMIT_S, _stats, _time  # noqa: E402  (the same timing)

W, H, G = 1920, 1080, 8
ITERATIONS = 5
INNER = 10
FEATURE_SAMPLES = 4


def _frame(rl, torch):
    """Seeded random sums as the renders leave them: counts 2 .. 9, sq >= sums^2 / n -> (tensors by name, the DenoiseInputs over them)."""
    dev = "cuda:0"
    gen = torch.Generator(device=dev).manual_seed(1)
    rand = lambda *shape: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen)
    counts = torch.randint(2, 10, (H, W), dtype=torch.int32, device=dev, generator=gen)
    n = counts.to(torch.float64)[..., None]
    sums = rand(H, W, 3) * 2.0 * n
    t = {"sums": sums, "sq": sums * sums / n * (1.0 + 0.5 * rand(H, W, 3)), "counts": counts, "albedo_sum": rand(H, W, 3) * 3.6 + 0.4,
         "normal_sum": rand(H, W, 3) * 2.0 - 1.0, "depth_sum": rand(H, W) * 8.0 + 1.0,
         "hit_count": torch.randint(0, FEATURE_SAMPLES + 1, (H, W), dtype=torch.int32, device=dev, generator=gen)}
    d = rl.api.denoise_inputs({k: v.data_ptr() for k, v in t.items()}, feature_samples=FEATURE_SAMPLES)
    return t, d


def _timed(torch, fn):  # INNER back-to-back calls between two events: a single kernel is too short a window
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(INNER):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / INNER


def step_kernels(rl, reps, warm, out):
    import torch
    api = rl.api
    dev = "cuda:0"
    t, d = _frame(rl, torch)
    s0 = torch.cuda.current_stream().cuda_stream
    npix = W * H
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    color, variance, guides, out_c, out_v = f64(H, W, 3), f64(H, W, 3), f64(H, W, G), f64(H, W, 3), f64(H, W, 3)
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    traffic = {"prepare": npix * (13 * 8 + 2 * 4 + 14 * 8), "finish": npix * (9 * 8 + 6 * 8 + 3), "finish_without_rgb8": npix * (9 * 8 + 6 * 8)}
    kernels = {"prepare": lambda: api.denoise_prepare_device(W, H, d, color.data_ptr(), variance.data_ptr(), guides.data_ptr(), stream=s0),
               "finish": lambda: api.denoise_finish_device(W, H, color.data_ptr(), variance.data_ptr(), t["albedo_sum"].data_ptr(), FEATURE_SAMPLES, out_c.data_ptr(),
                                                           out_v.data_ptr(), u8.data_ptr(), stream=s0),
               "finish_without_rgb8": lambda: api.denoise_finish_device(W, H, color.data_ptr(), variance.data_ptr(), t["albedo_sum"].data_ptr(), FEATURE_SAMPLES,
                                                                        out_c.data_ptr(), out_v.data_ptr(), stream=s0)}
    out.update(width=W, height=H, n_guides=G, calls_per_timed_window=INNER)
    for name, fn in kernels.items():
        src = torch.empty(traffic[name] // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        copy = lambda: dst.copy_(src)
        for _ in range(warm):
            fn(), copy()
        torch.cuda.synchronize()
        ms = {"kernel": [], "copy": []}
        for _ in range(reps):  # the two alternate repetition by repetition
            ms["kernel"].append(_timed(torch, fn))
            ms["copy"].append(_timed(torch, copy))
        rec = {k: _stats(v) for k, v in ms.items()}
        rec["bytes_moved"] = traffic[name]
        rec["kernel_GBps"] = traffic[name] / rec["kernel"]["median_ms"] / 1e6
        rec["copy_GBps"] = traffic[name] / rec["copy"]["median_ms"] / 1e6
        rec["copy_over_kernel"] = rec["copy"]["median_ms"] / rec["kernel"]["median_ms"]
        out[name] = rec


def step_whole(rl, reps, warm, out):
    import torch
    api = rl.api
    dev = "cuda:0"
    t, d = _frame(rl, torch)
    s0 = torch.cuda.current_stream().cuda_stream
    p = api.atrous_params(G, guide_sigma=[0.1] * 3 + [0.25] * 3 + [1.0, 0.25])
    work_bytes = api.denoise_render_work_bytes(W, H, G)
    work = torch.empty(work_bytes // 8, dtype=torch.float64, device=dev)
    image = W * H * 3
    pairs = [(work[0:image], work[image:2 * image]), (work[2 * image:3 * image], work[3 * image:4 * image])]
    guides = work[4 * image:]
    out_c, out_v = (torch.empty((H, W, 3), dtype=torch.float64, device=dev) for _ in range(2))
    u8 = torch.empty((H, W, 3), dtype=torch.uint8, device=dev)
    out.update(width=W, height=H, n_guides=G, iterations=ITERATIONS, work_bytes=work_bytes)
    whole = lambda: api.denoise_render_device(W, H, d, ITERATIONS, p, work.data_ptr(), work_bytes, out_c.data_ptr(), out_v.data_ptr(), u8.data_ptr(), stream=s0)
    out["render_device"] = _time(whole, reps, warm, torch)
    parts = {"prepare": lambda: api.denoise_prepare_device(W, H, d, pairs[0][0].data_ptr(), pairs[0][1].data_ptr(), guides.data_ptr(), stream=s0)}
    for it in range(ITERATIONS):
        src, dst = pairs[it & 1], pairs[(it + 1) & 1]
        parts[f"pass_step_{1 << it}"] = (lambda src=src, dst=dst, it=it: api.denoise_atrous_pass_device(
            W, H, 1 << it, p, src[0].data_ptr(), src[1].data_ptr(), guides.data_ptr(), dst[0].data_ptr(), dst[1].data_ptr(), stream=s0))
    last = pairs[ITERATIONS & 1]
    parts["finish"] = lambda: api.denoise_finish_device(W, H, last[0].data_ptr(), last[1].data_ptr(), t["albedo_sum"].data_ptr(), FEATURE_SAMPLES, out_c.data_ptr(),
                                                        out_v.data_ptr(), u8.data_ptr(), stream=s0)
    out["parts"] = {name: _time(fn, reps, warm, torch) for name, fn in parts.items()}  # in the chain's order, so each reads what the one before wrote
    out["sum_of_parts_median_ms"] = sum(r["median_ms"] for r in out["parts"].values())
    out["whole_over_sum_of_parts"] = out["render_device"]["median_ms"] / out["sum_of_parts_median_ms"]


def step_host(rl, reps, out):
    import numpy as np
    import torch
    api = rl.api
    t, _ = _frame(rl, torch)
    h = {k: v.cpu().numpy() for k, v in t.items()}
    est = api.Adaptive(h["sums"], h["sq"], h["counts"].view(np.uint32))
    feats = api.Features(FEATURE_SAMPLES, albedo_sum=h["albedo_sum"], normal_sum=h["normal_sum"], depth_sum=h["depth_sum"], hit_count=h["hit_count"].view(np.uint32))
    reps = max(3, reps // 4)

    def wall(fn):
        ms = []
        for _ in range(reps):
            t0 = time.perf_counter()
            res = fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return res, _stats(ms)
    (hc, hv), out["denoise_render_host_path_wall"] = wall(lambda: api.denoise_render(est, feats))
    (gc, gv), out["denoise_render_gpu_wall"] = wall(lambda: api.denoise_render_gpu(est, feats))
    assert hc.tobytes() == gc.tobytes() and hv.tobytes() == gv.tobytes(), "the two paths differ"
    out.update(width=W, height=H, same_bytes=True, host_over_gpu=out["denoise_render_host_path_wall"]["median_ms"] / out["denoise_render_gpu_wall"]["median_ms"])


def step(what, reps, warm):
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    out = {}
    if what == "kernels":
        step_kernels(rl, reps, warm, out)
    elif what == "whole":
        step_whole(rl, reps, warm, out)
    elif what == "host":
        step_host(rl, reps, out)
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
    ap.add_argument("--steps", default="kernels,whole,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_render.json"))
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
