#!/usr/bin/env python3
"""The direct-lighting render next to the ambient-occlusion render on the same 1920x1080 frame: ms of render_direct_device with L lights x K
points against render_ao_device with ao_rays = L * K and radius = inf.  Both trace one first hit per sample and send the same number of
any-hit rays from every hit (the direct render skips the light points that face away, the AO render none), so the ratio says what the
light arithmetic, the two floating-point folds and the bounded segments cost or save next to open cosine-weighted rays.  It is a ratio
between two different renders, reported, not a gate.  S = 4; cornell_box: its own light, K = 4; bouncing_spheres and the reduced stress
scene: two lights above the scene, K = 2.  HIP events on the launch stream, 3 warm-up + --reps timed repetitions, median [min, max].  The
counter-free render is also compared byte for byte with the counting one in the same run.
The parent process never opens the GPU: every step runs in a child of its own under a time limit, and the first failing step ends the
run.  Results: profiles/render_direct.json (merged per step) and one JSON line per step on stdout.

usage: tools/render_direct_ab.py [--reps 20] [--steps cornell,bouncing,stress60] [--width 1920] [--out profiles/render_direct.json]        (GPU)
steps: cornell = cornell_box; bouncing = bouncing_spheres(1); stress60 = stress_scene(60, 1): 3,600 spheres and the cow mesh subdivided once."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"cornell": 300, "bouncing": 300, "stress60": 300}
S = 4
ABOVE = [((-6.0, 20.0, -6.0), (12.0, 0.0, 0.0), (0.0, 0.0, 12.0), (4.0, 4.0, 4.0)), ((14.0, 6.0, -4.0), (0.0, 0.0, 8.0), (2.0, 3.0, 0.0), (3.0, 2.0, 1.0))]
SETUPS = {"cornell": ([((343.0, 554.0, 332.0), (-130.0, 0.0, 0.0), (0.0, 0.0, -105.0), 15.0)], 4), "bouncing": (ABOVE, 2), "stress60": (ABOVE, 2)}


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


def step(name, reps, width):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    rl.init(0)
    api = rl.api
    if name == "cornell":
        world = rl.World.example_scene("cornell_box")
    elif name == "bouncing":
        world = rl.World.bouncing_spheres(1)
    else:
        from PIL import Image
        import gzip
        G = os.path.join(ROOT, "tests", "golden")
        tex = np.asarray(Image.open(os.path.join(G, "spot_texture.png")).convert("RGB"))
        world = rl.World.stress_scene(60, 1, gzip.open(os.path.join(G, "spot_triangulated.obj.gz"), "rb").read(), tex)
    lights, K = SETUPS[name]
    L = len(lights)
    p = world.params
    p.aspect_ratio, p.image_width, p.samples_per_pixel = 16.0 / 9.0, width, S
    cam = rl.Camera(p)
    n = cam.c.image_width * cam.c.image_height
    s0 = torch.cuda.current_stream().cuda_stream
    dev = "cuda:0"
    d_di, d_un = torch.zeros(n * 3, dtype=torch.float64, device=dev), torch.zeros(n * 3, dtype=torch.float64, device=dev)
    d_hc, a_open, a_hits = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(3))
    direct = lambda: rl.render_direct_device(cam, world, lights, K, stream=s0, d_direct=d_di.data_ptr(), d_unshadowed=d_un.data_ptr(), d_hits=d_hc.data_ptr())
    ao = lambda: rl.render_ao_device(cam, world, L * K, float("inf"), stream=s0, d_open=a_open.data_ptr(), d_hits=a_hits.data_ptr())
    out = {"step": name, "width": cam.c.image_width, "height": cam.c.image_height, "pixels": n, "samples": S, "lights": L, "light_samples": K,
           "seg_tmax": rl.direct.SEG_TMAX, "render_lib": os.path.basename(api.RENDER_LIB)}
    for label, fn in (("render_direct_device", direct), ("render_ao_device", ao)):
        row = _time(fn, reps, torch)
        row["served_by"] = api.last_query()["kernel"]
        api.render_status(world, allow_degenerate=True)
        fn()
        torch.cuda.synchronize()
        st = api.render_status(world, allow_degenerate=True)
        row["retraced"], row["rays"] = int(st["slow_traces"]), int(st["rays"])
        out[label] = row
    out["hits"] = int(d_hc.sum().item())
    out["segments_traced"] = out["render_direct_device"]["rays"] - S * n
    out["ambient_rays"] = out["render_ao_device"]["rays"] - S * n
    out["same_hits_as_ao"] = bool(torch.equal(d_hc, a_hits))
    # the counter-free render against the counting one (the reference-order fold for every ray), byte for byte
    fast_di, fast_un = d_di.clone(), d_un.clone()
    rl.render_direct_device(cam, world, lights, K, stream=s0, d_direct=d_di.data_ptr(), d_unshadowed=d_un.data_ptr(), d_hits=d_hc.data_ptr(), stats={},
                            allow_degenerate=True)
    out["same_bytes_as_counting"] = bool(torch.equal(fast_di.view(torch.int64), d_di.view(torch.int64)) and torch.equal(fast_un.view(torch.int64), d_un.view(torch.int64)))
    out["ratio_direct_over_ao"] = out["render_direct_device"]["median_ms"] / out["render_ao_device"]["median_ms"]
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="cornell,bouncing,stress60")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_direct.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.width)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for name in a.steps.split(","):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--width", str(a.width)], stdout=subprocess.PIPE,
                               text=True, timeout=LIMITS[name])
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
