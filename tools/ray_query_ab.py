#!/usr/bin/env python3
"""Ray queries against the renders that trace the same rays: Mrays/s of hit_rays_device / color_at_rays_device on the pixel-centre rays
of a frame (device-resident buffers, HIP events on the launch stream, warm-up, --reps repetitions, median and spread), next to the
kernel_ms of render_device at samples_per_pixel = 1, max_depth = 1 (one ray per pixel plus RNG, get_ray and shading) and of the RTC
AA 1 render of the same frame.  The parent process never opens the GPU: every step runs in a child of its own under a time limit, and the
first failing step ends the run.  Results: profiles/ray_query.json (merged per step) and one JSON line per step on stdout.

usage: tools/ray_query_ab.py [--reps 20] [--steps bouncing,mirror[,cfg5]] [--out profiles/ray_query.json]        (GPU)
steps: bouncing = configs[1] bouncing_spheres 1920x1080; mirror = RTC mirror scene 1920x1080; cfg5 = the stress scene 3840x2160 (builds
a 1 M sphere world on the host first: minutes; not in the default list)."""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMITS = {"bouncing": 300, "mirror": 300, "cfg5": 1100}


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


def _rtc_camera_rays(np, cam):  # rays_for_pixel (scene/camera.rs:63-91), one sample per pixel, in the device's order of operations
    inv = np.array(list(cam.inverse)).reshape(4, 4)
    px, py = np.meshgrid(np.arange(cam.hsize, dtype=np.float64), np.arange(cam.vsize, dtype=np.float64))
    x = cam.half_width - (px.reshape(-1) + 0.5) * cam.pixel_size
    y = cam.half_height - (py.reshape(-1) + 0.5) * cam.pixel_size

    def mul_point(vx, vy, vz):
        return [((0.0 + inv[r, 0] * vx) + inv[r, 1] * vy) + inv[r, 2] * vz + inv[r, 3] * 1.0 for r in range(3)]
    pix, org = mul_point(x, y, np.full_like(x, -1.0)), mul_point(np.zeros_like(x), np.zeros_like(x), np.zeros_like(x))
    v = [pix[k] - org[k] for k in range(3)]
    m = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return np.stack(org, axis=1), np.stack([v[0] / m, v[1] / m, v[2] / m], axis=1)


def step(name, reps):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    api = rl.api
    rl.init(0)
    s0 = torch.cuda.current_stream().cuda_stream
    out = {"step": name}
    if name in ("bouncing", "cfg5"):
        if name == "bouncing":
            world = rl.World.bouncing_spheres(1)
            p = world.params
            p.aspect_ratio, p.image_width = 16.0 / 9.0, 1920
        else:
            from PIL import Image
            import gzip
            G = os.path.join(ROOT, "tests", "golden")
            tex = np.asarray(Image.open(os.path.join(G, "spot_texture.png")).convert("RGB"))
            world = rl.World.stress_scene(1000, 2, gzip.open(os.path.join(G, "spot_triangulated.obj.gz"), "rb").read(), tex)
            p = world.params
            p.aspect_ratio, p.image_width = 16.0 / 9.0, 3840
        p.samples_per_pixel, p.max_depth = 1, 1
        cam = rl.Camera(p)
        o, d = _pixel_centre_rays(np, cam)
        n = o.shape[0]
        rays = api.pack_rays(o, d)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 56).copy()).to("cuda:0")
        d_hits = torch.zeros((n, 88), dtype=torch.uint8, device="cuda:0")
        frame = torch.zeros((cam.c.image_height, cam.c.image_width, 3), dtype=torch.float64, device="cuda:0")
        q = _time(lambda: world.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s0), reps, torch)
        served = api.last_query()["kernel"]
        api.render_status(world)
        world.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s0)
        retraced = api.render_status(world)["slow_traces"]
        api.set_fast_traversal(False)  # the same call through the reference-order kernel
        qr = _time(lambda: world.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s0), reps, torch)
        api.set_fast_traversal(True)
        api.render_status(world)
        r = _time(lambda: cam.render_device(world, frame.data_ptr(), stream=s0), reps, torch)
        api.render_status(world)
        st = {}
        world.hit_rays_device(d_rays.data_ptr(), d_hits.data_ptr(), n, stream=s0, stats=st)
        out.update(rays=n, width=cam.c.image_width, height=cam.c.image_height, hit_rays_device=q, render_device_1spp_depth1=r,
                   hit_rays_mrays_per_s=n / q["median_ms"] / 1e3, ratio_query_over_render=q["median_ms"] / r["median_ms"],
                   hit_rays_counting_kernel_ms=st["kernel_ms"], served_by=served, retraced=int(retraced), hit_rays_device_reference_order=qr,
                   ratio_reference_order_over_render=qr["median_ms"] / r["median_ms"])
    else:
        world = rl.RtcWorld.test_mirror_scene(1920, 1080)
        cam = world.camera
        o, d = _rtc_camera_rays(np, cam)
        n = o.shape[0]
        rays = api.pack_rays(o, d)
        d_rays = torch.from_numpy(rays.view(np.uint8).reshape(n, 56).copy()).to("cuda:0")
        d_rgb = torch.zeros((n, 3), dtype=torch.float64, device="cuda:0")
        frame = torch.zeros((cam.vsize, cam.hsize, 3), dtype=torch.float64, device="cuda:0")
        q = _time(lambda: world.color_at_rays_device(d_rays.data_ptr(), d_rgb.data_ptr(), n, stream=s0), reps, torch)
        api.render_status(world)
        r = _time(lambda: world.render_device(frame.data_ptr(), 1, stream=s0), reps, torch)
        api.render_status(world)
        out.update(rays=n, width=cam.hsize, height=cam.vsize, color_at_rays_device=q, rtc_render_device_aa1=r,
                   ratio_query_over_render=q["median_ms"] / r["median_ms"], same_bits=bool(torch.equal(d_rgb.reshape(frame.shape), frame)))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="bouncing,mirror")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ray_query.json"))
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
