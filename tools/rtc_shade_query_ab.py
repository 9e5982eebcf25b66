#!/usr/bin/env python3
"""RTC shading queries, measured.  Per scene, on the 1920x1080 frame's pixel-centre rays (one per pixel):

  traversal  prepare_rays_device next to intersect_rays_device(k = 0) with the hit index on the same rays: the same traversal plus the
             208-byte record, so the ratio is the record's cost.
  split      prepare_rays_device + shade_hits_device next to color_at_rays_device (on the teapot scene there are no secondary rays, so
             the two do the same work).
  lighting   lighting_device next to a device-to-device copy that moves the same bytes per element (208 + 24 + 24 + 8 read, 24 written:
             a copy of 144 B per element reads and writes 288 B).
  compose    (mirror only) the loop of include/rl_render.h composed on device buffers, bounce-synchronous, torch compaction between the
             levels, next to color_at_rays_device; the colours are compared (the sum order differs from the render's depth-first order, so
             the comparison is a tolerance, not bytes: tests/test_gpu_rtc_shade_query.py pins the bytes).
  color      color_at_rays_device alone — the step an older library (RL_RENDER_LIB = a build of the parent commit) can run too.

Device-resident buffers, HIP events on the launch stream, 3 warm-up and --reps timed repetitions, median [min, max].  The parent process
never opens the GPU: every step runs in a child of its own under `timeout -k 10`, and the first failing step ends the run.
Results: profiles/rtc_shade_query.json (merged per step) and one JSON line per step on stdout.

usage: tools/rtc_shade_query_ab.py [--reps 20] [--steps mirror,csg,teapot] [--only all|color] [--out FILE]   (GPU)"""
import argparse
import importlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_S = 300
W, H = 1920, 1080


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


def _camera_rays(np, cam):
    """rays_for_pixel (scene/camera.rs:63-91) at the pixel centres, in the device's order of operations."""
    inv = np.array(list(cam.inverse)).reshape(4, 4)
    px, py = np.meshgrid(np.arange(cam.hsize, dtype=np.float64), np.arange(cam.vsize, dtype=np.float64))
    px, py = px.reshape(-1), py.reshape(-1)
    x = cam.half_width - (px + 0.5) * cam.pixel_size
    y = cam.half_height - (py + 0.5) * cam.pixel_size
    z = np.full_like(x, -1.0)
    pix = [((0.0 + inv[r, 0] * x) + inv[r, 1] * y) + inv[r, 2] * z + inv[r, 3] * 1.0 for r in range(3)]
    org = [np.full_like(x, ((0.0 + inv[r, 0] * 0.0) + inv[r, 1] * 0.0) + inv[r, 2] * 0.0 + inv[r, 3] * 1.0) for r in range(3)]
    v = [pix[k] - org[k] for k in range(3)]
    m = np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    return np.stack(org, axis=1), np.stack([v[0] / m, v[1] / m, v[2] / m], axis=1)


def step(name, reps, only):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    rl = importlib.import_module("rendering-learning_amd")
    api = rl.api
    rl.init(0)
    dev = "cuda:0"
    s0 = torch.cuda.current_stream().cuda_stream
    if name == "teapot":
        world = rl.RtcWorld.test_obj_scene(open(os.path.join(ROOT, "tests", "golden", "teapot-low.obj"), "rb").read(), W, H)
    else:
        world = rl.RtcWorld.test_mirror_scene(W, H) if name == "mirror" else rl.RtcWorld.test_csg_scene(W, H)
    o, d = _camera_rays(np, world.camera)
    n = o.shape[0]
    d_rays = torch.from_numpy(api.pack_rays(o, d).view(np.float64).reshape(n, 7).copy()).to(dev)
    d_rgb = torch.zeros((n, 3), dtype=torch.float64, device=dev)
    out = {"step": name, "library": os.environ.get("RL_RENDER_LIB", "product"), "rays": n, "width": W, "height": H}

    def color():
        world.color_at_rays_device(d_rays.data_ptr(), d_rgb.data_ptr(), n, stream=s0)
    out["color_at_rays_device"] = _time(color, reps, torch)
    out["color_rays"] = int(api.render_status(world)["rays"])
    if only == "all":
        lights, mats = world.lights(), world.materials()
        nl = len(lights)
        d_cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        d_hi = torch.zeros(n, dtype=torch.int32, device=dev)
        d_comps = torch.zeros((n, 26), dtype=torch.float64, device=dev)
        d_shade = torch.zeros((n, 19), dtype=torch.float64, device=dev)
        isect = _time(lambda: world.intersect_rays_device(d_rays.data_ptr(), n, 0, 0, d_cnt.data_ptr(), d_hi.data_ptr(), stream=s0), reps, torch)
        api.render_status(world)
        prep = _time(lambda: world.prepare_rays_device(d_rays.data_ptr(), n, d_comps.data_ptr(), stream=s0), reps, torch)
        api.render_status(world)
        out["traversal"] = {"intersect_rays_device_k0": isect, "prepare_rays_device": prep, "ratio_prepare_over_intersect": prep["median_ms"] / isect["median_ms"]}
        shade = _time(lambda: world.shade_hits_device(d_comps.data_ptr(), n, d_shade.data_ptr(), stream=s0), reps, torch)
        api.render_status(world)
        both = prep["median_ms"] + shade["median_ms"]
        out["split"] = {"shade_hits_device": shade, "prepare_plus_shade_ms": both, "ratio_split_over_color_at": both / out["color_at_rays_device"]["median_ms"]}
        d_lp = torch.from_numpy(np.tile(lights["position"][0], (n, 1))).to(dev)
        d_li = torch.from_numpy(np.tile(lights["intensity"][0], (n, 1))).to(dev)
        d_att = torch.ones(n, dtype=torch.float64, device=dev)
        d_lrgb = torch.zeros((n, 3), dtype=torch.float64, device=dev)
        src = torch.zeros((n, 18), dtype=torch.float64, device=dev)  # 144 B per element
        dst = torch.zeros_like(src)
        lt = _time(lambda: world.lighting_device(d_comps.data_ptr(), d_lp.data_ptr(), d_li.data_ptr(), d_att.data_ptr(), n, d_lrgb.data_ptr(), stream=s0),
                   reps, torch)
        api.render_status(world)
        cp = _time(lambda: dst.copy_(src), reps, torch)
        out["lighting"] = {"lighting_device": lt, "copy_144B_per_element": cp, "ratio_lighting_over_copy": lt["median_ms"] / cp["median_ms"],
                           "gb_per_s": n * 288 / lt["median_ms"] / 1e6, "copy_gb_per_s": n * 288 / cp["median_ms"] / 1e6}
        if name == "mirror":
            desc = api.RtcSceneDesc.from_address(world.desc)
            void = torch.tensor(list(desc.void_color), dtype=torch.float64, device=dev)
            t_refl = torch.from_numpy(mats["reflectivity"].copy()).to(dev)
            t_tran = torch.from_numpy(mats["transparency"].copy()).to(dev)
            total = torch.zeros((n, 3), dtype=torch.float64, device=dev)

            def compose():
                total.zero_()
                root, r, w = torch.arange(n, device=dev), d_rays, torch.ones(n, dtype=torch.float64, device=dev)
                remaining = int(desc.max_reflection_depth)
                while int(root.shape[0]):
                    k = int(root.shape[0])
                    c = torch.empty((k, 26), dtype=torch.float64, device=dev)
                    world.prepare_rays_device(r.data_ptr(), k, c.data_ptr(), stream=s0)
                    ci = c.view(torch.int64)
                    hit = ((ci[:, 24] & 0xFFFFFFFF) != 0) & (nl != 0)
                    total.index_add_(0, root[~hit], w[~hit, None] * void)
                    root, w, c = root[hit], w[hit], c[hit].contiguous()
                    k = int(root.shape[0])
                    if k == 0:
                        break
                    s = torch.empty((k, 19), dtype=torch.float64, device=dev)
                    world.shade_hits_device(c.data_ptr(), k, s.data_ptr(), stream=s0)
                    total.index_add_(0, root, w[:, None] * s[:, 0:3])
                    if remaining == 0:
                        break
                    mat = (c.view(torch.int64)[:, 25] >> 32) & 0xFFFFFFFF
                    fl = s.view(torch.int64)[:, 18]
                    refl, refr = (fl & 0xFFFFFFFF) != 0, ((fl >> 32) & 0xFFFFFFFF) != 0
                    mr, mt = t_refl[mat], t_tran[mat]
                    wl = w * float(nl)
                    bothm = (mr > 0) & (mt > 0)
                    wt = wl * mt * torch.where(bothm, 1.0 - s[:, 3], torch.ones_like(wl))
                    wr = wl * mr * torch.where(bothm, s[:, 3], torch.ones_like(wl))
                    r = torch.cat([s[refl, 4:11], s[refr, 11:18]]).contiguous()
                    w = torch.cat([wr[refl], wt[refr]])
                    root = torch.cat([root[refl], root[refr]])
                    remaining -= 1
            comp = _time(compose, reps, torch)
            api.render_status(world, allow_degenerate=True)
            color()
            api.render_status(world, allow_degenerate=True)
            out["compose"] = {"prepare_plus_shade_loop": comp, "max_abs_diff_to_color_at": float((total - d_rgb).abs().max()),
                              "ratio_compose_over_color_at": comp["median_ms"] / out["color_at_rays_device"]["median_ms"]}
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", default="mirror,csg,teapot")
    ap.add_argument("--only", default="all", choices=("all", "color"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rtc_shade_query.json"))
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        step(a.child, a.reps, a.only)
        return 0
    results = json.load(open(a.out)) if os.path.exists(a.out) else {}
    tag = os.environ.get("RL_RTC_SHADE_QUERY_TAG", "")
    for name in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--only", a.only]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
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
