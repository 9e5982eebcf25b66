"""GPU tier: the statements of Material::scatter + Material::emitted and of the instance POP against each other, bit for bit.  The shared
statement (csrc/rl_rtiow_scatter.h) is inlined by the counting general kernel, the wave-scheduled general kernels (ray-buffer form
included) and the scatter query; the fast general kernel's SHADE block, the cooperative kernel and the headline sphere kernel's `shade`
keep statements of their own, and this file is what holds those to the shared one.  The POP (pop_rec / pop_rec_chain,
csrc/rl_rtiow_general.h) is shared by the general, wave-scheduled general and hit-query kernels; the fast general kernel keeps its own
POP text too, held to the shared one here as well.  One small scene per family that reaches every material branch and both POP kinds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")


def _general_scene(b):
    checker = b.checker(0.8, b.solid((0.2, 0.3, 0.1)), b.solid((0.9, 0.9, 0.9)))
    ground = b.quad((-9.0, 0.0, -9.0), (18.0, 0.0, 0.0), (0.0, 0.0, 18.0), b.lambertian(checker))
    noisy = b.sphere((0.9, 0.7, 1.2), 0.7, b.lambertian(b.noise(4.0, 7)))
    fuzzy = b.sphere((-3.3, 1.0, 0.0), 1.0, b.metal((0.8, 0.6, 0.2), 0.6))
    mirror = b.sphere((0.5, 1.3, -2.6), 1.3, b.metal((0.9, 0.9, 0.9), 0.0))
    light = b.quad((-3.0, 2.8, -4.5), (6.0, 0.0, 0.0), (0.0, 1.6, 0.0), b.diffuse_light(b.solid((4.0, 3.5, 3.0))))
    flat = b.sphere((2.2, 0.35, 2.4), 0.35, b.flat())
    # a glass ball large enough to be entered and left and a checkered one, in object space; seen through scale, rotation and translation
    inside = b.list([b.sphere((0.0, 1.25, 0.0), 1.25, b.dielectric(1.5)), b.sphere((1.6, 0.5, 0.9), 0.5, b.lambertian(checker))])
    instance = b.translate(b.rotate_y(b.scale(inside, 0.8), 30.0), (-1.3, 0.0, 0.6))
    fog = b.constant_medium(b.sphere((3.2, 1.0, -0.3), 1.0, b.flat()), 1.2, b.isotropic(b.solid((0.7, 0.3, 0.9))))
    return b.list([ground, noisy, fuzzy, mirror, light, flat, instance, fog])


def _device_frame(rl, cam, world):
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.full((cam.c.image_height, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    st = rl.api.render_status(world, allow_degenerate=True)
    return buf.cpu().numpy(), st


def _frame_from_queries(rl, world, cam, path):
    """camera.rs:145-199 for the whole frame: sample s of a pixel on stream s * W * H + x * W + y, from the word its sample s - 1 stopped at;
    path(rays, cursors) -> (colours, final cursors, ray count, flagged).  -> sums in sample order, rays, flagged."""
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), W)
    acc = np.zeros((W * H, 3))
    pos = np.zeros(W * H, dtype=np.uint64)
    rays_total = flagged = 0
    for s in range(cam.params.samples_per_pixel):
        cur0 = rl.api.pack_cursors(np.uint64(s) * np.uint64(W * H) + x * np.uint64(W) + y, pos)
        rays, cur = cam.get_rays(x, y, cur0)
        rgb, cur, n_rays, n_flag = path(rays, cur)
        acc = acc + rgb
        pos = cur["word_pos"].copy()
        rays_total += n_rays
        flagged += n_flag
    return acc.reshape(H, W, 3), rays_total, flagged


def test_general_scene_five_ways(rl, oracle):
    api = rl.api
    rl.init(0)
    world = rl.World.build(_general_scene)
    assert world.counts()["media"] == 1
    p = rl.CameraParams(aspect_ratio=1.5, image_width=24, samples_per_pixel=4, max_depth=8, vfov=40.0, lookfrom=(0.0, 1.6, 9.0), lookat=(0.0, 1.0, 0.0),
                        background=(0.05, 0.06, 0.09), seed=1234)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (24, 16)
    table = world.materials()
    seen = []  # (material kind, front_face, scatter, emitted != 0) of every scatter_rays record of the host loop

    def ray_color(rays, cur):
        st = {}
        rgb, out, counts = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays, stats=st, allow_degenerate=True)
        assert st["rays"] == int(counts.sum(dtype=np.uint64))
        return rgb, out, st["rays"], st["flagged"]

    def host_loop(rays, cur):  # ray_color (camera.rs:232-260) from hit_rays_seeded + scatter_rays; only live paths are passed on
        n = rays.shape[0]
        bg = np.array(p.background, dtype=np.float64)
        total, thr = np.zeros((n, 3)), np.ones((n, 3))
        out_cur = cur.copy()
        live = np.arange(n)
        r, c = rays.copy(), cur.copy()
        n_rays = n_flag = 0
        for _ in range(p.max_depth):
            if live.size == 0:
                break
            st = {}
            hits, c = world.hit_rays_seeded(r, c, p.seed, tmin=1e-10, stats=st, allow_degenerate=True)
            n_rays += live.size
            n_flag += st["flagged"]
            out_cur[live] = c
            miss = hits["hit"] == 0
            total[live[miss]] = total[live[miss]] + thr[live[miss]] * bg
            live, r, c, hits = live[~miss], r[~miss], c[~miss], hits[~miss]
            if live.size == 0:
                break
            st = {}
            rec, c = world.scatter_rays(r, hits, c, p.seed, stats=st, allow_degenerate=True)
            n_flag += st["flagged"]
            seen.append(np.stack([table["kind"][hits["material"]], hits["front_face"], rec["scatter"], rec["emitted"].any(axis=1)], axis=1))
            total[live] = total[live] + thr[live] * rec["emitted"]
            out_cur[live] = c
            go = rec["scatter"] == 1
            thr[live[go]] = thr[live[go]] * rec["attenuation"][go]
            live, r, c = live[go], np.ascontiguousarray(rec["scattered"][go]), c[go]
        return total, out_cur, n_rays, n_flag

    gs = {}
    counting = cam.render(world, stats=gs, allow_degenerate=True).data
    frames = {"default": _device_frame(rl, cam, world)}
    api.set_fast_traversal(False)
    try:
        frames["fast traversal off"] = _device_frame(rl, cam, world)
    finally:
        api.set_fast_traversal(True)
    frames = {k: (f, st["rays"], st["flagged"]) for k, (f, st) in frames.items()}
    frames["ray_color_rays"] = _frame_from_queries(rl, world, cam, ray_color)
    frames["hit_rays_seeded + scatter_rays"] = _frame_from_queries(rl, world, cam, host_loop)
    for name, (frame, n_rays, n_flag) in frames.items():
        print(name, "rays", n_rays, "flagged", n_flag, "differing pixels", int((frame != counting).any(axis=2).sum()))
        assert np.array_equal(np.ascontiguousarray(frame).view(np.uint64), np.ascontiguousarray(counting).view(np.uint64)), name
        assert n_rays == gs["rays"] and n_flag == gs["flagged"], (name, n_rays, n_flag, gs)
    # the oracle, as in test_gpu_fuzz_general.py: counters exact, colours within 1e-9 relative
    cs = {}
    cpu = oracle.rtiow_render(world.desc, cam.c, stats=cs)
    for k in COUNTERS:
        assert gs[k] == cs[k], (k, gs[k], cs[k])
    err = np.abs(counting - cpu).max()
    print("oracle: max |d|", err, "of", np.abs(cpu).max(), "instance enters", gs["instance_enters"])
    assert err <= 1e-9 * max(1.0, np.abs(cpu).max())
    # the branches were reached (nothing is measured here: a scene that misses one would pass vacuously)
    seen = np.concatenate(seen)
    kind, front, scattered, emitted = seen[:, 0], seen[:, 1], seen[:, 2], seen[:, 3]
    reach = {"metal absorbed": int(((kind == api.MAT_METAL) & (scattered == 0)).sum()),
             "dielectric front": int(((kind == api.MAT_DIELECTRIC) & (front == 1)).sum()),
             "dielectric back": int(((kind == api.MAT_DIELECTRIC) & (front == 0)).sum()),
             "isotropic": int((kind == api.MAT_ISOTROPIC).sum()), "emitted": int((emitted != 0).sum()),
             "lambertian": int((kind == api.MAT_LAMBERTIAN).sum()), "flat": int((kind == api.MAT_FLAT).sum())}
    print(reach)
    assert all(v >= 1 for v in reach.values()), reach
    assert gs["instance_enters"] > 0


def test_sphere_scene_four_ways(rl):
    api = rl.api
    rl.init(0)
    tex = np.zeros(4, dtype=api.TEXTURE)
    tex["kind"][:3], tex["color"][:3] = api.TEX_SOLID, [(0.2, 0.3, 0.1), (0.9, 0.9, 0.9), (4.0, 3.5, 3.0)]
    tex[3]["kind"], tex[3]["inv_scale"], tex[3]["even"], tex[3]["odd"] = api.TEX_CHECKER, 1.0 / 0.8, 0, 1
    mats = np.zeros(5, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 3
    mats[1]["kind"], mats[1]["albedo"], mats[1]["fuzz"] = api.MAT_METAL, (0.8, 0.6, 0.2), 0.3
    mats[2]["kind"], mats[2]["ior"] = api.MAT_DIELECTRIC, 1.5
    mats[3]["kind"], mats[3]["texture"] = api.MAT_DIFFUSE_LIGHT, 2
    mats[4]["kind"] = api.MAT_FLAT
    sph = np.zeros(6, dtype=api.SPHERE)
    sph["center0"] = [(0.0, -100.5, 0.0), (-2.1, 0.5, 0.0), (0.0, 0.5, 0.3), (2.1, 0.5, 0.0), (0.0, 3.2, -1.5), (1.0, -0.2, 1.6)]
    sph["radius"] = [100.0, 1.0, 1.0, 1.0, 1.2, 0.3]
    sph["center1"] = sph["center0"]
    sph["material"] = [0, 1, 2, 0, 3, 4]
    world = rl.World.from_spheres(sph, mats, tex, True)
    p = rl.CameraParams(aspect_ratio=4.0 / 3.0, image_width=16, samples_per_pixel=4, max_depth=8, vfov=45.0, lookfrom=(0.0, 1.5, 7.0), lookat=(0.0, 0.7, 0.0),
                        background=(0.05, 0.06, 0.09), seed=77)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (16, 12)
    gs = {}
    counting = cam.render(world, stats=gs, allow_degenerate=True).data
    frames = {}
    try:
        frames["default (cooperative)"] = _device_frame(rl, cam, world)
        api.set_coop(False)
        frames["coop off"] = _device_frame(rl, cam, world)
        api.set_fast_traversal(False)
        frames["coop and fast traversal off"] = _device_frame(rl, cam, world)
        api.set_coop(True)
        frames["fast traversal off"] = _device_frame(rl, cam, world)
    finally:
        api.set_coop(True)
        api.set_fast_traversal(True)
    assert gs["rays"] > 16 * 12 * 4  # paths scatter
    for name, (frame, st) in frames.items():
        print(name, "rays", st["rays"], "differing pixels", int((frame != counting).any(axis=2).sum()))
        assert np.array_equal(frame.view(np.uint64), np.ascontiguousarray(counting).view(np.uint64)), name
        assert st["rays"] == gs["rays"] and st["flagged"] == gs["flagged"], (name, st, gs)
