"""GPU tier: the per-pixel entry table of the fast sphere kernel (csrc/rl_pixel_entry.h).  The camera rays of a pixel start their walk at
the entries a beam walk found for that pixel instead of at the root of the fast tree.  The frames must not change by a bit: the timed
frame equals the counting frame with the table on and with it off, `rays` and `slow_traces` are the same either way, and the table is
conservative — every sphere a ray from the extremes of a pixel's beam hits lies in the subtree of one of that pixel's entries."""
import numpy as np
import pytest

from test_gpu_fast_traversal import _mats, _same_bits

pytestmark = pytest.mark.gpu
FAST_NONE = 1023


def _timed(rl, cam, world, row_first=0, row_step=1, independent=False):
    import torch
    dev = torch.device("cuda", 0)
    rows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    buf = torch.full((rows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    render = cam.render_independent_device if independent else cam.render_device
    render(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream, row_first=row_first, row_step=row_step)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


def _on_off(rl, p_or_cam, world, row_first=0, row_step=1, entries=(3, 2, 1)):
    """Timed frames with the table at every cut size and switched off, against the counting frame: all the same bits and counts."""
    api = rl.api
    cam = p_or_cam if isinstance(p_or_cam, rl.Camera) else rl.Camera(p_or_cam)
    gs = {}
    counting = cam.render_rows(world, row_first, row_step, stats=gs) if (row_first, row_step) != (0, 1) else cam.render(world, stats=gs).data
    counting = np.asarray(counting).reshape(-1, cam.c.image_width, 3)
    try:
        api.set_coop(False)  # small frames: the wave-scheduled fast kernel, not the cooperative one
        api.set_pixel_entry(0)
        off, st_off = _timed(rl, cam, world, row_first, row_step)
        assert _same_bits(off, counting) and st_off["rays"] == gs["rays"]
        for n in entries:
            api.set_pixel_entry(n)
            on, st_on = _timed(rl, cam, world, row_first, row_step)
            print("entries", n, "rays", st_on["rays"], "slow_traces", st_on["slow_traces"], "off:", st_off["rays"], st_off["slow_traces"])
            assert _same_bits(on, counting), n
            assert st_on["rays"] == st_off["rays"] and st_on["slow_traces"] == st_off["slow_traces"] and st_on["flagged"] == st_off["flagged"], n
    finally:
        api.set_pixel_entry(3)
        api.set_coop(True)
    return st_off


def _random_world(rl, n, seed, use_bvh=True):
    """The recipe of test_gpu_fast_traversal.test_random_worlds_overlapping_moving_every_material."""
    rng = np.random.default_rng(4000 + seed)
    api = rl.api
    tex, mats = _mats(api)
    sph = np.zeros(n, dtype=api.SPHERE)
    sph["center0"] = rng.uniform(-3, 3, (n, 3))
    sph["center1"] = sph["center0"] + rng.uniform(0, 0.5, (n, 3))
    sph["radius"] = rng.uniform(0.05, 0.9, n)
    sph["moving"] = rng.integers(0, 2, n)
    sph["material"] = rng.integers(0, 5, n)
    return rl.World.from_spheres(sph, mats, tex, use_bvh), sph


def test_baseline_scene_with_its_own_camera_and_the_resume_path(rl):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 160, 72, 50  # spp >= 64: probe launch + cost-sorted resume launch
    _on_off(rl, p, world)


@pytest.mark.parametrize("defocus", [0.0, 10.0])
def test_no_lens_and_a_wide_lens(rl, defocus):
    world = rl.World.golden_test_scene()
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth, p.defocus_angle = 120, 8, 20, defocus
    _on_off(rl, p, world)


def test_camera_inside_a_small_spheres_box(rl):
    api = rl.api
    tex, mats = _mats(api)
    sph = np.zeros(6, dtype=api.SPHERE)
    sph["center0"] = [(0, 0, 0), (1.2, 0.1, -2), (-1.0, 0.3, -3), (0.2, -0.1, 2.0), (0, -100.5, 0), (0.5, 0.8, -1.5)]
    sph["radius"] = [0.5, 0.5, 0.7, 0.4, 100.0, 0.3]
    sph["material"] = [3, 0, 2, 1, 4, 0]
    world = rl.World.from_spheres(sph, mats, tex, True)
    # inside the padded box of sphere 0 but outside the sphere (a corner of the box), and once inside the glass sphere itself
    for lookfrom in [(0.45, 0.45, 0.45), (0.1, 0.0, 0.1)]:
        p = rl.CameraParams(aspect_ratio=1.5, image_width=96, samples_per_pixel=6, max_depth=10, vfov=70.0, lookfrom=lookfrom, lookat=(0.6, 0.2, -2.0),
                            defocus_angle=2.0, focus_dist=2.0, background=(0.6, 0.7, 0.9), seed=3)
        _on_off(rl, p, world)


@pytest.mark.parametrize("n,use_bvh,seed", [(1, True, 1), (2, True, 2), (9, True, 4), (37, True, 5), (150, False, 6), (511, True, 8)])
def test_random_overlapping_worlds_with_moving_spheres(rl, n, use_bvh, seed):
    world, _ = _random_world(rl, n, seed, use_bvh)
    p = rl.CameraParams(aspect_ratio=1.5, image_width=96, samples_per_pixel=6, max_depth=12, vfov=50.0, lookfrom=(0.0, 1.0, 9.0),
                        lookat=(0.0, 0.0, 0.0), defocus_angle=1.0, focus_dist=9.0, background=(0.5, 0.6, 0.9), seed=seed)
    _on_off(rl, p, world)


@pytest.mark.parametrize("w,aspect", [(1, 1.0), (3, 1.5)])
def test_tiny_frames(rl, w, aspect):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.aspect_ratio, p.samples_per_pixel, p.max_depth = w, aspect, 16, 20
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == ((1, 1) if w == 1 else (3, 2))
    _on_off(rl, cam, world)


def test_row_shard(rl):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 128, 66, 30
    _on_off(rl, p, world, row_first=3, row_step=8)


def test_camera_outside_reach_falls_back(rl):
    world, _ = _random_world(rl, 40, 9)
    far = rl.CameraParams(aspect_ratio=1.5, image_width=72, samples_per_pixel=4, max_depth=8, vfov=2.0, lookfrom=(0.0, 0.0, 400.0), lookat=(0, 0, 0))
    st = _on_off(rl, far, world)
    assert st["slow_traces"] == 0  # the reference-order kernel rendered it: nothing read the table


def test_sample_parallel_mode_shares_the_table(rl):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 96, 12, 30
    cam = rl.Camera(p)
    api = rl.api
    try:
        api.set_pixel_entry(0)
        off, st_off = _timed(rl, cam, world, independent=True)
        api.set_pixel_entry(3)
        on, st_on = _timed(rl, cam, world, independent=True)
    finally:
        api.set_pixel_entry(3)
    assert _same_bits(on, off) and st_on["rays"] == st_off["rays"] and st_on["slow_traces"] == st_off["slow_traces"]


def _scene_spheres(world):
    """The scene descriptor's sphere array (rl_rtiow_scene_desc starts with {const rl_sphere *spheres; uint32_t n_spheres})."""
    import ctypes as C
    ptr = C.cast(world.desc, C.POINTER(C.c_void_p))[0]
    n = C.cast(world.desc + 8, C.POINTER(C.c_uint32))[0]
    buf = (C.c_char * (n * 64)).from_address(ptr)
    return np.frombuffer(buf, dtype=np.dtype([("center0", "<f8", 3), ("center1", "<f8", 3), ("radius", "<f8"), ("moving", "<u4"), ("material", "<u4")])).copy()


def _subtree_spheres(children, n_inner, entry, cache):
    if entry == FAST_NONE:
        return frozenset()
    if entry >= n_inner:
        return frozenset([entry - n_inner])
    if entry not in cache:
        cache[entry] = _subtree_spheres(children, n_inner, int(children[entry][0]), cache) | _subtree_spheres(children, n_inner, int(children[entry][1]), cache)
    return cache[entry]


def _beam_extreme_rays(c, px, py, rng):
    """Rays from the extremes of pixel (px, py)'s beam: lens rim (and centre) x pixel corners (and centre), get_ray's arithmetic."""
    p00, du, dv = np.array(c.pixel_00[:]), np.array(c.pixel_du[:]), np.array(c.pixel_dv[:])
    lf, U, V = np.array(c.lookfrom[:]), np.array(c.defocus_disk_u[:]), np.array(c.defocus_disk_v[:])
    center = (p00 + du * float(px)) + dv * float(py)
    half = 0.5 - 2.0 ** -53
    offs = [(-0.5, -0.5), (-0.5, half), (half, -0.5), (half, half), (0.0, 0.0), tuple(rng.uniform(-0.5, 0.5, 2))]
    if c.defocus_angle <= 0.0:
        lens = [(0.0, 0.0)]
    else:
        ang = np.concatenate([np.arange(8) * (np.pi / 4), rng.uniform(0, 2 * np.pi, 2)])
        lens = [(np.cos(a) * (1 - 1e-12), np.sin(a) * (1 - 1e-12)) for a in ang] + [(0.0, 0.0)]
    o, d = [], []
    for a, b in lens:
        org = lf if c.defocus_angle <= 0.0 else (lf + U * a) + V * b
        for sx, sy in offs:
            o.append(org)
            d.append((center + (du * sx + dv * sy)) - org)
    return np.array(o), np.array(d)


@pytest.mark.parametrize("scene", ["baseline", "random_moving"])
@pytest.mark.parametrize("entries", [1, 3])
def test_table_is_conservative(rl, scene, entries):
    api = rl.api
    rng = np.random.default_rng(17)
    if scene == "baseline":
        world = rl.World.bouncing_spheres(1)
        p = world.params
        p.image_width, p.samples_per_pixel, p.max_depth = 240, 1, 2
    else:
        world, _ = _random_world(rl, 150, 6)
        p = rl.CameraParams(aspect_ratio=1.5, image_width=120, samples_per_pixel=1, max_depth=2, vfov=60.0, lookfrom=(0.0, 1.0, 9.0), lookat=(0.0, 0.0, 0.0),
                            defocus_angle=3.0, focus_dist=9.0, background=(0.5, 0.6, 0.9), seed=2)
    cam = rl.Camera(p)
    c = cam.c
    W, H = c.image_width, c.image_height
    try:
        api.set_coop(False)
        api.set_pixel_entry(entries)
        _timed(rl, cam, world)
        table = api.pixel_entry_table(world, W * H).reshape(H, W)
    finally:
        api.set_pixel_entry(3)
        api.set_coop(True)
    children, root = api.fast_tree(world)
    n_inner = len(children)
    assert np.all(table >> 30 == 3)
    e = np.stack([table & 1023, (table >> 10) & 1023, (table >> 20) & 1023], axis=-1)
    assert np.all((e[..., 1:] == FAST_NONE) | (e[..., :1] != FAST_NONE))  # the first slot is used first
    if entries == 1:
        assert np.all(e[..., 1:] == FAST_NONE)
    # pixel classes: sky (no entry), one leaf, an inner node / several entries; every class present in the frame is sampled, plus the
    # horizon rows (the first rows in which the entry changes from none to some along a column) and random pixels
    n_used = (e != FAST_NONE).sum(-1)
    leaf_only = (n_used == 1) & (e[..., 0] >= n_inner)
    classes = {"sky": n_used == 0, "one_leaf": leaf_only, "inner_or_cut": (n_used >= 1) & ~leaf_only}
    horizon = np.zeros_like(leaf_only)
    horizon[1:] = (n_used[1:] > 0) != (n_used[:-1] > 0)
    classes["horizon"] = horizon
    if scene == "baseline":
        assert all(m.any() for m in classes.values()), {k: int(m.sum()) for k, m in classes.items()}
    picks = set()
    for name, m in classes.items():
        ys, xs = np.nonzero(m)
        for k in rng.permutation(len(ys))[:80]:
            picks.add((int(xs[k]), int(ys[k])))
    for _ in range(80):
        picks.add((int(rng.integers(W)), int(rng.integers(H))))
    cache, o_all, d_all, t_all, owner = {}, [], [], [], []
    picks = sorted(picks)
    for i, (px, py) in enumerate(picks):
        o, d = _beam_extreme_rays(c, px, py, rng)
        for tm in (0.0, 1.0 - 2.0 ** -53, float(rng.uniform())):
            o_all.append(o), d_all.append(d), t_all.append(np.full(len(o), tm)), owner.append(np.full(len(o), i))
    o_all, d_all, t_all, owner = np.concatenate(o_all), np.concatenate(d_all), np.concatenate(t_all), np.concatenate(owner)
    hits = world.hit_rays(o_all, d_all, t_all)
    sph = _scene_spheres(world)
    bad = 0
    for i, (px, py) in enumerate(picks):
        allowed = sorted(frozenset().union(*[_subtree_spheres(children, n_inner, int(x), cache) for x in e[py, px]]))
        m = (owner == i) & (hits["hit"] != 0)
        if not m.any():
            continue
        if not allowed:
            bad += 1
            print("pixel", px, py, "has no entry but", int(m.sum()), "of its rays hit")
            continue
        # the hit point lies on the surface of one of the allowed spheres (at the ray's time): | |p - c| - r | <= 1e-9 r
        pts, tms = hits["p"][m], t_all[m]
        c0, c1, r, mov = sph["center0"][allowed], sph["center1"][allowed], np.abs(sph["radius"][allowed]), sph["moving"][allowed] != 0
        ctr = c0[None] + np.where(mov[None, :, None], (c1 - c0)[None] * tms[:, None, None], 0.0)
        res = np.abs(np.linalg.norm(pts[:, None, :] - ctr, axis=-1) - r[None]) / r[None]
        worst = res.min(axis=1).max()
        if not worst <= 1e-9:
            bad += 1
            print("pixel", px, py, "entries", e[py, px], "a hit point is", worst, "(relative) off every sphere below its entries")
    print(scene, "entries", entries, "pixels checked", len(picks), "rays", len(o_all), {k: int(m.sum()) for k, m in classes.items()})
    assert bad == 0
    assert len(picks) >= 200
