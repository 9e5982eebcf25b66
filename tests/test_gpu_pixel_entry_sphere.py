"""GPU tier: the sphere test of the per-pixel entry table (csrc/rl_pixel_entry.h).  A leaf stays in a pixel's cut only when the pixel's beam
may touch the SPHERE, not just its padded box.  The test may only ever remove a leaf that no camera ray of the pixel can hit, so frames,
ray counts and re-traces are those of the box-only cut and of the root walk, bit for bit.

What a word shows of the touched set: an entry that is a leaf is a touched leaf, and a word made of leaves only IS the touched set (at most
three leaves); an inner entry only says that the touched leaves lie below it.  The effect tests use exactly that."""
import numpy as np
import pytest

from test_gpu_fast_traversal import _mats, _same_bits
from test_gpu_pixel_entry import FAST_NONE, _beam_extreme_rays, _random_world, _scene_spheres, _subtree_spheres, _timed

pytestmark = pytest.mark.gpu


def _baseline(rl, defocus=None, width=160, spp=16, depth=8):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = width, spp, depth
    if defocus is not None:
        p.defocus_angle = defocus
    return world, p


def _inside_camera(rl, width=160):
    """Inside the field of small spheres (their tops are at y = 0.4, the moving ones rise to 0.9), a short way from several of them."""
    return rl.CameraParams(aspect_ratio=16.0 / 9.0, image_width=width, samples_per_pixel=1, max_depth=2, vfov=60.0, lookfrom=(1.45, 0.45, 2.45),
                           lookat=(0.0, 0.6, 0.0), defocus_angle=0.6, focus_dist=3.0, background=(0.7, 0.8, 1.0), seed=5)


def _words(rl, cam, world, sphere, entries=3, read=True, **kw):
    """(frame, status, entry ids [rows, W, 3]) of one timed render with the sphere test on / off."""
    api = rl.api
    try:
        api.set_coop(False)  # small frames: the wave-scheduled fast kernel, not the cooperative one (which starts at the root)
        api.set_pixel_entry(entries)
        api.set_pixel_entry_sphere(sphere)
        frame, st = _timed(rl, cam, world, **kw)
        rows = frame.shape[0]
        table = api.pixel_entry_table(world, rows * cam.c.image_width).reshape(rows, cam.c.image_width) if entries and read else None
    finally:
        api.set_pixel_entry(3)
        api.set_pixel_entry_sphere(True)
        api.set_coop(True)
    if table is None:
        return frame, st, None
    assert np.all(table >> 30 == 3)
    return frame, st, np.stack([table & 1023, (table >> 10) & 1023, (table >> 20) & 1023], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- bit-equality
@pytest.mark.parametrize("entry_point", ["sample_parallel", "row_shard"])
@pytest.mark.parametrize("defocus", ["lens", "no_lens"])
@pytest.mark.parametrize("scene", ["baseline", "random_moving"])
def test_frames_rays_and_retraces_do_not_change(rl, scene, defocus, entry_point):
    if scene == "baseline":
        world, p = _baseline(rl, defocus=None if defocus == "lens" else 0.0)
    else:
        world, _ = _random_world(rl, 64, 3)
        p = rl.CameraParams(aspect_ratio=16.0 / 9.0, image_width=64, samples_per_pixel=8, max_depth=8, vfov=50.0, lookfrom=(0.0, 1.0, 9.0), lookat=(0.0, 0.0, 0.0),
                            defocus_angle=1.5 if defocus == "lens" else 0.0, focus_dist=9.0, background=(0.5, 0.6, 0.9), seed=11)
    cam = rl.Camera(p)
    assert (cam.c.defocus_angle > 0.0) == (defocus == "lens")
    kw = dict(independent=True) if entry_point == "sample_parallel" else dict(row_first=1, row_step=3)
    on, st_on, e_on = _words(rl, cam, world, True, **kw)
    box, st_box, e_box = _words(rl, cam, world, False, **kw)
    root, st_root, _ = _words(rl, cam, world, True, entries=0, **kw)
    print(scene, defocus, entry_point, "rays", st_on["rays"], "slow_traces", st_on["slow_traces"], "words that differ", int((e_on != e_box).any(-1).sum()), "of", e_on.shape[0] * e_on.shape[1])
    assert _same_bits(on, box) and _same_bits(on, root)
    for k in ("rays", "slow_traces", "flagged"):
        assert st_on[k] == st_box[k] == st_root[k], k
    assert st_on["rays"] > 0


# ---------------------------------------------------------------------------------------------------------------- conservativeness
def _pixel_classes(e_on, e_box, n_inner, moving_entries):
    n_used = (e_on != FAST_NONE).sum(-1)
    horizon = np.zeros(n_used.shape, dtype=bool)
    horizon[1:] = (n_used[1:] > 0) != (n_used[:-1] > 0)
    corners = np.zeros_like(horizon)
    corners[0, 0] = corners[0, -1] = corners[-1, 0] = corners[-1, -1] = True
    return {"silhouette": (e_on != e_box).any(-1),  # the sphere test removed something: the beam passes a box corner next to a sphere
            "horizon": horizon, "moving": np.isin(e_on, moving_entries).any(-1), "corners": corners,
            "leaves_only": (n_used >= 1) & np.all((e_on >= n_inner) | (e_on == FAST_NONE), axis=-1), "inner": np.any(e_on < n_inner, axis=-1)}


@pytest.mark.parametrize("camera", ["scene_camera", "inside_the_field"])
def test_no_camera_ray_hits_a_removed_sphere(rl, camera):
    api = rl.api
    rng = np.random.default_rng(23)
    world, p = _baseline(rl, spp=1, depth=2)
    if camera == "inside_the_field":
        p = _inside_camera(rl)
    cam = rl.Camera(p)
    c = cam.c
    W, H = c.image_width, c.image_height
    assert (W, H) == (160, 90)
    _, _, e_on = _words(rl, cam, world, True)
    _, _, e_box = _words(rl, cam, world, False)
    children, _ = api.fast_tree(world)
    n_inner = len(children)
    sph = _scene_spheres(world)
    classes = _pixel_classes(e_on, e_box, n_inner, n_inner + np.nonzero(sph["moving"])[0])
    assert all(m.any() for m in classes.values()), {k: int(m.sum()) for k, m in classes.items()}
    picks = set()
    for name, m in classes.items():
        ys, xs = np.nonzero(m)
        for k in rng.permutation(len(ys))[:120 if name == "silhouette" else 60]:
            picks.add((int(xs[k]), int(ys[k])))
    while len(picks) < 400:
        picks.add((int(rng.integers(W)), int(rng.integers(H))))
    picks = sorted(picks)
    # the beam's extreme rays at three times each, and 256 seeded camera rays per pixel (stream of sample s at (x, y): s W H + x W + y, camera.rs:161-170)
    o_all, d_all, t_all, owner = [], [], [], []
    for i, (px, py) in enumerate(picks):
        o, d = _beam_extreme_rays(c, px, py, rng)
        for tm in (0.0, 1.0 - 2.0 ** -53, float(rng.uniform())):
            o_all.append(o), d_all.append(d), t_all.append(np.full(len(o), tm)), owner.append(np.full(len(o), i))
    n_seeded = 256
    pxs = np.repeat(np.array([q[0] for q in picks], dtype=np.uint32), n_seeded)
    pys = np.repeat(np.array([q[1] for q in picks], dtype=np.uint32), n_seeded)
    samples = np.tile(np.arange(n_seeded, dtype=np.uint64), len(picks))
    rays, _ = cam.get_rays(pxs, pys, api.pack_cursors(samples * np.uint64(W * H) + pxs.astype(np.uint64) * np.uint64(W) + pys.astype(np.uint64)))
    o_all.append(rays["origin"]), d_all.append(rays["dir"]), t_all.append(rays["time"]), owner.append(np.repeat(np.arange(len(picks)), n_seeded))
    o_all, d_all, t_all, owner = np.concatenate(o_all), np.concatenate(d_all), np.concatenate(t_all), np.concatenate(owner)
    hits = world.hit_rays(o_all, d_all, t_all)
    cache, bad, n_hit = {}, 0, 0
    for i, (px, py) in enumerate(picks):
        allowed = sorted(frozenset().union(*[_subtree_spheres(children, n_inner, int(x), cache) for x in e_on[py, px]]))
        m = (owner == i) & (hits["hit"] != 0)
        if not m.any():
            continue
        n_hit += int(m.sum())
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
            print("pixel", px, py, "entries", e_on[py, px], "box-only", e_box[py, px], "a hit point is", worst, "(relative) off every sphere below its entries")
    print(camera, "pixels", len(picks), "rays", len(o_all), "hits", n_hit, {k: int(m.sum()) for k, m in classes.items()})
    assert bad == 0
    assert len(picks) >= 400 and n_hit > 0


# ---------------------------------------------------------------------------------------------------------------- effect
@pytest.mark.parametrize("camera", ["scene_camera", "inside_the_field"])
def test_the_cut_shrinks_and_keeps_what_the_beam_crosses(rl, camera):
    api = rl.api
    world, p = _baseline(rl, spp=1, depth=2)
    if camera == "inside_the_field":
        p = _inside_camera(rl)
    cam = rl.Camera(p)
    c = cam.c
    W, H = c.image_width, c.image_height
    _, _, e_on = _words(rl, cam, world, True)
    _, _, e_box = _words(rl, cam, world, False)
    children, _ = api.fast_tree(world)
    n_inner = len(children)
    cache = {}
    below = lambda word: frozenset().union(*[_subtree_spheres(children, n_inner, int(x), cache) for x in word])
    leaves = lambda word: frozenset(int(x) - n_inner for x in word if x != FAST_NONE and x >= n_inner)
    only_leaves = lambda word: all(x == FAST_NONE or x >= n_inner for x in word)
    tot_on = tot_box = exact_on = exact_box = 0
    for y in range(H):
        for x in range(W):
            w_on, w_box = e_on[y, x], e_box[y, x]
            b_box = below(w_box)
            assert leaves(w_on) <= b_box, (x, y, w_on, w_box)  # a touched leaf of the new cut is below the box-only cut
            if only_leaves(w_box):  # the box-only word IS its touched set: the new word is a set of leaves too, and a subset
                assert only_leaves(w_on) and leaves(w_on) <= leaves(w_box), (x, y, w_on, w_box)
                exact_on += len(leaves(w_on)); exact_box += len(leaves(w_box))
            tot_on += len(below(w_on)); tot_box += len(b_box)
    n_leaf_on = int(np.all((e_on >= n_inner) | (e_on == FAST_NONE), axis=-1).sum())
    n_leaf_box = int(np.all((e_box >= n_inner) | (e_box == FAST_NONE), axis=-1).sum())
    print(camera, "touched leaves where the box-only word is leaves only:", exact_on, "of", exact_box, " spheres below the entries:", tot_on, "of", tot_box,
          " words of leaves only:", n_leaf_on, "against", n_leaf_box, "of", W * H)
    assert exact_on < exact_box and tot_on < tot_box and n_leaf_on >= n_leaf_box
    # a pixel whose beam holds the ray from the lens centre through a sphere's centre (at time 0) keeps that sphere
    sph = _scene_spheres(world)
    p00, du, dv, lf = np.array(c.pixel_00[:]), np.array(c.pixel_du[:]), np.array(c.pixel_dv[:]), np.array(c.lookfrom[:])
    kept = 0
    for s, ctr in enumerate(sph["center0"]):
        # lookfrom + k (ctr - lookfrom) = p00 + x du + y dv
        k, x, y = np.linalg.solve(np.stack([ctr - lf, -du, -dv], axis=1), p00 - lf)
        px, py = int(np.rint(x)), int(np.rint(y))
        if not (k > 0.0 and 0 <= px < W and 0 <= py < H and abs(x - px) < 0.49 and abs(y - py) < 0.49):
            continue
        assert s in below(e_on[py, px]), (s, px, py, e_on[py, px])
        kept += 1
    print("spheres whose centre projects into the frame:", kept)
    assert kept >= 100


# ---------------------------------------------------------------------------------------------------------------- degenerate inputs
@pytest.mark.parametrize("field,index,value", [("pixel_du", 0, float("nan")), ("pixel_00", 1, float("inf")), ("pixel_dv", 2, float("-inf")), ("pixel_00", 2, float("nan"))])
def test_a_non_finite_camera_field_gives_the_box_only_words(rl, field, index, value):
    world, p = _baseline(rl, width=64, spp=2, depth=4)
    cam = rl.Camera(p)
    getattr(cam.c, field)[index] = value
    on, st_on, e_on = _words(rl, cam, world, True)
    box, st_box, e_box = _words(rl, cam, world, False)
    assert np.array_equal(e_on, e_box)
    assert _same_bits(on, box) and st_on["rays"] == st_box["rays"] and st_on["slow_traces"] == st_box["slow_traces"]


def test_a_scene_without_a_fast_structure_has_no_table_either_way(rl):
    api = rl.api
    tex, mats = _mats(api)
    sph = np.zeros(4, dtype=api.SPHERE)
    sph["center0"] = [(0, 0, -1), (0, 0, -1.1), (-1.0, 0.2, -2.5), (0, -100.5, -1)]
    sph["radius"] = [0.5, 0.0, 0.6, 100.0]  # a radius-0 sphere (inside the diffuse one, where no ray gets): no padding is finite, the scene never gets the fast tree
    sph["material"] = [0, 2, 3, 4]
    world = rl.World.from_spheres(sph, mats, tex, True)
    assert api.fast_tree(world) is None
    cam = rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=48, samples_per_pixel=4, max_depth=6, vfov=60.0, defocus_angle=1.0, focus_dist=1.5))
    frames = []
    try:
        for on in (True, False):
            api.set_pixel_entry_sphere(on)
            frame, st = _timed(rl, cam, world)
            frames.append((frame, st["rays"]))
    finally:
        api.set_pixel_entry_sphere(True)
    assert _same_bits(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]
    counting = cam.render(world).data
    assert _same_bits(frames[0][0], np.asarray(counting).reshape(frames[0][0].shape))


def test_max_depth_zero_renders_black(rl):
    world, p = _baseline(rl, width=64, spp=3, depth=0)
    cam = rl.Camera(p)
    on, st_on, _ = _words(rl, cam, world, True, read=False)
    box, st_box, _ = _words(rl, cam, world, False, read=False)
    assert np.all(on == 0.0) and _same_bits(on, box) and st_on["rays"] == st_box["rays"]
