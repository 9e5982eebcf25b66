"""GPU tier: every route of the RTIOW launch tables (csrc/rl_rtiow_launch.h).

The four launchers (frame / moments / adaptive, sample-parallel, pixel lists, path query) pick their kernel instantiation from one table per
kernel family, by the scene's flags: a sphere-only world with the fast structure, and general worlds with and without transcendental
texture code (`trans`: a Noise texture) and with and without a ConstantMedium (`media`).  Five tiny worlds cover the four (trans, media)
flavours and the sphere kernels; on each, every entry point runs counter-free and counting, and the identities the project states
elsewhere (tests/test_gpu_wave_block_paths.py, test_gpu_render_pixels.py, test_gpu_render_moments.py, test_gpu_render_adaptive.py,
test_gpu_independent_samples.py, test_gpu_path_query.py) must hold bit for bit.

Equal bits do not show WHICH kernel rendered them: a wrong table row that still renders the right bits (TRANS set on a scene without
Noise), or route A silently being route B, passes every comparison.  So beside each comparison the test reads the library's launch log
(api.rtiow_launches: the kernel as the runtime names the function pointer that was launched, workgroup size, dynamic LDS, sample range)
and compares it with `_route` below — this file's own statement of DESIGN.md §3.1c, §3.6a, §3.7, §3.13 - §3.15 and §6, from the world's
construction, the entry point, counting or not, and the switches.  It never asks the library which kernel it would take.  Below the nine
cases, every threshold of those rules is held from both sides at 1 spp.

24 x 16 pixels at 64 spp (>= 64: the probe launch, the tile sort and the resumed launch run), depth 6."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
W, H, SPP, DEPTH = 24, 16, 64, 6
MIN, EVERY = 4, 4
WORLDS = ["spheres", "quads", "quads_noise", "media", "media_noise"]
FAST_DEPTH_MASK = 0x3FFFFF  # the fast sphere layout keeps a path's remaining depth in 22 bits (csrc/rl_program.h)
LPT_FIRST = 8  # samples of the probe launch


def _restore(api):
    api.set_coop(True), api.set_fast_traversal(True), api.set_steal(3.0), api.set_indep_k(1), api.set_fastg_one_wave(-1), api.set_lpt(True)


# ----------------------------------------------------------------------------- the expected route, stated here
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _b(v):
    return "true" if v else "false"


def _route(world, entry, counting, *, npix=W * H, n_list=40, spp=SPP, depth=DEPTH, coop=True, fast=True, lpt=True, steal=3.0, one_wave=-1):
    """The launches one call makes, oldest first, as a list of dicts with the fields _assert_route compares.

    world: "spheres" (sphere-only, small enough for every LDS layout, the camera within the guard frame's reach: it has the fast structure)
    or a general world named by its construction: "noise" in the name = a Noise texture (the transcendental code, TRANS), "media" = a
    ConstantMedium.  entry: frame / moments / adaptive / indep / pixels / pixels_moments / rays.  counting: the caller passed rl_stats.
    npix: pixels of the frame or shard; n_list: elements of the list; coop, fast, lpt, steal, one_wave: the switches as the test set them.

    Kernel families:
      reference   rtiow_wave_general*_kernel<512, TRANS, STATS, MEDIA>: every counting call but the sphere frame, and whatever no faster
                  kernel takes.  512 lanes; LDS 512 x (16 + 12 with a medium) x 8.
      fastgen     rtiow_fast_general*_kernel<NT, SD, TRANS, MEDIA>: counter-free calls on general worlds; the path query on every world.
                  <768, 20> plain, <512, 40> with TRANS or MEDIA; with both, and for frame / indep / pixels only, <256, 40, true, true>
                  while the work is at most 1536 items per CU (set_fastg_one_wave forces it on / off).  LDS NT x (128 + 4 SD) + 128 per
                  staged top node, at least 90000 in the one-wave form.
      wave        rtiow_wave_kernel<1024, L, STATS, STEAL> / rtiow_wave_moments_kernel<1024, L> / rtiow_wave_indep_kernel<1024, 4, false>:
                  sphere worlds.  L = 4 (fast tree; counter-free, max_depth <= FAST_DEPTH_MASK), else 3 (guarded compact ops: counting
                  frames, set_fast_traversal(0), deeper paths).  LDS 16 x 1024 x 8 + the layout's scene bytes.
      coop        rtiow_coop*_kernel<4, BOXES_IN_REGS, REGS>: counter-free sphere frames / lists of at most 160 pixels per CU;
                  <4, true, 256> up to 8 pixels per CU, <4, false, 1024> above.  256 lanes; LDS 8 x 256 x 8 + 4 x 128 x 4.
    Flow: frame, moments and adaptive calls of spp >= 64 launch twice — samples [0, 8), then [8, spp) with resume and the sorted tile
    order — on every kernel they reach here; everything else launches once over [0, spp) (one sample pass at this size).  The resume
    launch of a counter-free layout-4 FRAME steals (STEAL = true, steal_state set) when npix <= steal x CUs x 1024."""
    cus = _cus()
    spheres, trans, media = world == "spheres", "noise" in world, "media" in world
    suffix = {"frame": "", "moments": "_moments", "adaptive": "_moments", "indep": "_indep", "pixels": "_pixels", "pixels_moments": "_pixels_moments", "rays": "_rays"}[entry]

    def reference(stats):
        return dict(family="reference", kernel=f"rtiow_wave_general{suffix}_kernel<512, {_b(trans)}, {_b(stats)}, {_b(media)}>", wg_size=512, funnel="value",
                    lds=512 * (16 + (12 if media else 0)) * 8)

    def fastgen(work_items, has_one_wave_form, t=trans, m=media):
        one = has_one_wave_form and t and m and (one_wave == 1 or (one_wave == -1 and work_items <= cus * 1536))
        nt, sd = (256, 40) if one else (512, 40) if (t or m) else (768, 20)
        return dict(family="fastgen", kernel=f"rtiow_fast_general{suffix}_kernel<{nt}, {sd}, {_b(t)}, {_b(m)}>", wg_size=nt, funnel="pointer", lds=("fastgen", nt, sd, one))

    def cooperative(n):
        regs = n <= cus * 8
        return dict(family="coop", kernel=f"rtiow_coop{suffix}_kernel<4, {'true, 256' if regs else 'false, 1024'}>", wg_size=256, funnel="coop", lds=8 * 256 * 8 + 4 * 128 * 4, n_pixels=n)

    def wave(layout, stats=False):
        if entry in ("moments", "adaptive"):
            name = f"rtiow_wave_moments_kernel<1024, {layout}>"
        elif entry == "indep":
            name = "rtiow_wave_indep_kernel<1024, 4, false>"
        else:
            name = f"rtiow_wave_kernel<1024, {layout}, {_b(stats)}, false>"
        return dict(family="wave", kernel=name, wg_size=1024, funnel="value", lds=("wave", layout), layout=layout)

    deep = depth > FAST_DEPTH_MASK
    if entry == "rays":  # the queries' own tree on sphere worlds: no Noise, no medium there
        k = reference(True) if counting else fastgen(n_list, False, trans and not spheres, media and not spheres) if fast else reference(False)
        return [dict(k, samples=None)]
    if entry in ("pixels", "pixels_moments"):
        if counting:
            k = reference(True)
        elif not spheres:
            k = fastgen(n_list, entry == "pixels") if fast else reference(False)
        else:
            k = cooperative(n_list) if fast and coop and not deep and n_list <= cus * 160 else reference(False)
        return [dict(k, samples=(0, spp), resume=0, tile_order=False, steal_state=False)]
    if entry == "indep":
        if counting:
            k = reference(True)
        elif not spheres:
            k = fastgen(npix, True) if fast else reference(False)
        else:
            k = wave(4) if fast and not deep else reference(False)
        return [dict(k, samples=(0, spp), resume=0, tile_order=False, steal_state=False)]
    # frame, moments, adaptive
    if not spheres:
        k = fastgen(npix, entry == "frame") if fast and not counting else reference(counting)
    elif counting:
        k = wave(3, True) if entry == "frame" else reference(True)
    elif not fast:
        k = wave(3)
    elif coop and npix <= cus * 160:
        k = cooperative(npix) if entry != "adaptive" else reference(False) if deep else wave(4)
    else:
        k = wave(3) if deep else wave(4)
    if not (lpt and spp >= 64):
        return [dict(k, samples=(0, spp), resume=0, tile_order=False, steal_state=False)]
    second = dict(k, samples=(LPT_FIRST, spp), resume=1, tile_order=True, steal_state=False)
    if k["family"] == "wave" and k.get("layout") == 4 and entry == "frame" and steal > 0.0 and float(npix) <= steal * float(cus) * 1024.0:
        second.update(kernel="rtiow_wave_kernel<1024, 4, false, true>", steal_state=True)
    return [dict(k, samples=(0, LPT_FIRST), resume=0, tile_order=False, steal_state=False), second]


class _Log:
    """The launches since the last take()."""

    def __init__(self, api):
        self.api, self.total = api, api.rtiow_launch_total()

    def take(self):
        recs = self.api.rtiow_launches(self.total)
        self.total += len(recs)
        assert self.total == self.api.rtiow_launch_total()
        return recs


_names = {}  # test id -> the kernel names its calls launched (test_the_names_are_those_of_the_recorded_trace)


def _assert_route(api, recs, want, what, world=None, seen=None):
    """The launches `recs` of one call against _route's answer: kernel name, funnel, workgroup size, dynamic LDS, sample range, flow flags."""
    got = [(r["kernel"], r["funnel"]) for r in recs]
    assert got == [(w["kernel"], w["funnel"]) for w in want], (what, got, [w["kernel"] for w in want])
    for r, w in zip(recs, want):
        assert r["wg_size"] == w["wg_size"] and r["blocks"] >= 1, (what, r)
        lds = w["lds"]
        if isinstance(lds, tuple) and lds[0] == "fastgen":
            _, nt, sd, one = lds
            assert 0 <= r["fg_top"] <= 512, (what, r)
            lds = nt * (128 + 4 * sd) + r["fg_top"] * 128
            lds = max(lds, 90000) if one else lds
        elif isinstance(lds, tuple) and lds[1] == 4:  # 64 B per inner node of the fast tree, two bit sets of a word per 32 spheres + 1, to 16 B
            n_inner, n_sph = len(api.fast_tree(world)[0]), world.counts()["spheres"]
            lds = 16 * 1024 * 8 + ((n_inner * 64 + 2 * ((n_sph + 31) // 32 + 1) * 4 + 15) & ~15)
        elif isinstance(lds, tuple):  # layout 3: the compact ops' number is the library's own; the rings, and room for the scene beside them
            assert 16 * 1024 * 8 < r["lds_bytes"] <= 160 * 1024, (what, r)
            lds = r["lds_bytes"]
        assert r["lds_bytes"] == lds, (what, r, lds)
        if w["samples"] is not None:
            assert (r["sample_begin"], r["sample_end"]) == w["samples"] and r["resume"] == w["resume"], (what, r)
            assert r["tile_order"] == w["tile_order"] and r["steal_state"] == w["steal_state"], (what, r)
        if "n_pixels" in w:
            assert r["n_pixels"] == w["n_pixels"], (what, r)
    if seen is not None:
        seen.update(k for k, _ in got)


@pytest.fixture(autouse=True)
def _switches(rl, request):
    rl.init(0)
    request.addfinalizer(lambda: _restore(rl.api))


def _sphere_world(rl):
    """12 spheres: ground, a 3 x 3 field of every material (two moving), a glass ball and a light."""
    api = rl.api
    tex = np.zeros(3, dtype=api.TEXTURE)
    tex["kind"] = api.TEX_SOLID
    tex["color"] = [(0.5, 0.5, 0.5), (0.7, 0.3, 0.3), (4.0, 4.0, 4.0)]
    mats = np.zeros(5, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 0
    mats[1]["kind"], mats[1]["texture"] = api.MAT_LAMBERTIAN, 1
    mats[2]["kind"], mats[2]["albedo"], mats[2]["fuzz"] = api.MAT_METAL, (0.8, 0.8, 0.8), 0.3
    mats[3]["kind"], mats[3]["ior"] = api.MAT_DIELECTRIC, 1.5
    mats[4]["kind"], mats[4]["texture"] = api.MAT_DIFFUSE_LIGHT, 2
    centers, center1, radii, material, moving = [(0.0, -100.0, 0.0)], [(0.0, -100.0, 0.0)], [100.0], [0], [0]
    for i in range(9):
        x, z = -1.6 + 1.6 * (i % 3), -1.2 + 1.2 * (i // 3)
        centers.append((x, 0.3, z)), radii.append(0.3), material.append(1 + i % 3), moving.append(int(i % 4 == 0))
        center1.append((x, 0.3 + (0.3 if i % 4 == 0 else 0.0), z))
    for c, r, m in [((0.0, 1.3, 0.0), 0.5, 3), ((1.8, 1.6, -0.8), 0.3, 4)]:
        centers.append(c), center1.append(c), radii.append(r), material.append(m), moving.append(0)
    sph = np.zeros(len(centers), dtype=api.SPHERE)
    sph["center0"], sph["center1"], sph["radius"], sph["material"], sph["moving"] = centers, center1, radii, material, moving
    assert len(sph) == 12
    return rl.World.from_spheres(sph, mats, tex, True)


def _general_world(rl, noise, media):
    def scene(b):
        grey = b.lambertian(b.solid((0.6, 0.6, 0.6)))
        wall = b.lambertian(b.noise(4.0, 7)) if noise else b.lambertian(b.solid((0.7, 0.3, 0.3)))
        objs = [b.quad((-3, 0, -3), (6, 0, 0), (0, 0, 6), grey), b.quad((-3, 0, -3), (6, 0, 0), (0, 4, 0), wall),
                b.quad((-1, 3.5, -1), (2, 0, 0), (0, 0, 2), b.diffuse_light(b.solid((4.0, 4.0, 4.0)))),
                b.triangle((-2.2, 0, 0.5), (1.5, 0, 0), (0, 1.8, 0), b.metal((0.8, 0.8, 0.8), 0.1))]
        if media:
            flat, (x0, y0, z0), (dx, dy, dz) = b.flat(), (0.2, 0.0, -1.0), (1.6, 1.6, 1.6)
            box = [b.quad((x0, y0, z0), (dx, 0, 0), (0, dy, 0), flat), b.quad((x0, y0, z0 + dz), (dx, 0, 0), (0, dy, 0), flat),
                   b.quad((x0, y0, z0), (0, dy, 0), (0, 0, dz), flat), b.quad((x0 + dx, y0, z0), (0, dy, 0), (0, 0, dz), flat),
                   b.quad((x0, y0, z0), (dx, 0, 0), (0, 0, dz), flat), b.quad((x0, y0 + dy, z0), (dx, 0, 0), (0, 0, dz), flat)]
            return b.list([b.bvh(objs), b.constant_medium(b.list(box), 0.8, b.isotropic(b.solid((0.9, 0.9, 0.9))))])
        return b.bvh(objs)
    return rl.World.build(scene)


_cache = {}


def _scene(rl, name):
    """World, camera, the 40 listed pixels, and the yardstick: the counting frame and the counting moments (reference-order kernel, whatever
    the switches say).  Built once, with the switches at their defaults, and never written to afterwards."""
    if name not in _cache:
        _restore(rl.api)
        world = _sphere_world(rl) if name == "spheres" else _general_world(rl, "noise" in name, "media" in name)
        cam = rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=W, samples_per_pixel=SPP, max_depth=DEPTH, vfov=50.0, lookfrom=(0.0, 1.8, 6.0),
                                        lookat=(0.0, 1.0, 0.0), defocus_angle=0.3, focus_dist=6.0, background=(0.6, 0.7, 0.9), seed=5))
        assert (cam.c.image_width, cam.c.image_height) == (W, H)
        pick = np.random.default_rng(3).choice(np.setdiff1d(np.arange(W * H), [0, W - 1, W * (H - 1), W * H - 1]), 36, replace=False)
        pick = np.concatenate([[0, W - 1, W * (H - 1), W * H - 1], pick]).astype(np.uint32)
        ys, xs = np.divmod(pick, np.uint32(W))
        gs, ms = {}, {}
        frame = cam.render(world, stats=gs).data
        mom = cam.render_moments(world, stats=ms)
        for a in (frame, mom.sums, mom.sq):
            a.setflags(write=False)
        assert gs["flagged"] == 0 and ms["rays"] == gs["rays"] and _bits(mom.sums, frame)
        if name == "spheres":
            assert rl.api.fast_tree(world) is not None
        # the adaptive bound, from the yardstick alone: an eighth of the mean per-sample variance (largest channel).  A pixel stops at
        # checkpoint n when its variance of the mean, about its per-sample variance / n, is below it: from n = 8 on that is every pixel
        # of below-average variance, and the pixels of a constant colour (sky, light) stop at the first checkpoint.
        var = np.maximum((mom.sq - mom.sums * mom.sums / SPP) / (SPP - 1), 0.0).max(axis=-1)
        bound = float(var.mean()) / 8.0
        assert bound > 0.0 and np.isfinite(bound)
        _cache[name] = dict(name=name, world=world, cam=cam, xs=xs, ys=ys, frame=frame, rays=gs["rays"], mom=mom, bound=bound)
    return _cache[name]


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _device_call(rl, world, shapes, call):
    """A counter-free `_device` call into NaN- / 0xFF-filled buffers -> (host arrays, status)."""
    import torch
    dev = torch.device("cuda", 0)
    bufs = [torch.full(s, float("nan"), dtype=torch.float64, device=dev) if dt is np.float64 else torch.full(s, -1, dtype=torch.int32, device=dev) for s, dt in shapes]
    call(torch.cuda.current_stream(dev).cuda_stream, *[b.data_ptr() for b in bufs])
    st = rl.api.render_status(world)
    return [b.cpu().numpy() if dt is np.float64 else b.cpu().numpy().view(np.uint32) for b, (_, dt) in zip(bufs, shapes)], st


def _frame(rl, S, row_first=0, row_step=1):
    cam, world = S["cam"], S["world"]
    nrows = rl.api.rows_for(H, row_first, row_step)
    (out,), st = _device_call(rl, world, [((nrows, W, 3), np.float64)], lambda stream, d: cam.render_device(world, d, stream=stream, row_first=row_first, row_step=row_step))
    return out, st


def _indep(rl, S):
    cam, world = S["cam"], S["world"]
    (out,), st = _device_call(rl, world, [((H, W, 3), np.float64)], lambda stream, d: cam.render_independent_device(world, d, stream=stream))
    return out, st


def _moments(rl, S):
    cam, world = S["cam"], S["world"]
    (sums, sq), st = _device_call(rl, world, [((H, W, 3), np.float64)] * 2, lambda stream, d0, d1: cam.render_moments_device(world, d0, d1, stream=stream))
    return sums, sq, st


def _adaptive(rl, S):
    cam, world = S["cam"], S["world"]
    (sums, sq, counts), _ = _device_call(rl, world, [((H, W, 3), np.float64)] * 2 + [((H, W), np.uint32)],
                                         lambda stream, d0, d1, d2: cam.render_adaptive_device(world, MIN, EVERY, d0, d1, d2, abs_variance=S["bound"], stream=stream))
    return sums, sq, counts


def _check_frame_and_list(rl, S, what, log, seen, **sw):
    """The counter-free frame and list (with indep the calls that have a one-wave-per-SIMD form; on sphere worlds a cooperative form);
    sw: the switches as the caller set them, for _route."""
    api, cam, world, xs, ys, frame = rl.api, S["cam"], S["world"], S["xs"], S["ys"], S["frame"]
    out, st = _frame(rl, S)
    assert _bits(out, frame) and st["rays"] == S["rays"] and st["flagged"] == 0, (what, "frame")
    _assert_route(api, log.take(), _route(S["name"], "frame", False, **sw), (what, "frame"), world, seen)
    px = cam.render_pixels(world, xs, ys)
    assert _bits(px, frame[ys, xs]), (what, "pixels")
    _assert_route(api, log.take(), _route(S["name"], "pixels", False, **sw), (what, "pixels"), world, seen)
    return out, px


@pytest.mark.parametrize("name", WORLDS)
def test_every_entry_point_reaches_a_kernel_that_renders_the_reference_bits(rl, name):
    api = rl.api
    S = _scene(rl, name)
    cam, world, xs, ys, frame, mom = S["cam"], S["world"], S["xs"], S["ys"], S["frame"], S["mom"]
    log, seen = _Log(api), _names.setdefault(f"every[{name}]", set())

    def routed(entry, counting, what, **sw):
        _assert_route(api, log.take(), _route(name, entry, counting, **sw), (name, what), world, seen)

    # the yardsticks themselves (a cached scene made them earlier: made again here, they show their routes)
    gs0, ms0 = {}, {}
    assert _bits(cam.render(world, stats=gs0).data, frame) and gs0["rays"] == S["rays"]
    routed("frame", True, "counting frame")
    assert _bits(cam.render_moments(world, stats=ms0).sq, mom.sq)
    routed("moments", True, "counting moments")

    # 1, 2: the frame, counter-free == counting; 5: listed pixels == the frame's pixels (counter-free and counting)
    _check_frame_and_list(rl, S, name, log, seen)
    ps = {}
    assert _bits(cam.render_pixels(world, xs, ys, stats=ps), frame[ys, xs]) and ps["flagged"] == 0
    routed("pixels", True, "counting pixels")

    # 3, 4: sample-parallel, k = 1 == k = 3 == its own counting form
    frames = []
    for k in (1, 3):
        api.set_indep_k(k)
        fast, st = _indep(rl, S)
        routed("indep", False, ("indep", k))
        gs = {}
        counted = cam.render_independent_rows(world, 0, 1, stats=gs)
        routed("indep", True, ("counting indep", k))
        assert _bits(fast, counted) and st["rays"] == gs["rays"] and gs["flagged"] == 0, (name, k)
        frames.append((fast, gs["rays"]))
    api.set_indep_k(1)
    assert _bits(frames[0][0], frames[1][0]) and frames[0][1] == frames[1][1]

    # 6: moments sums == the frame, squares == their reference-order form; 7: the list's moments == the frame's at the listed pixels
    sums, sq, st = _moments(rl, S)
    routed("moments", False, "moments")
    assert _bits(sums, frame) and _bits(sq, mom.sq) and st["rays"] == S["rays"]
    psums, psq = cam.render_pixels_moments(world, xs, ys)
    routed("pixels_moments", False, "pixels moments")
    assert _bits(psums, frame[ys, xs]) and _bits(psq, mom.sq[ys, xs])
    api.set_fast_traversal(False)
    sums_ref, sq_ref, _ = _moments(rl, S)
    routed("moments", False, "moments, fast off", fast=False)
    psums_ref, psq_ref = cam.render_pixels_moments(world, xs, ys)
    routed("pixels_moments", False, "pixels moments, fast off", fast=False)
    api.set_fast_traversal(True)
    assert _bits(sums_ref, frame) and _bits(sq_ref, sq) and _bits(psums_ref, psums) and _bits(psq_ref, psq)

    # 8: adaptive counts, sums and squares == their reference-order form; the bound stops some pixels
    a_sums, a_sq, a_counts = _adaptive(rl, S)
    routed("adaptive", False, "adaptive")
    api.set_fast_traversal(False)
    r_sums, r_sq, r_counts = _adaptive(rl, S)
    routed("adaptive", False, "adaptive, fast off", fast=False)
    api.set_fast_traversal(True)
    assert _bits(a_counts, r_counts) and _bits(a_sums, r_sums) and _bits(a_sq, r_sq)
    print(name, "adaptive counts", dict(zip(*[v.tolist() for v in np.unique(a_counts, return_counts=True)])))
    assert (a_counts < SPP).any() and (a_counts >= MIN).all() and (a_counts <= SPP).all()
    full = a_counts == SPP
    assert _bits(a_sums[full], frame[full]) and _bits(a_sq[full], mom.sq[full])

    # 9: path-query colours of the 40 camera rays == their counting form, with the same out-cursors
    p = cam.params
    rays, cur = cam.get_rays(xs, ys, api.pack_cursors(xs.astype(np.uint64) * np.uint64(W) + ys.astype(np.uint64)))
    assert log.take() == []  # camera rays are no render launch
    rgb, out_cur, counts = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays)
    assert api.last_query()["kernel"] == "fast"
    routed("rays", False, "rays")
    qs = {}
    rgb_c, out_cur_c, counts_c = world.ray_color_rays(None, None, None, cur, p.seed, p.max_depth, p.background, rays=rays, stats=qs)
    assert api.last_query()["kernel"] == "reference"
    routed("rays", True, "counting rays")
    assert _bits(rgb, rgb_c) and _bits(out_cur, out_cur_c) and np.array_equal(counts, counts_c) and qs["rays"] == int(counts.sum()) and qs["flagged"] == 0


@pytest.mark.parametrize("one_wave", [1, 0])
def test_both_forms_of_the_media_and_noise_flavour(rl, one_wave):
    """The flavour with both the media and the transcendental code: forced into / out of its one-wave-per-SIMD form (frame, indep, pixels)."""
    api = rl.api
    S = _scene(rl, "media_noise")
    log, seen = _Log(api), _names.setdefault(f"one_wave[{one_wave}]", set())
    api.set_fastg_one_wave(one_wave)
    _check_frame_and_list(rl, S, one_wave, log, seen, one_wave=one_wave)
    fast, st = _indep(rl, S)
    _assert_route(api, log.take(), _route("media_noise", "indep", False, one_wave=one_wave), (one_wave, "indep"), S["world"], seen)
    gs = {}
    assert _bits(fast, S["cam"].render_independent_rows(S["world"], 0, 1, stats=gs)) and st["rays"] == gs["rays"]
    _assert_route(api, log.take(), _route("media_noise", "indep", True, one_wave=one_wave), (one_wave, "counting indep"), S["world"], seen)
    fastgen = sorted(k for k in seen if k.startswith("rtiow_fast_general"))
    assert len(fastgen) == 3 and all(("<256, 40, true, true>" in k) == bool(one_wave) for k in fastgen), fastgen


@pytest.mark.parametrize("coop", [False, True])
def test_sphere_world_through_the_cooperative_and_the_wave_kernel(rl, coop):
    """Frame and list with and without the cooperative kernel, and a row shard of 24 x 8.  Without the cooperative kernel the frame and
    the shard run the fast layout of the wave kernel, and the resumed launch of each — 384 and 192 pixels against 3 x CUs x 1024 — is the
    stealing instantiation rtiow_wave_kernel<1024, 4, false, true>; the list, which has no wave-kernel form, takes the reference-order
    kernel.  With it, frame, shard and list all run the cooperative kernel, and nothing steals."""
    api = rl.api
    S = _scene(rl, "spheres")
    log, seen = _Log(api), _names.setdefault(f"spheres[coop={coop}]", set())
    api.set_coop(coop)
    _check_frame_and_list(rl, S, coop, log, seen, coop=coop)
    api.set_steal(3.0)
    shard, st = _frame(rl, S, 1, 2)
    recs = log.take()
    _assert_route(api, recs, _route("spheres", "frame", False, npix=W * (H // 2), coop=coop), (coop, "shard"), S["world"], seen)
    if coop:
        assert [r["kernel"] for r in recs] == ["rtiow_coop_kernel<4, true, 256>"] * 2 and not any(r["steal_state"] for r in recs)
    else:
        assert [r["kernel"] for r in recs] == ["rtiow_wave_kernel<1024, 4, false, false>", "rtiow_wave_kernel<1024, 4, false, true>"]
        assert [r["steal_state"] for r in recs] == [False, True]
        state, n = api.steal_record(S["world"], W * (H // 2))
        assert (state == 3).all() and ((n == api.NEVER_OFFERED) | ((n >= LPT_FIRST) & (n < SPP))).all()
    gs = {}
    assert _bits(shard, S["cam"].render_rows(S["world"], 1, 2, stats=gs)) and st["rays"] == gs["rays"]
    _assert_route(api, log.take(), _route("spheres", "frame", True, npix=W * (H // 2)), (coop, "counting shard"), S["world"], seen)
    assert _bits(shard, S["frame"][1::2])


CASES = [f"every[{n}]" for n in WORLDS] + ["one_wave[1]", "one_wave[0]", "spheres[coop=False]", "spheres[coop=True]"]


def test_the_names_are_those_of_the_recorded_trace():
    """profiles/rtiow_launch_tables.txt §3 lists every instantiation the nine cases above launched under rocprofv3 --kernel-trace, at the
    commit that introduced the tables.  The log must name the same set: a kernel the trace has and the log lacks is a launch that went
    elsewhere (or past the log), one the log has and the trace lacks is a row that changed.  (Run alone, with no case before it, the test
    has nothing to compare; after a part of the cases, what they launched must at least be in the trace.)"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "rtiow_launch_tables.txt")
    text = open(path).read()
    section = text[text.index("\n3. Routing"):text.index("\n4. Speed")]
    traced = set(re.findall(r"^\s+\d+\s+rl::(rtiow_(?:coop|fast_general|wave)\w*<[^>]*>)\s+grid", section, re.M))
    assert len(traced) == 66 and "rtiow_wave_kernel<1024, 4, false, true>" in traced
    logged = set().union(*[_names.get(c, set()) for c in CASES])
    assert logged <= traced, sorted(logged - traced)
    if all(c in _names for c in CASES):
        assert logged == traced, sorted(traced - logged)


# ----------------------------------------------------------------------------- thresholds, both sides of each
# 1 spp and depth 2 unless the rule is about them: a frame costs milliseconds.  Each side asserts its route from the log, and that 40 of
# its pixels are the counting list render's (rtiow_wave_general_pixels_kernel, the reference order).
def _set(api, coop=True, fast=True, lpt=True, steal=3.0, one_wave=-1):
    api.set_coop(coop), api.set_fast_traversal(fast), api.set_lpt(lpt), api.set_steal(steal), api.set_fastg_one_wave(one_wave)
    return dict(coop=coop, fast=fast, lpt=lpt, steal=steal, one_wave=one_wave)


def _camera(rl, w, h, spp, depth):
    cam = rl.Camera(rl.CameraParams(aspect_ratio=w / (h + 0.5), image_width=w, samples_per_pixel=spp, max_depth=depth, vfov=50.0, lookfrom=(0.0, 1.8, 6.0),
                                    lookat=(0.0, 1.0, 0.0), defocus_angle=0.3, focus_dist=6.0, background=(0.6, 0.7, 0.9), seed=5))
    assert (cam.c.image_width, cam.c.image_height) == (w, h)
    return cam


def _forty(w, h):
    pick = np.random.default_rng(3).choice(np.setdiff1d(np.arange(w * h), [0, w - 1, w * (h - 1), w * h - 1]), 36, replace=False)
    ys, xs = np.divmod(np.concatenate([[0, w - 1, w * (h - 1), w * h - 1], pick]).astype(np.uint32), np.uint32(w))
    return xs, ys


def _frame_side(rl, name, w, h, spp, depth, kernels, **switches):
    """A counter-free w x h frame of world `name` under the switches: its launches are _route's and are named `kernels`."""
    import torch
    api, world = rl.api, _scene(rl, name)["world"]
    sw = _set(api, **switches)
    cam = _camera(rl, w, h, spp, depth)
    log = _Log(api)
    dev = torch.device("cuda", 0)
    buf = torch.full((h, w, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    st = api.render_status(world)
    recs = log.take()
    print(name, w, h, spp, depth, switches, [(r["kernel"], r["blocks"], r["lds_bytes"], r["sample_begin"], r["sample_end"]) for r in recs])
    _assert_route(api, recs, _route(name, "frame", False, npix=w * h, spp=spp, depth=depth, **sw), (name, w, h, spp, depth), world)
    assert [r["kernel"] for r in recs] == kernels
    xs, ys = _forty(w, h)
    ps = {}
    counting = cam.render_pixels(world, xs, ys, stats=ps)
    assert [r["kernel"] for r in log.take()] == [f"rtiow_wave_general_pixels_kernel<512, {_b('noise' in name)}, true, {_b('media' in name)}>"]
    assert _bits(buf.cpu().numpy()[ys, xs], counting) and st["flagged"] == 0 and ps["flagged"] == 0
    return recs


def _list_side(rl, name, w, h, n, depth, kernel, **switches):
    """A counter-free list of the first n pixels of a fixed shuffle of the w x h frame (1 spp): one launch of `kernel`, as _route says."""
    api, world = rl.api, _scene(rl, name)["world"]
    sw = _set(api, **switches)
    cam = _camera(rl, w, h, 1, depth)
    ys, xs = np.divmod(np.random.default_rng(9).permutation(w * h)[:n].astype(np.uint32), np.uint32(w))
    assert len(xs) == n
    log = _Log(api)
    px = cam.render_pixels(world, xs, ys)
    recs = log.take()
    print(name, w, h, n, depth, switches, [(r["kernel"], r["blocks"], r["n_pixels"]) for r in recs])
    _assert_route(api, recs, _route(name, "pixels", False, n_list=n, spp=1, depth=depth, **sw), (name, "list", n, depth), world)
    assert [r["kernel"] for r in recs] == [kernel]
    forty = np.linspace(0, n - 1, 40).astype(int)
    assert _bits(px[forty], cam.render_pixels(world, xs[forty], ys[forty], stats={}))


def test_cooperative_small_frame_rule_both_sides(rl):
    """Counter-free sphere frames of at most 160 pixels per CU take the cooperative kernel; one row more, the wave kernel's fast layout."""
    cus = _cus()
    _frame_side(rl, "spheres", 160, cus, 1, 2, ["rtiow_coop_kernel<4, false, 1024>"])
    _frame_side(rl, "spheres", 160, cus + 1, 1, 2, ["rtiow_wave_kernel<1024, 4, false, false>"])


def test_cooperative_register_mode_both_sides(rl):
    """Up to 8 pixels per CU every pixel has a wave at once and the boxes live in registers; one pixel more, they are read from L2."""
    cus = _cus()
    h = (cus * 8 + 1 + 63) // 64 + 1
    _list_side(rl, "spheres", 64, h, cus * 8, 2, "rtiow_coop_pixels_kernel<4, true, 256>")
    _list_side(rl, "spheres", 64, h, cus * 8 + 1, 2, "rtiow_coop_pixels_kernel<4, false, 1024>")
    _frame_side(rl, "spheres", 64, cus // 8, 1, 2, ["rtiow_coop_kernel<4, true, 256>"])
    _frame_side(rl, "spheres", 64, cus // 8 + 1, 1, 2, ["rtiow_coop_kernel<4, false, 1024>"])


def test_one_wave_rule_of_the_media_and_noise_flavour_both_sides(rl):
    """Up to 1536 pixels per CU the flavour with both code paths runs as one wave per SIMD; above, in the 512-lane form."""
    cus = _cus()
    _frame_side(rl, "media_noise", 1536, cus, 1, 2, ["rtiow_fast_general_kernel<256, 40, true, true>"])
    _frame_side(rl, "media_noise", 1536, cus + 1, 1, 2, ["rtiow_fast_general_kernel<512, 40, true, true>"])


def test_steal_rule_both_sides(rl):
    """The resumed launch steals while npix <= fill x CUs x 1024: the 24 x 16 frame with the fill that makes this an equality, and with
    the next smaller double."""
    cus, npix = _cus(), W * H
    inside = npix / (cus * 1024.0)
    while inside * float(cus) * 1024.0 < float(npix):
        inside = float(np.nextafter(inside, np.inf))
    outside = float(np.nextafter(inside, 0.0))
    while outside * float(cus) * 1024.0 >= float(npix):
        outside = float(np.nextafter(outside, 0.0))
    plain, stealing = "rtiow_wave_kernel<1024, 4, false, false>", "rtiow_wave_kernel<1024, 4, false, true>"
    recs = _frame_side(rl, "spheres", W, H, 64, DEPTH, [plain, stealing], coop=False, steal=inside)
    assert [r["steal_state"] for r in recs] == [False, True]
    recs = _frame_side(rl, "spheres", W, H, 64, DEPTH, [plain, plain], coop=False, steal=outside)
    assert [r["steal_state"] for r in recs] == [False, False]


@pytest.mark.parametrize("name,kernel,switches", [("spheres", "rtiow_wave_kernel<1024, 4, false, false>", dict(coop=False, steal=0.0)),
                                                  ("spheres", "rtiow_coop_kernel<4, true, 256>", {}),
                                                  ("quads", "rtiow_fast_general_kernel<768, 20, false, false>", {})], ids=["wave", "coop", "fastgen"])
def test_two_launch_rule_both_sides(rl, name, kernel, switches):
    """63 samples: one launch over [0, 63); 64: the probe launch [0, 8), then [8, 64) resumed in the sorted tile order."""
    recs = _frame_side(rl, name, W, H, 63, DEPTH, [kernel], **switches)
    assert [(r["sample_begin"], r["sample_end"], r["resume"], r["tile_order"]) for r in recs] == [(0, 63, 0, False)]
    recs = _frame_side(rl, name, W, H, 64, DEPTH, [kernel, kernel], **switches)
    assert [(r["sample_begin"], r["sample_end"], r["resume"], r["tile_order"]) for r in recs] == [(0, 8, 0, False), (8, 64, 1, True)]


def test_depth_rule_both_sides(rl):
    """The fast layout keeps the remaining depth in 22 bits: max_depth = 2^22 - 1 still runs layout 4 (and a list the cooperative kernel),
    2^22 the next layout that fits (guarded compact ops; the list the reference-order kernel)."""
    _frame_side(rl, "spheres", W, H, 1, FAST_DEPTH_MASK, ["rtiow_wave_kernel<1024, 4, false, false>"], coop=False)
    _frame_side(rl, "spheres", W, H, 1, FAST_DEPTH_MASK + 1, ["rtiow_wave_kernel<1024, 3, false, false>"], coop=False)
    _list_side(rl, "spheres", W, H, 40, FAST_DEPTH_MASK, "rtiow_coop_pixels_kernel<4, true, 256>")
    _list_side(rl, "spheres", W, H, 40, FAST_DEPTH_MASK + 1, "rtiow_wave_general_pixels_kernel<512, false, false, false>")
