"""GPU tier: the fast sphere walk on centre / half-extent boxes (csrc/rl_fast_bvh.cpp fast_node_ch, the TRAV step of
csrc/rl_rtiow_wave_body.inc).  The boxes only ever reject and the walk's answer does not depend on the visiting order, so the
counter-free frame must equal the reference-order frame (`stats=`) of the same call bit for bit, with the same ray and panic-site
counts, in the worlds where the new form's rounding is largest against the boxes: coordinates scaled by 1e-3 and 1e3, radius-0.01
spheres at coordinates around 1e4 (|c| / h near 1e6), a camera that looks along an axis to within 1e-6, a camera at the frame's reach,
coincident spheres, and a tree of the full depth (14 levels of inner nodes).  64 x 48 pixels, 4 samples, depth 8; one case at 64
samples so that the probe launch and the cost-sorted resume launch both run.  `slow_traces` is printed, not asserted."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _structures(rl, world):
    out = (C.c_uint64 * 16)()
    L = rl.api.render_lib()
    assert L.rl_debug_host_structures(world.desc, out) == 0, L.rl_last_error().decode()
    return list(out)


def _timed(rl, cam, world):
    import torch
    dev = torch.device("cuda", 0)
    buf = torch.full((cam.c.image_height, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    cam.render_device(world, buf.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
    st = rl.api.render_status(world)
    return buf.cpu().numpy(), st


def _check(rl, world, p, depth=None):
    s = _structures(rl, world)
    assert s[0] & 1  # the world is one the fast traversal takes
    if depth is not None:
        assert s[13] == depth
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (64, 48)
    try:
        rl.api.set_coop(False)
        rl.api.set_rtiow_variant(1029)  # the wave-scheduled fast kernel, not the cooperative small-frame one
        timed, st = _timed(rl, cam, world)
    finally:
        rl.api.set_rtiow_variant(0)
        rl.api.set_coop(True)
    gs = {}
    counting = cam.render(world, stats=gs).data
    print(f"rays {gs['rays']} flagged {gs['flagged']} / {st['flagged']} slow_traces {st['slow_traces']}")
    assert np.array_equal(timed.view(np.uint64), counting.view(np.uint64))
    assert st["rays"] == gs["rays"] and st["flagged"] == gs["flagged"]
    assert gs["rays"] > cam.c.image_width * cam.c.image_height * p.samples_per_pixel  # some rays scatter


def _materials(b, rng):
    return [b.lambertian(b.solid(tuple(rng.uniform(0.2, 0.9, 3)))), b.metal((0.8, 0.8, 0.9), float(rng.uniform(0, 0.5))), b.dielectric(1.5)][rng.integers(0, 3)]


def _cloud(rl, seed, n, scale, at=0.0, rmin=0.15, rmax=0.6, moving=True):
    """n spheres of radius [rmin, rmax] * scale in a slab of 8 x 2 x 8 * scale around (at, at, at), every fourth one moving."""
    rng = np.random.default_rng(seed)

    def build(b):
        items = []
        for i in range(n):
            c = np.array([at + scale * rng.uniform(-4, 4), at + scale * rng.uniform(-1, 1), at + scale * rng.uniform(-4, 4)])
            r = float(scale * rng.uniform(rmin, rmax))
            if moving and i % 4 == 3:
                items.append(b.sphere(tuple(c), r, _materials(b, rng), center2=tuple(c + scale * rng.uniform(-0.2, 0.2, 3))))
            else:
                items.append(b.sphere(tuple(c), r, _materials(b, rng)))
        return b.bvh(items)

    return rl.World.build(build)


def _params(rl, scale=1.0, at=0.0, spp=4, lookfrom=(0.5, 1.0, 9.0), lookat=(0.0, 0.0, 0.0), seed=5):
    lf = tuple(at + scale * v for v in lookfrom)
    la = tuple(at + scale * v for v in lookat)
    return rl.CameraParams(aspect_ratio=4.0 / 3.0, image_width=64, samples_per_pixel=spp, max_depth=8, vfov=50.0, lookfrom=lf, lookat=la,
                           background=(0.7, 0.8, 1.0), seed=seed)


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_scaled_worlds(rl, scale):
    _check(rl, _cloud(rl, 21, 60, scale), _params(rl, scale))


def test_small_spheres_far_from_the_origin(rl):
    """Radius 0.01 at coordinates around 1e4: a leaf box's half-extent is 1e-6 of its centre, the case in which the centre's rounding in
    the step is largest against the box."""
    _check(rl, _cloud(rl, 22, 60, 0.02, at=1e4, rmin=0.5, rmax=0.5, moving=False), _params(rl, 0.02, at=1e4))


def test_camera_along_an_axis(rl):
    """The central rays have two direction components 1e-6 of the third: |1/d| spans six decades across the axes."""
    _check(rl, _cloud(rl, 23, 60, 1.0), _params(rl, lookfrom=(0.0, 0.0, 9.0), lookat=(9e-6, 9e-6, 0.0)))


def _frame(spheres):
    """centre and reach of the frame of a world of stationary spheres (rl_fast_bvh.cpp guard_frame)"""
    lo = np.min([np.array(c) - r for c, r in spheres], axis=0)
    hi = np.max([np.array(c) + r for c, r in spheres], axis=0)
    return 0.5 * (lo + hi), 2.0 * 0.5 * float(np.sqrt(((hi - lo) ** 2).sum())) + 1.0


def test_camera_at_reach(rl):
    """The farthest camera the guarded boxes are valid for: origins at the frame's bound."""
    rng = np.random.default_rng(24)
    spheres = [((float(rng.uniform(-4, 4)), float(rng.uniform(-1, 1)), float(rng.uniform(-4, 4))), float(rng.uniform(0.15, 0.6))) for _ in range(60)]

    def build(b):
        return b.bvh([b.sphere(c, r, _materials(b, rng)) for c, r in spheres])

    centre, reach = _frame(spheres)
    d = np.array([0.6, 0.3, 0.74])
    lookfrom = centre + d / np.linalg.norm(d) * reach * (1.0 - 1e-9)
    p = rl.CameraParams(aspect_ratio=4.0 / 3.0, image_width=64, samples_per_pixel=4, max_depth=8, vfov=18.0, lookfrom=tuple(lookfrom), lookat=tuple(centre),
                        background=(0.7, 0.8, 1.0), seed=6)
    _check(rl, rl.World.build(build), p)


def test_coincident_spheres(rl):
    """Pairs of spheres with the same centre and radius: equal boxes (tA == tB), equal roots (ties go to the reference's own fold)."""
    rng = np.random.default_rng(25)

    def build(b):
        items = []
        for _ in range(20):
            c, r = (float(rng.uniform(-3, 3)), float(rng.uniform(-1, 1)), float(rng.uniform(-3, 3))), float(rng.uniform(0.3, 0.8))
            items += [b.sphere(c, r, _materials(b, rng)), b.sphere(c, r, _materials(b, rng))]
        return b.bvh(items)

    _check(rl, rl.World.build(build), _params(rl))


def _deep_world(rl):
    """400 spheres whose distances from the origin are log-uniform over [0.5, 100] and whose radii grow with the distance: the surface-area
    heuristic keeps splitting the far, large ones off the dense core until the depth cap (FAST_MAX_DEPTH = 14 levels of inner nodes) takes over."""
    rng = np.random.default_rng(3)

    def build(b):
        m = b.lambertian(b.solid((0.6, 0.5, 0.4)))
        items = []
        for _ in range(400):
            dist = 0.5 * 200.0 ** rng.uniform()
            v = rng.normal(size=3)
            items.append(b.sphere(tuple(v / np.linalg.norm(v) * dist), float(0.08 * dist), m))
        return b.bvh(items)

    return rl.World.build(build)


def test_tree_of_full_depth(rl):
    """14 levels of inner nodes above a leaf (the structure report counts the leaf: 15): the per-lane stack is used to its last entry."""
    _check(rl, _deep_world(rl), _params(rl, lookfrom=(1.0, 2.0, 30.0), lookat=(0.0, 0.0, 0.0)), depth=15)


def test_probe_and_resume_launches(rl):
    """64 samples: the probe launch, then the cost-sorted launch that resumes every pixel."""
    _check(rl, _cloud(rl, 26, 60, 1.0), _params(rl, spp=64))
