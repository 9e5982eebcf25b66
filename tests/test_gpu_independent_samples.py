"""GPU tier (-m gpu): sample-parallel rendering with independent sample streams (rl_rtiow_render_independent_rows / _device).

Every sample s of the mode is what the reference renders as the FIRST sample of a render from sample s (render_from_checkpoint of a
canvas with `samples = s`, camera.rs:136-174): the existing chained render of ONE sample per pixel from first_sample = s.  So the mode's
frame must equal, bit for bit, the left-to-right f64 fold from zeros of those single-sample chained frames — on every kernel flavour
the automatic choice reaches (counting renders: the reference-order wave kernel; counter-free: the fast traversals), for every split
of the work (calls, passes, claims, row shards)."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
TOL = 1e-4


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_indep_cap(0)
    rl.api.set_indep_k(1)


def _synthetic_image():
    y, x = np.mgrid[0:12, 0:20]
    return np.stack([(x * 13) % 256, (y * 21) % 256, ((x + y) * 7) % 256], axis=-1).astype(np.uint8)


def _scene(rl, golden, name):
    """(world, camera params) at a small frame; 48 - 64 px wide."""
    if name == "golden_test_scene":
        w = rl.World.golden_test_scene()
    elif name == "bouncing_spheres":
        w = rl.World.bouncing_spheres(1)
    elif name == "perlin_spheres":
        w = rl.World.perlin_spheres()
    elif name == "earth_scene":
        w = rl.World.earth_scene(_synthetic_image())
    elif name == "teapot":
        w = rl.World.example_scene("teapot", obj_text=golden("teapot-low.obj"))
    else:
        w = rl.World.example_scene(name)
    p = w.params
    p.image_width = 48 if name in ("cornell_smoke", "teapot") else 64
    p.max_depth = min(p.max_depth, 20)
    return w, p


SCENES = ["golden_test_scene", "bouncing_spheres", "checkered_spheres", "quads", "flat_world", "cornell_box", "cornell_smoke",
          "perlin_spheres", "earth_scene", "teapot"]


def _cam(rl, p, spp):
    return rl.Camera(dataclasses.replace(p, samples_per_pixel=spp))


def _chained(rl, world, p, F, S, row_first=0, row_step=1):
    """Left-to-right fold from zeros of the chained single-sample counting renders of samples F .. F+S-1, and their summed counters."""
    cam1 = _cam(rl, p, 1)
    acc, tot = None, dict.fromkeys(COUNTERS, 0)
    for s in range(F, F + S):
        st = {}
        frame = cam1._render(s, world, row_first, row_step, stats=st, allow_degenerate=True)
        acc = (np.zeros_like(frame) if acc is None else acc) + frame
        for k in COUNTERS:
            tot[k] += st[k]
    return acc, tot


def _device(rl, cam, world, **kw):
    import torch
    nrows = rl.api.rows_for(cam.c.image_height, kw.get("row_first", 0), kw.get("row_step", 1))
    buf = torch.zeros((nrows, cam.c.image_width, 3), dtype=torch.float64, device="cuda:0")
    if "init" in kw:
        buf.copy_(torch.from_numpy(kw.pop("init")))
    cam.render_independent_device(world, buf.data_ptr(), stream=torch.cuda.current_stream().cuda_stream, **kw)
    st = rl.api.render_status(world, allow_degenerate=True)
    return buf.cpu().numpy(), st


@pytest.mark.parametrize("i,name", list(enumerate(SCENES)))
def test_independent_frame_is_the_fold_of_chained_single_sample_renders(rl, golden, i, name):
    """1 + 2 + 3: composition bit for bit on the counting and the counter-free path, counters = the sums of the chained renders,
    and the counter-free frame / ray count = the counting one."""
    world, p = _scene(rl, golden, name)
    F, S = (0, 8) if i % 2 == 0 else (5, 12)
    ref, tot = _chained(rl, world, p, F, S)
    cam = _cam(rl, p, S)
    gs = {}
    counted = cam.render_independent_rows(world, 0, 1, first_sample=F, stats=gs, allow_degenerate=True)
    assert np.array_equal(counted, ref), (name, np.abs(counted - ref).max())
    for k in COUNTERS:
        assert gs[k] == tot[k], (name, k, gs[k], tot[k])
    assert gs["rc"] == (rl.api.RL_E_DEGENERATE if tot["flagged"] else rl.api.RL_OK)
    fast, st = _device(rl, cam, world, first_sample=F)
    assert np.array_equal(fast, ref), (name, np.abs(fast - ref).max())
    assert st["rays"] == gs["rays"] and st["flagged"] == gs["flagged"], (name, st, gs["rays"])


def test_independent_frame_does_not_depend_on_the_split(rl):
    """4: one call = a + (S - a) samples with accumulate = several passes (shrunk buffer cap) = other claim sizes = three row shards."""
    world, p = rl.World.bouncing_spheres(1), None
    p = world.params
    p.image_width, p.max_depth = 64, 20
    F, S, a = 3, 12, 5
    cam = _cam(rl, p, S)
    one, _ = _device(rl, cam, world, first_sample=F)
    ref, _ = _chained(rl, world, p, F, S)
    assert np.array_equal(one, ref)
    first, _ = _device(rl, _cam(rl, p, a), world, first_sample=F)
    two, _ = _device(rl, _cam(rl, p, S - a), world, first_sample=F + a, accumulate=True, init=first)
    assert np.array_equal(two, one)
    # the same through the host-buffer entry (counting kernel)
    h = cam.render_independent_rows(world, 0, 1, first_sample=F)
    h2 = _cam(rl, p, a).render_independent_rows(world, 0, 1, first_sample=F)
    _cam(rl, p, S - a).render_independent_rows(world, 0, 1, first_sample=F + a, accumulate=True, out=h2)
    assert np.array_equal(h, one) and np.array_equal(h2, one)
    try:
        per_sample = cam.c.image_height * cam.c.image_width * 3 * 8
        rl.api.set_indep_cap(per_sample * 4)  # 4 samples per pass: 3 passes
        passes, _ = _device(rl, cam, world, first_sample=F)
        rl.api.set_indep_cap(per_sample * 5)  # 5 + 5 + 2, with 3 samples per claim (groups cut at the pass end)
        rl.api.set_indep_k(3)
        passes_k, _ = _device(rl, cam, world, first_sample=F)
        hp = cam.render_independent_rows(world, 0, 1, first_sample=F)
    finally:
        rl.api.set_indep_cap(0)
        rl.api.set_indep_k(1)
    assert np.array_equal(passes, one) and np.array_equal(passes_k, one) and np.array_equal(hp, one)
    shards = np.zeros_like(one)
    for g in range(3):
        part, _ = _device(rl, cam, world, row_first=g, row_step=3, first_sample=F)
        shards[g::3] = part
    assert np.array_equal(shards, one)


def test_independent_small_frames(rl):
    """5: an 8x8 frame at 512 spp and a 1x1 frame (far fewer pixels than lanes) match the composition."""
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.aspect_ratio, p.max_depth = 1.0, 20
    for width, S in ((8, 512), (1, 64)):
        p.image_width = width
        cam = _cam(rl, p, S)
        assert (cam.c.image_width, cam.c.image_height) == (width, width)
        ref, tot = _chained(rl, world, p, 0, S)
        fast, st = _device(rl, cam, world)
        assert np.array_equal(fast, ref), (width, np.abs(fast - ref).max())
        assert st["rays"] == tot["rays"]


def test_independent_two_rows_against_the_oracle(rl, oracle):
    """6: two rows of bouncing_spheres against the CPU oracle's single-sample renders, summed left to right."""
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.max_depth = 96, 50
    F, S = 2, 6
    cam = _cam(rl, p, S)
    H = cam.c.image_height
    row_first, row_step = 7, H // 2
    assert rl.api.rows_for(H, row_first, row_step) == 2
    gs = {}
    gpu = cam.render_independent_rows(world, row_first, row_step, first_sample=F, stats=gs)
    cam1 = _cam(rl, p, 1)
    cpu, tot = None, dict.fromkeys(COUNTERS, 0)
    for s in range(F, F + S):
        cs = {}
        frame = oracle.rtiow_render(world.desc, cam1.c, first_sample=s, row_first=row_first, row_step=row_step, stats=cs)
        cpu = (np.zeros_like(frame) if cpu is None else cpu) + frame
        for k in COUNTERS:
            tot[k] += cs[k]
    for k in COUNTERS:
        assert gs[k] == tot[k], (k, gs[k], tot[k])
    assert gpu.shape == cpu.shape
    assert np.abs(gpu - cpu).max() / S <= TOL
    assert np.abs(gpu - cpu).max() <= 1e-9 * max(1.0, np.abs(cpu).max())


def _degenerate_worlds(rl):
    api = rl.api
    tex = np.zeros(1, dtype=api.TEXTURE)
    tex[0]["kind"], tex[0]["color"] = api.TEX_SOLID, (0.5, 0.4, 0.3)
    mats = np.zeros(3, dtype=api.MATERIAL)
    mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 0
    mats[1]["kind"], mats[1]["ior"] = api.MAT_DIELECTRIC, 1.5
    mats[2]["kind"], mats[2]["albedo"], mats[2]["fuzz"] = api.MAT_METAL, (0.9, 0.9, 0.9), 0.0
    # test_gpu_edge_cases.py::test_degenerate_inputs_reach_the_reference_panic_sites_as_flags: a sphere of radius 0
    sph = np.zeros(2, dtype=api.SPHERE)
    sph["center0"] = [(0, 0, -1), (0.6, 0, -1)]
    sph["radius"] = [0.5, 0.0]
    sph["material"] = [0, 0]
    yield (rl.World.from_spheres(sph, mats, tex, False),
           rl.CameraParams(aspect_ratio=1.0, image_width=32, samples_per_pixel=2, max_depth=4, lookfrom=(0, 0, 1), lookat=(0, 0, -1)))
    # test_gpu_timed_kernels.py::test_async_render_surfaces_reference_panic_sites: a unit sphere at x = 1e12 trips vec3.rs:219 thousands of times
    sph = np.zeros(1, dtype=api.SPHERE)
    sph[0]["center0"], sph[0]["radius"] = (1e12, 0.0, -1.0), 1.0
    yield (rl.World.from_spheres(sph, mats[:1], tex, False),
           rl.CameraParams(aspect_ratio=1.0, image_width=33, samples_per_pixel=16, max_depth=5, lookfrom=(1e12, 0, 3), lookat=(1e12, 0, -1), vfov=40.0))


def test_independent_degenerate_input_is_flagged(rl):
    """7: reached panic sites: RL_E_DEGENERATE (also from the asynchronous entry's status), and flagged = the chained renders' sum."""
    api = rl.api
    S = 6
    flagged_any = 0
    for world, p in _degenerate_worlds(rl):
        ref, tot = _chained(rl, world, p, 0, S)
        cam = _cam(rl, p, S)
        gs = {}
        out = cam.render_independent_rows(world, 0, 1, stats=gs, allow_degenerate=True)
        for k in COUNTERS:
            assert gs[k] == tot[k], (k, gs[k], tot[k])
        assert gs["rc"] == (api.RL_E_DEGENERATE if tot["flagged"] else api.RL_OK)
        fin = np.isfinite(ref)
        assert np.array_equal(np.isfinite(out), fin) and np.array_equal(out[fin], ref[fin])
        fast, st = _device(rl, cam, world)
        assert st["flagged"] == tot["flagged"] and st["rc"] == gs["rc"]
        assert np.array_equal(np.isfinite(fast), fin) and np.array_equal(fast[fin], ref[fin])
        if tot["flagged"]:
            with pytest.raises(rl.RLError) as e:
                cam.render_independent(world)
            assert e.value.code == api.RL_E_DEGENERATE
        flagged_any += tot["flagged"]
    assert flagged_any > 1000


def test_independent_from_checkpoint_through_the_cpp_mirror(rl):
    """8: rtiow::Camera::render_independent_from_checkpoint (host/host_render.cpp) = Camera.render_independent(checkpoint=...)."""
    import ctypes as C
    world = rl.World.golden_test_scene()
    p = world.params
    p.image_width = 48
    ckpt = _cam(rl, p, 3).render(world)
    c = _cam(rl, p, 7).render_independent(world, checkpoint=ckpt)
    assert c.samples == 10
    ref, _ = _chained(rl, world, p, 3, 7)
    # the fold continues from the checkpoint's sums: ((ckpt + c_3) + c_4) + ...
    acc = ckpt.data.copy()
    cam1 = _cam(rl, p, 1)
    for s in range(3, 10):
        acc = acc + cam1._render(s, world)
    assert np.array_equal(c.data, acc)
    L = rl.api.host_lib()
    L.rlh_rtiow_golden_independent.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint64]
    data = np.ascontiguousarray(ckpt.data, dtype=np.float64).copy()
    assert L.rlh_rtiow_golden_independent(48, 7, 3, data.ctypes.data, data.size) == 0, L.rlh_last_error()
    assert np.array_equal(data.reshape(c.data.shape), c.data)


def _flavour(rl, name):
    """(world, camera params, one-wave switch) of each kernel flavour the sample-parallel mode reaches besides the sphere kernel."""
    if name == "reference_order":  # 512 spheres: one more than the fast sphere tree's entry ids allow -> variant 4
        api = rl.api
        tex = np.zeros(1, dtype=api.TEXTURE)
        tex[0]["kind"], tex[0]["color"] = api.TEX_SOLID, (0.5, 0.4, 0.3)
        mats = np.zeros(3, dtype=api.MATERIAL)
        mats[0]["kind"], mats[0]["texture"] = api.MAT_LAMBERTIAN, 0
        mats[1]["kind"], mats[1]["ior"] = api.MAT_DIELECTRIC, 1.5
        mats[2]["kind"], mats[2]["albedo"], mats[2]["fuzz"] = api.MAT_METAL, (0.9, 0.9, 0.9), 0.2
        rng = np.random.default_rng(99)
        sph = np.zeros(512, dtype=api.SPHERE)
        sph["center0"], sph["radius"], sph["material"] = rng.uniform(-4, 4, (512, 3)), rng.uniform(0.05, 0.3, 512), rng.integers(0, 3, 512)
        world = rl.World.from_spheres(sph, mats, tex, True)
        p = rl.CameraParams(aspect_ratio=1.5, image_width=48, samples_per_pixel=1, max_depth=8, vfov=60.0, lookfrom=(0.0, 1.0, 9.0), lookat=(0, 0, 0))
        return world, p, -1
    if name == "perlin_spheres":
        world = rl.World.perlin_spheres()
    elif name == "final_scene_one_wave":
        world = rl.World.example_scene("final_scene", rgb8=_synthetic_image())
    else:
        world = rl.World.example_scene(name)
    p = world.params
    p.image_width = 48
    p.max_depth = min(p.max_depth, 20)
    return world, p, 1 if name.endswith("_one_wave") else -1


@pytest.mark.parametrize("name", ["cornell_box", "cornell_smoke", "perlin_spheres", "final_scene_one_wave", "reference_order"])
def test_independent_splits_on_every_kernel_flavour(rl, name):
    """4 on the other flavours: the fast general kernel (cornell_box: <768, 20>), its media (cornell_smoke), texture (perlin_spheres) and
    one-wave (final_scene, forced) forms, which take their parameters through the two-slot ring, and the reference-order wave kernel
    (variant 4): one call = a + (S - a) = 3+ passes = claims of 3 samples cut at a pass end = 3 row shards = the chained fold, also from
    a first sample beyond 2^32."""
    world, p, one_wave = _flavour(rl, name)
    F, S, a = 3, 11, 4
    cam = _cam(rl, p, S)
    per_sample = cam.c.image_height * cam.c.image_width * 3 * 8
    try:
        rl.api.set_fastg_one_wave(one_wave)
        ref, tot = _chained(rl, world, p, F, S)
        one, st = _device(rl, cam, world, first_sample=F)
        assert np.array_equal(one, ref), (name, np.abs(one - ref).max())
        assert st["rays"] == tot["rays"] and st["flagged"] == tot["flagged"] == 0, (name, st, tot["rays"])
        first, _ = _device(rl, _cam(rl, p, a), world, first_sample=F)
        two, _ = _device(rl, _cam(rl, p, S - a), world, first_sample=F + a, accumulate=True, init=first)
        assert np.array_equal(two, ref), name
        rl.api.set_indep_cap(per_sample * 3)  # 3 + 3 + 3 + 2: four passes, the parameter ring wraps twice
        passes, _ = _device(rl, cam, world, first_sample=F)
        assert np.array_equal(passes, ref), name
        rl.api.set_indep_cap(per_sample * 5)  # 5 + 5 + 1 with 3 samples per claim: groups of 3, 2 / 3, 2 / 1
        rl.api.set_indep_k(3)
        passes_k, _ = _device(rl, cam, world, first_sample=F)
        assert np.array_equal(passes_k, ref), name
        rl.api.set_indep_cap(0)
        rl.api.set_indep_k(1)
        shards = np.zeros_like(ref)
        for g in range(3):
            part, _ = _device(rl, cam, world, row_first=g, row_step=3, first_sample=F)
            shards[g::3] = part
        assert np.array_equal(shards, ref), name
        big = (1 << 32) + 5
        far_ref, _ = _chained(rl, world, p, big, 4)
        far, _ = _device(rl, _cam(rl, p, 4), world, first_sample=big)
        assert np.array_equal(far, far_ref), name
        assert not np.array_equal(far, _chained(rl, world, p, 5, 4)[0]), name  # the sample index is not truncated to 32 bits
    finally:
        rl.api.set_fastg_one_wave(-1)
        rl.api.set_indep_cap(0)
        rl.api.set_indep_k(1)
