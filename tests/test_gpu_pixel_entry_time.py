"""GPU tier: the time slices of the per-pixel entry table and its reuse across calls (csrc/rl_pixel_entry.h "Time slices", rl_render.hip
build_pixel_entry).  With T = 2, 4 or 8 slices a camera ray starts at the entry word of its pixel AND of the slice its time falls into; the
frames must not change by a bit: for every T the timed frame equals the root walk's (no table), the one-slice table's and the counting
kernel's, with the same `rays`, `flagged` and `slow_traces`.  The slice words themselves are read back: a sphere that crosses a pixel's beam
in one slice only is in that slice's word and in no other, a stationary world's slice words are the all-times word, and below a slice
word's entries lie no leaves that are not below the all-times word's.  A call that repeats camera, rows and switches launches no table
kernel (entry_table.builds(): the table kernels launched; the render funnels' launch log lists the render kernels only)."""
import numpy as np
import pytest

from test_gpu_fast_traversal import _mats, _same_bits
from test_gpu_pixel_entry import FAST_NONE, _subtree_spheres, _timed

pytestmark = pytest.mark.gpu
SLICES = (1, 2, 4, 8)


@pytest.fixture(autouse=True)
def _switches(rl):
    """Small frames through the wave-scheduled fast kernel (not the cooperative one); every switch back to its default afterwards."""
    rl.init(0)  # (before the switches: initialising the library reads them from the environment again)
    rl.api.set_coop(False)
    yield
    rl.api.set_coop(True), rl.api.set_pixel_entry(3), rl.entry_table.set_slices(0), rl.entry_table.set_reuse(True)


def _counts(st):
    return st["rays"], st["flagged"], st["slow_traces"]


def _every_slicing(rl, cam, world, render=_timed, **kw):
    """The frame with no table, then with 1, 2, 4 and 8 slices: all the same bits and counts.  Returns the frame and its status."""
    rl.api.set_pixel_entry(0)
    root, st_root = render(rl, cam, world, **kw)
    rl.api.set_pixel_entry(3)
    for T in SLICES:
        rl.entry_table.set_slices(T)
        got, st = render(rl, cam, world, **kw)
        print("slices", T, "rays, flagged, slow_traces", _counts(st), "root walk:", _counts(st_root))
        assert _same_bits(got, root), T
        assert _counts(st) == _counts(st_root), T
    return root, st_root


def _against_counting(rl, cam, world):
    gs = {}
    counting = np.asarray(cam.render(world, stats=gs).data).reshape(-1, cam.c.image_width, 3)
    root, st = _every_slicing(rl, cam, world)
    assert _same_bits(root, counting) and st["rays"] == gs["rays"]
    return st


def _words(rl, cam, world, T):
    """(all-times words [H, W], slice words [H, W, T]) of a render with T slices."""
    rl.api.set_pixel_entry(3), rl.entry_table.set_slices(T)
    _timed(rl, cam, world)
    W, H = cam.c.image_width, cam.c.image_height
    return rl.api.pixel_entry_table(world, W * H).reshape(H, W), rl.entry_table.sliced_table(world, W * H, T).reshape(H, W, T)


def _entries(word):
    return [int(word) & 1023, (int(word) >> 10) & 1023, (int(word) >> 20) & 1023]


def _leaves(children, n_inner, word, cache):
    return frozenset().union(*[_subtree_spheres(children, n_inner, e, cache) for e in _entries(word)])


def _check_words(rl, cam, world, T):
    """Format, and for every pixel and slice: the leaves below the slice word's entries are among those below the all-times word's."""
    one, sliced = _words(rl, cam, world, T)
    children, _ = rl.api.fast_tree(world)
    n_inner, cache = len(children), {}
    assert np.all(one >> 30 == 3) and np.all(sliced >> 30 == 3)
    first, rest = sliced & 1023, np.stack([(sliced >> 10) & 1023, (sliced >> 20) & 1023], axis=-1)
    assert np.all((rest == FAST_NONE) | (first[..., None] != FAST_NONE))  # the first slot is used first: a walk starts there
    smaller = 0
    for y in range(one.shape[0]):
        for x in range(one.shape[1]):
            whole = _leaves(children, n_inner, one[y, x], cache)
            for k in range(T):
                part = _leaves(children, n_inner, sliced[y, x, k], cache)
                assert part <= whole, (x, y, k, sorted(part - whole))
                smaller += len(part) < len(whole)
    return one, sliced, smaller


def _camera(rl, **kw):
    p = dict(aspect_ratio=16.0 / 9.0, image_width=64, samples_per_pixel=16, max_depth=8, vfov=40.0, lookfrom=(0.0, 1.0, 10.0), lookat=(0.0, 0.0, 0.0),
             defocus_angle=0.6, focus_dist=10.0, background=(0.5, 0.6, 0.9), seed=5)
    p.update(kw)
    return rl.Camera(rl.CameraParams(**p))


def _world(rl, c0, c1, r, material=None):
    api = rl.api
    tex, mats = _mats(api)
    n = len(c0)
    sph = np.zeros(n, dtype=api.SPHERE)
    sph["center0"], sph["center1"], sph["radius"] = c0, c1, r
    sph["moving"] = [int(tuple(a) != tuple(b)) for a, b in zip(c0, c1)]
    sph["material"] = material if material is not None else [i % 5 for i in range(n)]
    return rl.World.from_spheres(sph, mats, tex, True)


def _long_sweeps(rl):
    """Twelve spheres that move by ten radii, along x, y and z in turn: the sweep is much larger than the sphere."""
    rng = np.random.default_rng(12)
    c0 = rng.uniform(-3.0, 3.0, (12, 3))
    r = rng.uniform(0.15, 0.4, 12)
    c1 = c0.copy()
    for i in range(12):
        c1[i, i % 3] += 10.0 * r[i] * (1 if i % 2 else -1)
    return _world(rl, [tuple(c) for c in c0], [tuple(c) for c in c1], r)


def test_baseline_scene(rl):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 64, 16, 8
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (64, 36)
    _against_counting(rl, cam, world)
    _, _, smaller = _check_words(rl, cam, world, 4)
    assert smaller > 0  # the slices do cut: somewhere a slice holds fewer leaves than the whole shutter interval


def test_baseline_scene_deep_paths_and_the_resume_launch(rl):
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 64, 64, 50  # spp >= 64: probe launch + cost-sorted resume launch
    _against_counting(rl, rl.Camera(p), world)


def test_sweeps_of_ten_radii(rl):
    world = _long_sweeps(rl)
    cam = _camera(rl)
    _against_counting(rl, cam, world)
    for T in (2, 8):
        _, _, smaller = _check_words(rl, cam, world, T)
        assert smaller > 0


def test_stationary_world_every_slice_word_is_the_all_times_word(rl):
    rng = np.random.default_rng(3)
    c0 = [tuple(c) for c in rng.uniform(-3.0, 3.0, (20, 3))]
    world = _world(rl, c0, c0, rng.uniform(0.1, 0.8, 20))
    cam = _camera(rl)
    _against_counting(rl, cam, world)
    for T in (2, 4, 8):
        one, sliced = _words(rl, cam, world, T)
        assert np.array_equal(sliced, np.repeat(one[..., None], T, axis=-1)), T
    assert np.unique(one).size > 3


def test_coincident_moving_pair_is_retraced_as_before(rl):
    """Two spheres that are the same sphere at every time: their hits tie, the fast walk hands such rays to the reference-order fold, and the
    slices must leave exactly those rays to it."""
    c0 = [(-2.0, 0.0, 0.0), (-2.0, 0.0, 0.0), (1.5, 0.5, -1.0), (0.0, -100.5, 0.0), (2.5, -0.2, 1.0)]
    c1 = [(2.0, 0.6, 0.0), (2.0, 0.6, 0.0), (1.5, 0.5, -1.0), (0.0, -100.5, 0.0), (2.5, 1.2, 1.0)]
    world = _world(rl, c0, c1, [0.5, 0.5, 0.6, 100.0, 0.3], material=[0, 4, 2, 4, 3])
    st = _against_counting(rl, _camera(rl), world)
    assert st["slow_traces"] > 0


def test_a_sphere_that_crosses_a_beam_in_one_slice_only(rl):
    """A sphere of radius 0.1 moves from x = -4 to x = +4: in slice k of 4 it stays within x in [-4 + 2 k, -2 + 2 k].  The pixel that looks at
    (-3, 0, 0) has it in the word of slice 0 and of no other slice; the pixel that looks at (+1, 0, 0) in the word of slice 2 only."""
    c0 = [(-4.0, 0.0, 0.0), (0.0, 3.0, -2.0), (0.0, -3.0, -2.0)]
    c1 = [(4.0, 0.0, 0.0), (0.0, 3.0, -2.0), (0.0, -3.0, -2.0)]
    world = _world(rl, c0, c1, [0.1, 0.5, 0.5], material=[0, 2, 4])
    cam = _camera(rl, lookfrom=(0.0, 0.0, 10.0), defocus_angle=0.0, vfov=60.0)
    _against_counting(rl, cam, world)
    one, sliced, _ = _check_words(rl, cam, world, 4)
    children, _ = rl.api.fast_tree(world)
    n_inner, cache = len(children), {}
    c = cam.c
    p00, du, dv, lf = (np.array(v[:]) for v in (c.pixel_00, c.pixel_du, c.pixel_dv, c.lookfrom))
    for target_x, only in ((-3.0, 0), (1.0, 2)):
        # the pixel whose centre ray passes closest to (target_x, 0, 0): the image plane is parallel to z = 0
        t = (0.0 - lf[2]) / (p00[2] - lf[2])
        at = lf + (p00 - lf) * t, du * t, dv * t  # where pixel (0, 0) meets z = 0, and the steps per pixel there
        px, py = int(round((target_x - at[0][0]) / at[1][0])), int(round((0.0 - at[0][1]) / at[2][1]))
        assert 0 <= px < c.image_width and 0 <= py < c.image_height
        assert 0 in _leaves(children, n_inner, one[py, px], cache)
        holds = [0 in _leaves(children, n_inner, sliced[py, px, k], cache) for k in range(4)]
        assert holds == [k == only for k in range(4)], (px, py, holds)


@pytest.mark.parametrize("mode", ["row_shard", "moments", "indep", "pixel_list"])
def test_other_entry_points(rl, mode):
    import torch
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 64, 16, 8
    cam = rl.Camera(p)
    dev = torch.device("cuda", 0)
    W, H = cam.c.image_width, cam.c.image_height

    def moments(rl, cam, world):
        sums, sq = (torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
        cam.render_moments_device(world, sums.data_ptr(), sq.data_ptr(), stream=torch.cuda.current_stream(dev).cuda_stream)
        st = rl.api.render_status(world)
        return np.concatenate([sums.cpu().numpy(), sq.cpu().numpy()]), st

    def pixel_list(rl, cam, world):
        ys, xs = np.divmod(np.arange(0, W * H, 7, dtype=np.uint32), np.uint32(W))
        out = cam.render_pixels(world, xs, ys)
        return out, rl.api.render_status(world)

    if mode == "row_shard":
        _every_slicing(rl, cam, world, row_first=1, row_step=3)
    elif mode == "indep":
        _every_slicing(rl, cam, world, independent=True)
    else:
        _every_slicing(rl, cam, world, render=moments if mode == "moments" else pixel_list)


def test_a_call_on_another_stream_reuses_the_table_behind_its_build(rl):
    """The build is enqueued on one stream and the very next call, on another stream, reads the table: it waits on the build's event."""
    import torch
    et = rl.entry_table
    dev = torch.device("cuda", 0)
    world = rl.World.bouncing_spheres(1)
    p = world.params
    p.image_width, p.samples_per_pixel, p.max_depth = 64, 16, 8
    cam = rl.Camera(p)
    rl.api.set_pixel_entry(3), et.set_slices(4)
    want, st_want = _timed(rl, cam, world)
    moved = rl.Camera(rl.CameraParams(**{**p.__dict__, "lookfrom": (12.0, 2.5, 3.0)}))
    a, b = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    shape = (cam.c.image_height, cam.c.image_width, 3)
    other, got = (torch.full(shape, float("nan"), dtype=torch.float64, device=dev) for _ in range(2))
    torch.cuda.synchronize(dev)
    b0 = et.builds()
    moved.render_device(world, other.data_ptr(), stream=a.cuda_stream)  # another camera: its table is built on stream a
    cam.render_device(world, other.data_ptr(), stream=a.cuda_stream)    # back: built on stream a again, and not waited for
    cam.render_device(world, got.data_ptr(), stream=b.cuda_stream)      # the same key on stream b: no kernel, behind the build
    st = rl.api.render_status(world)
    torch.cuda.synchronize(dev)
    assert et.builds() == b0 + 2
    assert _same_bits(got.cpu().numpy(), want) and _same_bits(other.cpu().numpy(), want) and st["rays"] == st_want["rays"]


def test_a_repeated_call_reuses_the_table(rl):
    et = rl.entry_table
    world = _long_sweeps(rl)
    cam = _camera(rl)
    rl.api.set_pixel_entry(3), et.set_slices(4)
    b0 = et.builds()
    first, st1 = _timed(rl, cam, world)
    assert et.builds() == b0 + 1
    again, st2 = _timed(rl, cam, world)
    assert et.builds() == b0 + 1  # the same camera, rows and switches: no table kernel
    assert _same_bits(first, again) and _counts(st1) == _counts(st2)
    more = _camera(rl, samples_per_pixel=4, seed=9)  # what the table does not depend on: still no table kernel
    _timed(rl, more, world)
    assert et.builds() == b0 + 1
    moved = _camera(rl, lookfrom=(0.5, 1.0, 10.0))
    other, _ = _timed(rl, moved, world)
    assert et.builds() == b0 + 2 and not _same_bits(other, first)
    back, _ = _timed(rl, cam, world)
    assert et.builds() == b0 + 3 and _same_bits(back, first)
    shard, _ = _timed(rl, cam, world, row_first=1, row_step=3)  # other rows: another table
    assert et.builds() == b0 + 4 and _same_bits(shard, first[1::3])
    et.set_slices(2)  # another slicing: another table
    _timed(rl, cam, world, row_first=1, row_step=3)
    assert et.builds() == b0 + 5
    et.set_slices(4), et.set_reuse(False)
    for n in (6, 7):  # switched off: every call builds, the frames are the same
        rebuilt, st3 = _timed(rl, cam, world)
        assert et.builds() == b0 + n
        assert _same_bits(rebuilt, first) and _counts(st3) == _counts(st1)
    et.set_reuse(True)
    _timed(rl, cam, world)
    assert et.builds() == b0 + 7
