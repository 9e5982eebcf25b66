"""GPU tier: the feature renders (Camera.render_features / render_features_device / render_pixels_features / render_pixels_features_device;
include/rl_render.h "Feature renders").  No tolerance anywhere: everything is compared as bytes.

The yardstick is the host composition of calls that know nothing of this feature (as _compose of tests/test_gpu_path_query.py): per sample
s the cursors (s*W*H + px*W + py, 0), cam.get_rays for rays and the cursors behind them, world.hit_rays_seeded for the hits, the colour
factor from world.materials(), world.texture_values and the header's table, and a numpy float64 fold in ascending s."""
import ctypes as C
import dataclasses
import itertools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
SCENES = ["golden_test_scene", "bouncing_spheres", "cornell_smoke", "simple_light", "perlin_spheres", "cow_scene", "flat_world"]
OUTPUTS = ("albedo_sum", "normal_sum", "depth_sum", "hit_count")
FLAT, LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT, ISOTROPIC = range(6)  # include/rl_render.h RL_MAT_*
W0, H0, S = 24, 18, 3  # non-square: a kernel that numbered its streams y*W + x would not get these bytes


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_fast_traversal(True)


def _spot_texture():
    from PIL import Image
    root = os.path.dirname(os.path.abspath(__file__))
    return np.asarray(Image.open(os.path.join(root, "golden", "spot_texture.png")).convert("RGB"))


_worlds = {}


def _scene(rl, golden, name):
    """(world, camera of S samples) at W0 x H0."""
    if name not in _worlds:
        if name == "golden_test_scene":
            w = rl.World.golden_test_scene()
        elif name == "bouncing_spheres":
            w = rl.World.bouncing_spheres(1)
        elif name == "cow_scene":
            w = rl.World.cow_scene(golden("spot_triangulated.obj.gz"), _spot_texture())
        elif name == "simple_light":
            w = rl.World.simple_light()
        elif name == "perlin_spheres":
            w = rl.World.perlin_spheres()
        else:
            w = rl.World.example_scene(name)
        _worlds[name] = w
    w = _worlds[name]
    p = dataclasses.replace(w.params, image_width=W0, aspect_ratio=W0 / (H0 + 0.5), samples_per_pixel=S)  # height = floor(W / aspect) = H0
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (W0, H0)
    return w, cam


def _pixels(cam):
    W, H = cam.c.image_width, cam.c.image_height
    y, x = np.divmod(np.arange(W * H, dtype=np.uint64), np.uint64(W))
    return x, y


def _compose(rl, world, cam, px, py, F, samples, counting=False):
    """-> ({the four outputs, [n, ...]}, the material kinds of the first hits, the summed counters with rng_words = the summed final word
    positions)."""
    api = rl.api
    W, H = cam.c.image_width, cam.c.image_height
    px, py = np.asarray(px, dtype=np.uint64), np.asarray(py, dtype=np.uint64)
    n = px.shape[0]
    mats = world.materials()
    background = np.array(cam.params.background, dtype=np.float64)
    albedo, normal, depth, count = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n), np.zeros(n, dtype=np.uint32)
    kinds = set()
    tot = dict.fromkeys(COUNTERS, 0)
    for s in range(F, F + samples):
        cur = api.pack_cursors(np.uint64(s) * np.uint64(W * H) + px * np.uint64(W) + py, 0)
        rays, cur1 = cam.get_rays(px, py, cur)
        st = {} if counting else None
        hits, cur2 = world.hit_rays_seeded(rays, cur1, cam.params.seed, stats=st, allow_degenerate=True)
        hit = hits["hit"] != 0
        m = mats[np.where(hit, hits["material"], 0)]
        kind = m["kind"]
        a = np.zeros((n, 3))
        tex = hit & np.isin(kind, (LAMBERTIAN, DIFFUSE_LIGHT, ISOTROPIC))
        if tex.any():
            a[tex] = world.texture_values(m["texture"][tex], np.stack([hits["u"][tex], hits["v"][tex]], axis=1), hits["p"][tex])
        a[hit & (kind == METAL)] = m["albedo"][hit & (kind == METAL)]
        a[hit & (kind == DIELECTRIC)] = 1.0
        a[~hit] = background
        albedo = albedo + a
        normal = normal + np.where(hit[:, None], hits["normal"], 0.0)
        depth = depth + np.where(hit, hits["t"], 0.0)
        count = count + hit.astype(np.uint32)
        kinds |= set(int(k) for k in np.unique(kind[hit]))
        if counting:
            for k in COUNTERS:
                tot[k] += st[k]
            tot["rng_words"] += int(cur2["word_pos"].sum(dtype=np.uint64)) - st["rng_words"]  # (st: the media's words, part of the final positions)
    return {"albedo_sum": albedo, "normal_sum": normal, "depth_sum": depth, "hit_count": count}, kinds, tot


_frames = {}


def _yardstick(rl, golden, name, F):
    """The whole W0 x H0 frame of `name` from sample F on, computed once and shared: ({outputs [H*W, ...]}, kinds)."""
    if (name, F) not in _frames:
        world, cam = _scene(rl, golden, name)
        px, py = _pixels(cam)
        want, kinds, _ = _compose(rl, world, cam, px, py, F, S)
        for a in want.values():
            a.setflags(write=False)
        _frames[(name, F)] = (want, kinds)
    return _frames[(name, F)]


def _same(got, want):
    return got is not None and got.size == want.size and np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


def _assert_features(got, want, what, outputs=OUTPUTS):
    for k in OUTPUTS:
        if k in outputs:
            assert _same(getattr(got, k), want[k]), (what, k)
        else:
            assert getattr(got, k) is None, (what, k)


def test_the_scene_set_covers_every_material_kind_partial_hits_and_misses(rl, golden):
    """Asserted on the yardstick alone, before any result of the feature is looked at."""
    kinds, partial, none = set(), 0, 0
    for name in SCENES:
        want, k = _yardstick(rl, golden, name, 0)
        kinds |= k
        partial += int(((want["hit_count"] > 0) & (want["hit_count"] < S)).sum())
        none += int((want["hit_count"] == 0).sum())
    assert {LAMBERTIAN, METAL, DIELECTRIC, DIFFUSE_LIGHT, ISOTROPIC} <= kinds, kinds
    assert partial > 0 and none > 0, (partial, none)


@pytest.mark.parametrize("name", SCENES)
def test_frames_through_both_routes_are_the_yardsticks_bytes(rl, golden, name):
    """1: all four outputs, F in {0, 3}, through the fast walk (counter-free calls on a scene with a media-free query tree) and through the
    reference-order trace (set_fast_traversal(False), media scenes, every counting call); last_query() names the route that ran."""
    api = rl.api
    world, cam = _scene(rl, golden, name)
    px, py = _pixels(cam)
    fast_route = "features_reference" if name == "cornell_smoke" else "features_fast"  # a medium draws: the reference's order
    for F in (0, 3):
        want, _ = _yardstick(rl, golden, name, F)
        for on, route in ((True, fast_route), (False, "features_reference")):
            api.set_fast_traversal(on)
            try:
                got = cam.render_pixels_features(world, px, py, first_sample=F, allow_degenerate=True)  # counter-free: may take the fast walk
                assert api.last_query()["kernel"] == route, (name, F, on, api.last_query())
                _assert_features(got, want, (name, F, on))
                got = cam.render_features(world, first_sample=F, allow_degenerate=True)  # _rows always counts
                assert api.last_query() == {"kernel": "features_reference", "retraced": 0}, (name, F, on)
                _assert_features(got, want, (name, F, on, "rows"))
                assert got.albedo_sum.shape == (H0, W0, 3) and got.depth_sum.shape == (H0, W0) and got.hit_count.dtype == np.uint32
            finally:
                api.set_fast_traversal(True)


def test_a_first_sample_beyond_32_bits(rl, golden):
    """F = 2**33 + 1: the stream number is 64-bit arithmetic."""
    world, cam = _scene(rl, golden, "bouncing_spheres")
    px, py = _pixels(cam)
    F = 2 ** 33 + 1
    want, _, _ = _compose(rl, world, cam, px, py, F, S)
    _assert_features(cam.render_pixels_features(world, px, py, first_sample=F), want, "fast")
    _assert_features(cam.render_features(world, first_sample=F), want, "reference")
    assert not _same(want["albedo_sum"], _yardstick(rl, golden, "bouncing_spheres", 0)[0]["albedo_sum"])  # (other streams than F = 0's)


@pytest.mark.parametrize("name", ["golden_test_scene", "bouncing_spheres"])
def test_against_the_render_kernels_at_depth_one(rl, golden, name):
    """2: scenes without emitters.  At max_depth = 1 a sample that hits adds 0.0 and one that misses adds the background, so
    render_independent_rows equals, per pixel and channel, the left-to-right fold of S - hit_count copies of the background."""
    world, cam = _scene(rl, golden, name)
    cam1 = rl.Camera(dataclasses.replace(cam.params, max_depth=1))
    background = np.array(cam.params.background, dtype=np.float64)
    folds = np.zeros((S + 1, 3))
    for k in range(1, S + 1):
        folds[k] = folds[k - 1] + background
    for F in (0, 3):
        beauty = cam1.render_independent_rows(world, 0, 1, first_sample=F, allow_degenerate=True)
        got = cam.render_features(world, first_sample=F, want=("hit_count",), allow_degenerate=True)
        assert _same(beauty, folds[S - got.hit_count.astype(np.int64)]), (name, F)


def test_row_shards_lists_and_every_subset_of_the_outputs(rl, golden):
    """3: shards and a shuffled list with duplicates give the frame's bytes; every subset of the four outputs gives the same bytes in the ones
    requested."""
    name = "bouncing_spheres"
    world, cam = _scene(rl, golden, name)
    want, _ = _yardstick(rl, golden, name, 3)
    frame = {k: v.reshape((H0, W0) + v.shape[1:]) for k, v in want.items()}
    for row_first, row_step in ((0, 1), (1, 3), (H0 - 1, 7)):
        got = cam.render_features(world, first_sample=3, row_first=row_first, row_step=row_step)
        _assert_features(got, {k: v[row_first::row_step] for k, v in frame.items()}, (row_first, row_step))
        assert got.hit_count.shape == (rl.api.rows_for(H0, row_first, row_step), W0)
    rng = np.random.default_rng(20261019)
    pick = np.concatenate([rng.permutation(W0 * H0), rng.integers(0, W0 * H0, 70)])  # every pixel once, shuffled, then 70 duplicates
    ys, xs = np.divmod(pick, W0)
    listed = {k: v[pick] for k, v in want.items()}
    for stats in (None, {}):  # counter-free (fast walk) and counting (reference order)
        _assert_features(cam.render_pixels_features(world, xs, ys, first_sample=3, stats=stats), listed, ("list", stats is not None))
    for r in range(1, 5):
        for subset in itertools.combinations(OUTPUTS, r):
            _assert_features(cam.render_pixels_features(world, xs, ys, first_sample=3, want=subset), listed, subset, subset)
            _assert_features(cam.render_features(world, first_sample=3, row_first=1, row_step=3, want=subset), {k: v[1::3] for k, v in frame.items()}, subset, subset)
    # the empty list: RL_OK, stats zeroed; a pixel outside the image: refused by the host form
    st = {"rays": 7}
    empty = cam.render_pixels_features(world, [], [], stats=st)
    assert empty.albedo_sum.shape == (0, 3) and st["rays"] == 0
    with pytest.raises(rl.RLError) as e:
        cam.render_pixels_features(world, [0, W0], [0, 0])
    assert e.value.code == rl.api.RL_E_INVALID


def _device_buffers(torch, n, guard=0):
    dev = torch.device("cuda", 0)
    return {"albedo_sum": torch.full((n + 2 * guard, 3), float("nan"), dtype=torch.float64, device=dev),
            "normal_sum": torch.full((n + 2 * guard, 3), float("nan"), dtype=torch.float64, device=dev),
            "depth_sum": torch.full((n + 2 * guard,), float("nan"), dtype=torch.float64, device=dev),
            "hit_count": torch.full((n + 2 * guard,), -1, dtype=torch.int32, device=dev)}  # 0xFFFFFFFF


def _ptrs(bufs, guard=0, outputs=OUTPUTS):
    return {"d_" + k: bufs[k][guard:].data_ptr() for k in outputs}


def _host(bufs):
    out = {k: v.cpu().numpy() for k, v in bufs.items()}
    out["hit_count"] = out["hit_count"].view(np.uint32)
    return out


def test_device_list_with_an_element_outside_the_image(rl, golden):
    """3: in the device list form an outside element is zeros in every given output and its neighbours are untouched."""
    import torch
    name = "bouncing_spheres"
    world, cam = _scene(rl, golden, name)
    want, _ = _yardstick(rl, golden, name, 0)
    xs = np.array([3, W0, 5, 7, 0xFFFFFFFF, W0 - 1, 0], dtype=np.uint32)
    ys = np.array([2, 4, H0, 9, 3, H0 - 1, 0], dtype=np.uint32)
    inside = (xs < W0) & (ys < H0)
    n = xs.size
    d_xs, d_ys = torch.from_numpy(xs.view(np.int32).copy()).cuda(), torch.from_numpy(ys.view(np.int32).copy()).cuda()
    for outputs in (OUTPUTS, ("normal_sum", "hit_count")):
        bufs = _device_buffers(torch, n, guard=1)
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        cam.render_pixels_features_device(world, d_xs.data_ptr(), d_ys.data_ptr(), n, stream=stream.cuda_stream, **_ptrs(bufs, 1, outputs))
        assert rl.api.render_status(world)["rays"] == S * int(inside.sum())  # an outside element traces nothing
        torch.cuda.synchronize()
        got = _host(bufs)
        for k in OUTPUTS:
            g = got[k]
            if k not in outputs:  # not asked for: not written
                assert (g == 0xFFFFFFFF).all() if k == "hit_count" else np.isnan(g).all(), k
                continue
            for edge in (g[0], g[-1]):  # the guard elements on either side of the list's outputs
                assert (edge == 0xFFFFFFFF).all() if k == "hit_count" else np.isnan(edge).all(), k
            for i in range(n):
                e = np.zeros_like(want[k][0]) if not inside[i] else want[k][int(ys[i]) * W0 + int(xs[i])]
                assert g[1 + i].tobytes() == np.asarray(e).tobytes(), (k, i)


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_smoke"])
def test_counting_calls_have_the_reference_counters(rl, golden, name):
    """4: all seven counters of a counting call equal the sums over s of the yardstick's counting hit_rays_seeded stats, the nested boundary
    traces of media included; rng_words is the summed final word positions."""
    world, cam = _scene(rl, golden, name)
    px, py = _pixels(cam)
    want, _, tot = _compose(rl, world, cam, px, py, 3, S, counting=True)
    assert tot["rays"] == S * W0 * H0 and tot["rng_words"] >= 6 * S * W0 * H0  # get_ray draws at least three f64
    gs = {}
    got = cam.render_features(world, first_sample=3, stats=gs, allow_degenerate=True)
    _assert_features(got, want, name)
    assert {k: gs[k] for k in COUNTERS} == tot, (name, gs, tot)
    ls = {}
    got = cam.render_pixels_features(world, px, py, first_sample=3, stats=ls, allow_degenerate=True)
    _assert_features(got, want, name)
    assert {k: ls[k] for k in COUNTERS} == tot, (name, ls, tot)
    if name == "cornell_smoke":
        assert cam.params.defocus_angle <= 0 and tot["rng_words"] > 6 * S * W0 * H0  # get_ray draws exactly three f64 here: the media drew


def test_device_form_status_and_a_call_between_two_renders(rl, golden):
    """5: render_features_device on a side stream gives the host form's bytes; rl_render_status counts the call once, with rays = S*W*H; a
    call between two asynchronous renders of the same scene on another stream changes neither frame."""
    import torch
    api = rl.api
    name = "bouncing_spheres"
    world, cam = _scene(rl, golden, name)
    want, _ = _yardstick(rl, golden, name, 3)
    host = cam.render_features(world, first_sample=3)
    _assert_features(host, want, "host")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bufs = _device_buffers(torch, W0 * H0)
    torch.cuda.synchronize()
    cam.render_features_device(world, stream=s2.cuda_stream, first_sample=3, **_ptrs(bufs))
    assert api.last_query()["kernel"] == "features_fast"
    st = api.render_status(world)
    assert st["rays"] == S * W0 * H0 and st["flagged"] == 0 and st["rc"] == api.RL_OK
    assert api.render_status(world)["rays"] == 0  # counted once
    torch.cuda.synchronize()
    for k, g in _host(bufs).items():
        assert _same(g, getattr(host, k)), k
    # a row shard, synchronous with stats: the reference-order trace, the same bytes
    nrows = api.rows_for(H0, 1, 3)
    shard = _device_buffers(torch, nrows * W0)
    ss = {}
    torch.cuda.synchronize()
    cam.render_features_device(world, stream=s2.cuda_stream, first_sample=3, row_first=1, row_step=3, stats=ss, **_ptrs(shard))
    assert ss["rays"] == S * nrows * W0 and api.last_query()["kernel"] == "features_reference"
    for k, g in _host(shard).items():
        assert _same(g, getattr(host, k)[1::3]), k
    # between two asynchronous renders
    gs = {}
    frame = cam.render(world, stats=gs).data
    a = torch.zeros((H0, W0, 3), dtype=torch.float64, device="cuda:0")
    b = torch.zeros((H0, W0, 3), dtype=torch.float64, device="cuda:0")
    bufs = _device_buffers(torch, W0 * H0)
    torch.cuda.synchronize()
    cam.render_device(world, a.data_ptr(), stream=s1.cuda_stream)
    cam.render_features_device(world, stream=s2.cuda_stream, first_sample=3, **_ptrs(bufs))
    cam.render_device(world, b.data_ptr(), stream=s1.cuda_stream)
    st = api.render_status(world)
    assert st["rays"] == gs["rays"] and st["flagged"] == 0  # rays: of the most recently enqueued one, the second render
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), frame) and np.array_equal(b.cpu().numpy(), frame)
    for k, g in _host(bufs).items():
        assert _same(g, getattr(host, k)), k
    assert api.render_status(world)["rays"] == 0


def test_more_pixels_than_lanes(rl, golden):
    """6: a frame whose pixels exceed the lanes one launch has (features_max_lanes), S = 1: every lane renders several pixels.  Checked as
    bytes against the same frame rendered as two row shards, each of which fits the lanes."""
    import torch
    world = _scene(rl, golden, "golden_test_scene")[0]
    lanes = rl.api.features_max_lanes()
    Wb = 1024
    Hb = lanes // Wb + 2
    Hb += Hb & 1
    cam = rl.Camera(dataclasses.replace(world.params, image_width=Wb, aspect_ratio=Wb / (Hb + 0.5), samples_per_pixel=1))
    assert (cam.c.image_width, cam.c.image_height) == (Wb, Hb) and Wb * Hb > lanes >= Wb * Hb // 2
    whole = _device_buffers(torch, Wb * Hb)
    even, odd = _device_buffers(torch, Wb * Hb // 2), _device_buffers(torch, Wb * Hb // 2)
    torch.cuda.synchronize()
    cam.render_features_device(world, **_ptrs(whole))
    cam.render_features_device(world, row_first=0, row_step=2, **_ptrs(even))
    cam.render_features_device(world, row_first=1, row_step=2, **_ptrs(odd))
    assert rl.api.render_status(world)["rays"] == Wb * Hb // 2
    torch.cuda.synchronize()
    for k in OUTPUTS:
        w = whole[k].reshape((Hb, Wb) + tuple(whole[k].shape[1:]))
        assert torch.equal(w[0::2].reshape(even[k].shape), even[k]) and torch.equal(w[1::2].reshape(odd[k].shape), odd[k]), k
        assert not torch.isnan(w.double()).any()
    assert int(whole["hit_count"].max()) == 1  # S = 1
    # and a sample of the frame against the yardstick itself
    pick = np.random.default_rng(5).choice(Wb * Hb, 2000, replace=False)
    ys, xs = np.divmod(pick, Wb)
    want, _, _ = _compose(rl, world, cam, xs, ys, 0, 1)
    got = _host(whole)
    for k in OUTPUTS:
        assert got[k][pick].tobytes() == want[k].tobytes(), k


def test_arguments_the_other_family_and_a_row_past_the_frame(rl, golden):
    api = rl.api
    lib = api.render_lib()
    world, cam = _scene(rl, golden, "golden_test_scene")
    n = W0 * H0
    bufs = [np.full(n * 3, 7.0), np.full(n * 3, 7.0), np.full(n, 7.0), np.full(n, 7, dtype=np.uint32)]
    f = api.RtiowFeatures(*(b.ctypes.data for b in bufs))
    c = C.byref(cam.c)
    assert lib.rl_rtiow_render_features_rows(world.device(), c, 0, 0, 0, C.byref(f), None) == api.RL_E_INVALID  # row_step 0
    assert lib.rl_rtiow_render_features_rows(world.device(), None, 0, 0, 1, C.byref(f), None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_pixels_features(world.device(), c, 0, None, None, 4, C.byref(f), None) == api.RL_E_INVALID
    rw = rl.RtcWorld.test_mirror_scene(32, 24)
    assert lib.rl_rtiow_render_features_rows(rw.device(), c, 0, 0, 1, C.byref(f), None) == api.RL_E_INVALID  # an RTC scene
    st = api.Stats(rays=9)
    assert lib.rl_rtiow_render_features_rows(world.device(), c, 0, H0, 1, C.byref(f), C.byref(st)) == api.RL_OK and st.rays == 0  # no rows
    assert all((b == 7).all() for b in bufs)


@pytest.mark.skipif(bool(os.environ.get("RL_RENDER_LIB")), reason="the C++ host mirror links librl_render.so (the product library)")
def test_cpp_mirror_renders_features(rl, golden):
    H = rl.api.host_lib()
    H.rlh_render_features_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    world = _scene(rl, golden, "golden_test_scene")[0]
    cam = rl.Camera(dataclasses.replace(world.params, image_width=W0, samples_per_pixel=S))
    n = cam.c.image_width * cam.c.image_height
    want = cam.render_features(world, first_sample=3)
    a, nr, d, k = np.zeros(n * 3), np.zeros(n * 3), np.zeros(n), np.zeros(n, dtype=np.uint32)
    assert H.rlh_render_features_probe(W0, S, 3, a.ctypes.data, nr.ctypes.data, d.ctypes.data, k.ctypes.data) == 0, H.rlh_last_error()
    assert _same(a, want.albedo_sum) and _same(nr, want.normal_sum) and _same(d, want.depth_sum) and _same(k, want.hit_count)
