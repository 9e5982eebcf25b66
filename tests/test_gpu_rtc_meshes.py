"""GPU tier: RTC triangle meshes beyond the LDS scene and under hard guard cases, against the oracle's every-triangle loop (no guards).

Routes.  rtc_render_launch stages ops, triangles and guards in LDS while they fit 64 KB and reads them from global memory above that
(rtc_kernel<256, false>, rtc_pixels_kernel<256, false>); worlds with reflective materials go through rtc_full_kernel and the unbounded
line test.  Each test reads api.last_rtc_launch() after its launches and asserts the route it is there for, so a moved threshold fails
the test instead of quietly taking it off the route.  Sizes: 7 (no guards), 8 (the smallest tree), the largest n that still fits LDS,
that n + 1, and 1024 (a tree 11 levels deep); two and three ranges with the second tree at a nonzero root offset.

Hard guard cases (tests/rtc_mesh_worlds.py hard_cases): frames, and directed rays through intersect_rays and color_at_rays, on worlds
where the slack and pad terms of the binary32 box test are largest against the boxes.  tests/test_rtc_guard_trees.py holds the CPU half:
the trees' structure, and that the directed rays both hit and miss."""
import numpy as np
import pytest

import rtc_mesh_worlds as mw
from rtc_mesh_worlds import COUNTERS, H, W

pytestmark = pytest.mark.gpu
AA = 2
K = 8
_cache = {}


def _n_lds(rl):
    """the largest n whose scene still fits the 64 KB of LDS, found on the host"""
    if "n_lds" not in _cache:
        sizes = {n: rl.api.rtc_program(mw.route_world(rl, n))["scene_bytes"] for n in range(280, 301)}
        n_lds = max(n for n, b in sizes.items() if b <= 65536)
        assert n_lds + 1 < 300 and 0 <= 65536 - sizes[n_lds] < 224 and sizes[n_lds + 1] > 65536  # the pair really straddles the limit
        _cache["n_lds"] = n_lds
    return _cache["n_lds"]


def _launch_is(api, kernel, is_list, lds_bytes):
    got = api.last_rtc_launch()
    assert (got["kernel"], got["list"], got["lds_bytes"]) == (kernel, is_list, lds_bytes) and got["blocks"] >= 1, got


def _frame(rl, oracle, w, aa, tol, tag):
    """-> (frame, its counters) after asserting: counters equal the oracle's, colours within tol"""
    gs, cs = {}, {}
    img = w.render(aa, stats=gs, allow_degenerate=True)
    ref = oracle.rtc_render(w.desc, w.camera, aa=aa, stats=cs)
    err = float(np.abs(img - ref).max())
    print(tag, "max colour error", err, {k: gs[k] for k in COUNTERS})
    for k in COUNTERS:
        assert gs[k] == cs[k], (tag, k, gs[k], cs[k])
    assert err <= tol, (tag, err)
    return img, gs


def _scene_bytes(rl, w):
    return rl.api.rtc_program(w)["scene_bytes"]


@pytest.mark.parametrize("size", ["7", "8", "n_lds", "n_lds + 1", "1024"])
def test_every_route_of_the_triangle_kernel_equals_the_oracle(rl, oracle, size):
    import torch
    rl.init(0)
    api = rl.api
    n_lds = _n_lds(rl)
    n = {"n_lds": n_lds, "n_lds + 1": n_lds + 1}.get(size) or int(size)
    w = mw.route_world(rl, n)
    prog = api.rtc_program(w)
    assert len(prog["guards"]) == (0 if n < 8 else 2 * n - 1)
    lds = prog["scene_bytes"] if n <= n_lds else 0  # above the limit the scene is read from global memory
    cam = w.camera
    assert (cam.hsize, cam.vsize) == (W, H)
    img, gs = _frame(rl, oracle, w, AA, 1e-12, f"route {n}")
    _launch_is(api, "rtc", False, lds)
    assert gs["rays"] > W * H * AA * AA and img.std() > 0.05  # the mesh is in view and lit: shadow rays were traced
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    # the counter-free frame
    buf = torch.full((H, W, 3), float("nan"), dtype=torch.float64, device=dev)
    w.render_device(buf.data_ptr(), AA, stream=stream)
    st = api.render_status(w)
    _launch_is(api, "rtc", False, lds)
    assert np.array_equal(buf.cpu().numpy(), img) and st["rays"] == gs["rays"]
    # a shuffled pixel list with duplicates and an odd length, host and device forms
    rng = np.random.default_rng(n)
    idx = np.concatenate([rng.permutation(W * H)[:700], rng.integers(0, W * H, 77)])
    xs, ys = idx % W, idx // W
    assert len(idx) % 2 == 1 and len(np.unique(idx)) < len(idx)
    px = w.render_pixels(xs, ys, AA)
    _launch_is(api, "rtc", True, lds)
    assert np.array_equal(px, img[ys, xs])
    xs_d, ys_d = xs.copy(), ys.copy()
    xs_d[5], ys_d[9] = W, H + 3  # two elements outside the image: zeros
    d_xs = torch.from_numpy(xs_d.astype(np.uint32).view(np.int32)).to(dev)
    d_ys = torch.from_numpy(ys_d.astype(np.uint32).view(np.int32)).to(dev)
    d_out = torch.full((len(idx), 3), float("nan"), dtype=torch.float64, device=dev)
    w.render_pixels_device(d_xs.data_ptr(), d_ys.data_ptr(), len(idx), d_out.data_ptr(), AA, stream=stream)
    api.render_status(w)
    _launch_is(api, "rtc", True, lds)
    want = img[ys, xs].copy()
    want[5], want[9] = 0.0, 0.0
    assert np.array_equal(d_out.cpu().numpy(), want)
    # row shards
    whole = np.full_like(img, np.nan)
    for first in range(3):
        whole[first::3] = w.render(AA, row_first=first, row_step=3)
        _launch_is(api, "rtc", False, lds)
    assert np.array_equal(whole, img)


def test_a_reflective_1024_triangle_mesh_through_the_full_kernel(rl, oracle):
    """rtc_full_kernel and guard_reject32_line on the 11-level tree: material 3 reflects, so hits spawn secondary rays"""
    rl.init(0)
    w = mw.route_world(rl, 1024, reflective=(3,))
    img, gs = _frame(rl, oracle, w, AA, 1e-10, "full 1024")
    _launch_is(rl.api, "full", False, 0)
    assert gs["rays"] > 2 * W * H and img.std() > 0.05


@pytest.mark.parametrize("same", [False, True])
@pytest.mark.parametrize("depth", [2, 8])
def test_two_and_three_ranges_with_trees_at_nonzero_offsets(rl, oracle, depth, same):
    """Group A (300 flat triangles), Transformed^depth(Group B) — 40 smooth triangles, or Group A itself once more under another chain: two
    trees over the same triangles — and the unguarded Group C.  The second tree's root is op.skip - 1 = 599."""
    rl.init(0)
    api = rl.api
    w = mw.multi_range_world(rl, depth, same)
    prog = api.rtc_program(w)
    roots = [int(o["skip"]) for o in prog["ops"][prog["ops"]["code"] == api.ROP_TRIS]]
    assert roots == [1, 600, 0] and prog["scene_bytes"] > 65536
    img, gs = _frame(rl, oracle, w, AA, 1e-12, f"ranges depth {depth} same {same}")
    _launch_is(api, "rtc", False, 0)
    assert gs["instance_enters"] > 0 and img.std() > 0.05
    o, d = mw.directed_rays(w, 11, n_sample=6)
    _rays_equal_the_oracle(rl, oracle, w, o, d, f"ranges depth {depth} same {same}")


# ----------------------------------------------------------------------------- hard guard cases
def _hit_of(ts):  # intersect.rs:159-168
    want = -1
    for j in range(len(ts)):
        if ts[j] >= 0.0 and (want < 0 or not (ts[want] < ts[j])):
            want = j
    return want


def _rays_equal_the_oracle(rl, oracle, w, o, d, tag):
    """intersect_rays(k = 8): counts, the first entries' object ids and t bit for bit, hit_index; color_at_rays within 1e-10.  Asserts on
    the oracle's lists alone that at least half of the rays hit and at least a tenth miss, so that both answers are compared."""
    n = len(o)
    lists = [oracle.rtc_intersect(w.desc, o[i], d[i], cap=64) for i in range(n)]
    hits = sum(len(l[0]) > 0 for l in lists)
    assert 2 * hits >= n and 10 * (n - hits) >= n, (tag, hits, n)
    st = {}
    counts, isects, hit_index = w.intersect_rays(o, d, k=K, stats=st, allow_degenerate=True)
    rgb = w.color_at_rays(o, d, allow_degenerate=True)
    assert st["rays"] == n
    worst = 0.0
    for i, (ts, objs, _) in enumerate(lists):
        m = min(len(ts), K)
        assert counts[i] == len(ts), (tag, i, o[i], d[i], counts[i], isects["t"][i, :K], ts)
        assert np.array_equal(isects["t"][i, :m], ts[:m]), (tag, i, o[i], d[i], isects["t"][i, :m], ts[:m])
        assert np.array_equal(isects["object"][i, :m], objs[:m]), (tag, i, isects["object"][i, :m], objs[:m])
        want = _hit_of(ts)
        assert hit_index[i] == (rl.api.NO_HIT if want < 0 else want), (tag, i, hit_index[i], want)
        ref = oracle.rtc_color_at(w.desc, o[i], d[i])
        err = float(np.abs(rgb[i] - ref).max())
        worst = max(worst, err)
        assert err <= 1e-10 * max(1.0, float(np.abs(ref).max())), (tag, i, o[i], d[i], rgb[i], ref)
    print(tag, "rays", n, "hit", hits, "longest list", max(len(l[0]) for l in lists), "max colour error", worst)


@pytest.mark.parametrize("name", mw.CASE_NAMES)
def test_hard_guard_cases_equal_the_oracle(rl, oracle, name):
    rl.init(0)
    api = rl.api
    build, full = mw.hard_cases(rl)[name]
    w = build()
    axis = name.startswith("axis")
    img, gs = _frame(rl, oracle, w, 1 if axis else AA, 1e-10 if full else 1e-12, name)  # (the axis camera's exact zeros need one sample per pixel)
    _launch_is(api, "full" if full else "rtc", False, 0 if full or _scene_bytes(rl, w) > 65536 else _scene_bytes(rl, w))
    if name != "extent 1e-4":  # (to unit directions that mesh does not exist: rtc_mesh_worlds.py)
        assert img.std() > 0.01 and gs["rays"] > (1.2 if axis else 2) * img.shape[0] * img.shape[1]  # in view, and shadow rays were traced
    o, d = mw.directed_rays(w, 7)
    _rays_equal_the_oracle(rl, oracle, w, o, d, name)


def test_duplicated_triangles_show_the_later_material(rl, oracle):
    """the ties case once more, by what it is there for: rays at the centroids of the duplicated triangles return both entries at one t and the
    hit is the later one"""
    rl.init(0)
    w = mw.hard_cases(rl)["ties: duplicates 150 later and a coplanar fan"][0]()
    cen = w.verts[20:28].mean(axis=1)
    ang = np.arctan2(cen[:, 2], cen[:, 0])
    out = cen - 0.35 * np.stack([np.cos(ang), np.zeros(8), np.sin(ang)], axis=1)  # away from the tube's centre line: nothing lies in front
    o = cen + out / np.linalg.norm(out, axis=1, keepdims=True) * 0.1
    d = cen - o
    counts, isects, hit_index = w.intersect_rays(o, d, k=K)
    for i in range(8):
        ts, objs, _ = oracle.rtc_intersect(w.desc, o[i], d[i], cap=64)
        assert counts[i] == len(ts) and np.array_equal(isects["t"][i, :len(ts)], ts) and np.array_equal(isects["object"][i, :len(ts)], objs)
        h = int(hit_index[i])
        assert h == _hit_of(ts) and isects["object"][i, h] == 170 + i and isects["t"][i, h] == isects["t"][i, h - 1] and isects["object"][i, h - 1] == 20 + i


def test_axis_parallel_rays_through_the_global_memory_route(rl, oracle):
    """the axis camera on the n_lds + 1 world: the centre row and column (d.y == 0, d.x == 0: infinite 1/d) through rtc_kernel<256, false>"""
    rl.init(0)
    w = mw.axis_world(rl, _n_lds(rl) + 1)
    img, gs = _frame(rl, oracle, w, 1, 1e-12, "axis n_lds + 1")
    _launch_is(rl.api, "rtc", False, 0)
    assert img[15].std() > 0.01 and img[:, 23].std() > 0.01  # the centre row and column see the mesh
    xs, ys = np.concatenate([np.arange(47), np.full(31, 23)]), np.concatenate([np.full(47, 15), np.arange(31)])
    assert np.array_equal(w.render_pixels(xs, ys, 1), img[ys, xs])
    _launch_is(rl.api, "rtc", True, 0)
