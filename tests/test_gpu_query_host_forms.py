"""GPU tier: what the host-buffer forms of the batched queries do around their kernels (csrc/rl_query_api.h), seen through the C ABI
itself.  The Python wrappers always pass every optional output and a zeroed rl_stats, so they cannot observe

  * which entries of rl_rtc_intersect_rays' out_isects stay the caller's, and that out_hit_index is optional;
  * that a call without its optional outputs computes the same bytes and never writes the caller's input arrays;
  * that opt_stats is zeroed by an empty batch and filled by a full one, in the host and in the _device forms;
  * that rl_rtiow_hit_rays asks for the counting kernel only when the caller passed opt_stats.

Rays: the first 257 camera rays of each scene (one more than the 256-lane query block) and a batch of 1."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 257
SIZES = [N, 1]


def _p(a):
    return None if a is None else a.ctypes.data


def _ff_stats(api):
    st = api.Stats()
    assert C.sizeof(st) == 64
    C.memset(C.byref(st), 0xFF, 64)
    return st


def _stats_bytes(st):
    return bytes((C.c_ubyte * 64).from_buffer_copy(st))


@pytest.fixture(scope="module")
def rtiow(rl):
    """The golden test scene, its first 257 camera rays with the cursors behind them, and their hit records; left unchanged."""
    rl.init(0)
    api = rl.api
    world = rl.World.golden_test_scene()
    p = world.params
    p.image_width = 24
    cam = rl.Camera(p)
    W, H = cam.c.image_width, cam.c.image_height
    assert W * H >= N
    py, px = np.divmod(np.arange(N, dtype=np.uint64), np.uint64(W))
    rays, cur = cam.get_rays(px, py, api.pack_cursors(px * np.uint64(W) + py))
    hits = world.hit_rays(rays["origin"], rays["dir"], rays["time"])
    assert (hits["hit"] != 0).any()
    return dict(world=world, h=world.device(), p=p, rays=rays, cur=cur, hits=hits)


@pytest.fixture(scope="module")
def rtc(rl):
    """The mirror scene at 30x20, the pixel-centre rays of its first 257 pixels (scene/camera.rs:63-91), their comps and the lengths of
    their intersection lists; left unchanged."""
    rl.init(0)
    api = rl.api
    world = rl.RtcWorld.test_mirror_scene(30, 20)
    cam = world.camera
    inv = np.array(list(cam.inverse)).reshape(4, 4)
    py, px = np.divmod(np.arange(N, dtype=np.float64), float(cam.hsize))
    x = cam.half_width - (px + 0.5) * cam.pixel_size
    y = cam.half_height - (py + 0.5) * cam.pixel_size
    pix = (inv @ np.stack([x, y, np.full(N, -1.0), np.ones(N)]))[:3].T
    org = np.tile(inv[:3, 3], (N, 1))
    d = pix - org
    rays = api.pack_rays(org, d / np.linalg.norm(d, axis=1, keepdims=True))
    comps = world.prepare_rays(rays["origin"], rays["dir"])
    assert (comps["hit"] != 0).any()
    counts, _, _ = world.intersect_rays(rays["origin"], rays["dir"], k=0)
    return dict(world=world, h=world.device(), rays=rays, comps=comps, counts=counts, n_lights=len(world.lights()))


# ----------------------------------------------------------------------------- rl_rtc_intersect_rays: out_isects is uploaded first
@pytest.mark.parametrize("K", [4, 8])  # every ray of this scene crosses its five planes, so only k = 8 leaves entries beyond a ray's count
@pytest.mark.parametrize("n", SIZES)
def test_intersect_rays_leaves_the_entries_beyond_a_rays_count_to_the_caller(rl, rtc, n, K):
    api, lib = rl.api, rl.api.render_lib()
    first = int(np.nonzero(rtc["counts"] < 8)[0][0]) if n == 1 else 0  # the batch of 1 is a ray with a short list
    rays = rtc["rays"][first:first + n].copy()
    rec = api.RTC_ISECT.itemsize

    def call(fill, with_index):
        isects = np.full((n, K, rec), fill, dtype=np.uint8)
        counts = np.zeros(n, dtype=np.uint32)
        index = np.zeros(n, dtype=np.uint32) if with_index else None
        assert lib.rl_rtc_intersect_rays(rtc["h"], _p(rays), n, K, _p(isects), _p(counts), _p(index), None) == api.RL_OK
        return isects, counts, index

    zero, counts0, index0 = call(0, True)
    kept, counts, index = call(0xAB, True)
    assert counts.tobytes() == counts0.tobytes() and index.tobytes() == index0.tobytes()
    written = np.arange(K)[None, :] < np.minimum(counts, K)[:, None]  # [n, K]
    assert written.any()
    if K == 8:
        assert (~written).any()  # short lists: entries that must stay the caller's
    if n == N:
        assert (counts > K).any()  # and cut ones
    assert (kept[~written] == 0xAB).all()
    assert kept[written].tobytes() == zero[written].tobytes()
    no_index, counts1, _ = call(0xAB, False)  # out_hit_index = NULL
    assert counts1.tobytes() == counts0.tobytes() and no_index.tobytes() == kept.tobytes()


# ----------------------------------------------------------------------------- absent optional outputs
@pytest.mark.parametrize("n", SIZES)
def test_ray_color_rays_without_its_optional_outputs(rl, rtiow, n):
    api, lib = rl.api, rl.api.render_lib()
    p = rtiow["p"]
    rays, cur = rtiow["rays"][:n].copy(), rtiow["cur"][:n].copy()
    before = cur.tobytes()
    bg = (C.c_double * 3)(*[float(v) for v in p.background])
    rgb_full, rgb_bare = np.zeros((n, 3)), np.zeros((n, 3))
    out_cur, counts = np.zeros(n, dtype=api.RNG_CURSOR), np.zeros(n, dtype=np.uint32)
    args = (rtiow["h"], _p(rays), _p(cur), n, int(p.seed), int(p.max_depth), bg)
    assert lib.rl_rtiow_ray_color_rays(*args, _p(rgb_full), _p(out_cur), _p(counts), None) == api.RL_OK
    assert cur.tobytes() == before
    assert lib.rl_rtiow_ray_color_rays(*args, _p(rgb_bare), None, None, None) == api.RL_OK
    assert cur.tobytes() == before
    assert rgb_bare.tobytes() == rgb_full.tobytes()
    assert counts.all() and np.array_equal(out_cur["stream"], cur["stream"])  # (the full call did fill them)
    if n == N:
        assert (out_cur["word_pos"] > cur["word_pos"]).any()


@pytest.mark.parametrize("n", SIZES)
def test_scatter_rays_without_its_output_cursors(rl, rtiow, n):
    api, lib = rl.api, rl.api.render_lib()
    first = int(np.nonzero(rtiow["hits"]["hit"] != 0)[0][0]) if n == 1 else 0  # the batch of 1 is a hit
    sl = slice(first, first + n)
    rays, hits, cur = rtiow["rays"][sl].copy(), rtiow["hits"][sl].copy(), rtiow["cur"][sl].copy()
    before = cur.tobytes()
    full, bare = np.zeros(n, dtype=api.SCATTER), np.zeros(n, dtype=api.SCATTER)
    out_cur = np.zeros(n, dtype=api.RNG_CURSOR)
    args = (rtiow["h"], _p(rays), _p(hits), _p(cur), n, int(rtiow["p"].seed))
    assert lib.rl_rtiow_scatter_rays(*args, _p(full), _p(out_cur), None) == api.RL_OK
    assert cur.tobytes() == before
    assert lib.rl_rtiow_scatter_rays(*args, _p(bare), None, None) == api.RL_OK
    assert cur.tobytes() == before
    assert bare.tobytes() == full.tobytes() and np.array_equal(out_cur["stream"], cur["stream"])
    if n == N:
        assert (full["scatter"] != 0).any() and (out_cur["word_pos"] > cur["word_pos"]).any()


@pytest.mark.parametrize("n", SIZES)
def test_shade_hits_without_its_shadow_output(rl, rtc, n):
    api, lib = rl.api, rl.api.render_lib()
    first = int(np.nonzero(rtc["comps"]["hit"] != 0)[0][0]) if n == 1 else 0
    comps = rtc["comps"][first:first + n].copy()
    full, bare = np.zeros(n, dtype=api.RTC_SHADE), np.zeros(n, dtype=api.RTC_SHADE)
    shadow = np.full((n, rtc["n_lights"]), -1.0)
    assert lib.rl_rtc_shade_hits(rtc["h"], _p(comps), n, _p(full), _p(shadow), None) == api.RL_OK
    assert lib.rl_rtc_shade_hits(rtc["h"], _p(comps), n, _p(bare), None, None) == api.RL_OK
    assert bare.tobytes() == full.tobytes() and (n != N or full["surface"].any())
    assert ((shadow >= 0.0) & (shadow <= 1.0)).all()  # every entry was copied back


# ----------------------------------------------------------------------------- opt_stats
def test_an_empty_batch_zeroes_opt_stats_in_host_and_device_forms(rl, rtiow, rtc):
    api, lib = rl.api, rl.api.render_lib()
    rt, rc = rtiow["h"], rtc["h"]
    bg = (C.c_double * 3)(0.0, 0.0, 0.0)
    inf = float("inf")
    calls = {  # one host form and one _device form per family, and the other forms that take opt_stats
        "hit_rays": lambda s: lib.rl_rtiow_hit_rays(rt, None, 0, 1e-10, inf, None, s),
        "hit_rays_device": lambda s: lib.rl_rtiow_hit_rays_device(rt, None, 0, 1e-10, inf, None, None, s),
        "intersect_rays": lambda s: lib.rl_rtc_intersect_rays(rc, None, 0, 4, None, None, None, s),
        "intersect_rays_device": lambda s: lib.rl_rtc_intersect_rays_device(rc, None, 0, 4, None, None, None, None, s),
        "color_at_rays": lambda s: lib.rl_rtc_color_at_rays(rc, None, 0, None, s),
        "color_at_rays_device": lambda s: lib.rl_rtc_color_at_rays_device(rc, None, 0, None, None, s),
        "ray_color_rays": lambda s: lib.rl_rtiow_ray_color_rays(rt, None, None, 0, 1, 5, bg, None, None, None, s),
        "ray_color_rays_device": lambda s: lib.rl_rtiow_ray_color_rays_device(rt, None, None, 0, 1, 5, bg, None, None, None, None, s),
        "scatter_rays": lambda s: lib.rl_rtiow_scatter_rays(rt, None, None, None, 0, 1, None, None, s),
        "scatter_rays_device": lambda s: lib.rl_rtiow_scatter_rays_device(rt, None, None, None, 0, 1, None, None, None, s),
        "prepare_rays": lambda s: lib.rl_rtc_prepare_rays(rc, None, 0, None, s),
        "prepare_rays_device": lambda s: lib.rl_rtc_prepare_rays_device(rc, None, 0, None, None, s),
        "shade_hits": lambda s: lib.rl_rtc_shade_hits(rc, None, 0, None, None, s),
        "shade_hits_device": lambda s: lib.rl_rtc_shade_hits_device(rc, None, 0, None, None, None, s),
        "shadow_attenuation": lambda s: lib.rl_rtc_shadow_attenuation(rc, None, None, 0, None, s),
        "shadow_attenuation_device": lambda s: lib.rl_rtc_shadow_attenuation_device(rc, None, None, 0, None, None, s),
    }
    for name, call in calls.items():
        st = _ff_stats(api)
        assert call(C.byref(st)) == api.RL_OK, name
        assert _stats_bytes(st) == bytes(64), name


def test_a_full_batch_fills_opt_stats_of_the_host_forms(rl, rtiow, rtc):
    api, lib = rl.api, rl.api.render_lib()
    n, p = N, rtiow["p"]
    rays, cur, hits = rtiow["rays"].copy(), rtiow["cur"].copy(), rtiow["hits"].copy()
    rrays, comps = rtc["rays"].copy(), rtc["comps"].copy()
    bg = (C.c_double * 3)(*[float(v) for v in p.background])
    out_hits, rgb, scat = np.zeros(n, dtype=api.RTIOW_HIT), np.zeros((n, 3)), np.zeros(n, dtype=api.SCATTER)
    counts, out_comps, shade = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=api.RTC_COMPS), np.zeros(n, dtype=api.RTC_SHADE)
    calls = {
        "hit_rays": lambda s: lib.rl_rtiow_hit_rays(rtiow["h"], _p(rays), n, 1e-10, float("inf"), _p(out_hits), s),
        "ray_color_rays": lambda s: lib.rl_rtiow_ray_color_rays(rtiow["h"], _p(rays), _p(cur), n, int(p.seed), int(p.max_depth), bg, _p(rgb), None, None, s),
        "scatter_rays": lambda s: lib.rl_rtiow_scatter_rays(rtiow["h"], _p(rays), _p(hits), _p(cur), n, int(p.seed), _p(scat), None, s),
        "intersect_rays": lambda s: lib.rl_rtc_intersect_rays(rtc["h"], _p(rrays), n, 0, None, _p(counts), None, s),
        "color_at_rays": lambda s: lib.rl_rtc_color_at_rays(rtc["h"], _p(rrays), n, _p(rgb), s),
        "prepare_rays": lambda s: lib.rl_rtc_prepare_rays(rtc["h"], _p(rrays), n, _p(out_comps), s),
        "shade_hits": lambda s: lib.rl_rtc_shade_hits(rtc["h"], _p(comps), n, _p(shade), None, s),
    }
    for name, call in calls.items():
        st = _ff_stats(api)
        assert call(C.byref(st)) == api.RL_OK, name
        assert 0 < st.rays < 2 ** 40 and st.flagged == 0, (name, st.as_dict())
        assert 0.0 <= st.kernel_ms < 60e3, (name, st.kernel_ms)
    assert out_hits.tobytes() == rtiow["hits"].tobytes() and out_comps.tobytes() == rtc["comps"].tobytes()


# ----------------------------------------------------------------------------- rl_rtiow_hit_rays: counting only when asked
@pytest.mark.parametrize("n", SIZES)
def test_hit_rays_counts_only_when_the_caller_passes_opt_stats(rl, rtiow, n):
    api, lib = rl.api, rl.api.render_lib()
    rays = rtiow["rays"][:n].copy()
    bare, counted = np.zeros(n, dtype=api.RTIOW_HIT), np.zeros(n, dtype=api.RTIOW_HIT)
    assert lib.rl_rtiow_hit_rays(rtiow["h"], _p(rays), n, 1e-10, float("inf"), _p(bare), None) == api.RL_OK
    assert api.last_query()["kernel"] == "fast"  # kernel 2: a sphere-only scene, the default switches
    st = _ff_stats(api)
    assert lib.rl_rtiow_hit_rays(rtiow["h"], _p(rays), n, 1e-10, float("inf"), _p(counted), C.byref(st)) == api.RL_OK
    assert api.last_query()["kernel"] == "reference"  # kernel 1
    assert bare.tobytes() == counted.tobytes() == rtiow["hits"][:n].tobytes()
    assert st.rays == n and st.node_tests + st.sphere_tests > 0 and st.flagged == 0
