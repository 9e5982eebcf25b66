"""GPU tier: the adaptive renders (Camera.render_adaptive / render_adaptive_device; include/rl_render.h "Adaptive renders").

No tolerance anywhere.  The yardstick uses only calls that know nothing about stopping: for every checkpoint k and for the maximum S,
Camera(samples_per_pixel=k).render_moments(world, first_sample=F) gives sums_k and sq_k (the counting host form: the reference-order
kernel, whatever the switches say), and the header's rule is applied to them in numpy float64, operation by operation.  That gives every
pixel's expected count and its expected sum and sq at that count; every route of the adaptive call must return those bytes.

The bounds come from the yardstick too: the `abs` rule's abs_variance is the median over pixels of max_c (n sq - sum^2) / (n^2 (n - 1)) at
the last checkpoint, the `rel` rule's rel_variance the median of that quantity divided by sum^2 / n^2 over the pixels whose sums are all
nonzero.  On the sphere scenes the expected counts must then hold at least three distinct values, the first checkpoint and S among them
(asserted on the yardstick before the GPU result is looked at): a wrong stop cannot hide."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
SPHERE_SCENES = ["golden_test_scene", "bouncing_spheres"]
SCENES = SPHERE_SCENES + ["cornell_smoke", "flat_world"]
MIN, EVERY = 4, 4


@pytest.fixture(scope="module", autouse=True)
def _switches(rl):
    rl.init(0)
    yield
    rl.api.set_coop(True)
    rl.api.set_fast_traversal(True)
    rl.api.set_lpt(True)


def _routes(name):
    """(coop, fast) switch settings, as tests/test_gpu_render_moments.py: sphere scenes — small-frame routing (the cooperative kernel for a
    moments call; an adaptive call must take the wave kernel's fast layout instead), the fast layout, the guarded compact layout; general
    scenes — the fast general kernel, the reference-order kernel."""
    return [(True, True), (False, True), (True, False)] if name in SPHERE_SCENES else [(True, True), (True, False)]


def _scene(rl, name, spp, width=None):
    w = rl.World.golden_test_scene() if name == "golden_test_scene" else rl.World.bouncing_spheres(1) if name == "bouncing_spheres" else rl.World.example_scene(name)
    p = w.params
    p.image_width = width or (24 if p.aspect_ratio >= 4.0 / 3.0 else 18)
    p.max_depth = min(p.max_depth, 10)
    cam = rl.Camera(dataclasses.replace(p, samples_per_pixel=spp))
    assert cam.c.image_width <= 24 and cam.c.image_height <= 18
    return w, cam


def _checkpoints(S):
    return list(range(MIN, S, EVERY))


def _ok(n, s, q, a, r):
    """The header's rule at n samples, in float64, every operation on its own: [H, W] bool, all three channels pass."""
    nd = np.float64(n)
    a, r = np.float64(a), np.float64(r)
    s2 = s * s
    lhs = (nd * q) - s2
    rhs = (nd - np.float64(1.0)) * ((a * (nd * nd)) + (r * s2))
    return (lhs <= rhs).all(axis=-1)


_cache = {}


def _yardstick(rl, name, S, F):
    """Scene, the camera at S samples, and the moments renders of every checkpoint and of S at first_sample F — built once, with the
    switches at their defaults, and never written to afterwards.  Also the two rules' bounds, from the last checkpoint."""
    key = (name, S, F)
    if key not in _cache:
        rl.api.set_coop(True), rl.api.set_fast_traversal(True), rl.api.set_lpt(True)
        world, cam = _scene(rl, name, S)
        at = {}
        for k in _checkpoints(S) + [S]:
            m = rl.Camera(dataclasses.replace(cam.params, samples_per_pixel=k)).render_moments(world, first_sample=F, allow_degenerate=True)
            m.sums.setflags(write=False), m.sq.setflags(write=False)
            at[k] = (m.sums, m.sq)
        n = _checkpoints(S)[-1]
        s, q = at[n]
        var = (n * q - s * s) / (n * n * (n - 1))  # per channel: the variance of the mean at the last checkpoint
        abs_v = float(np.median(var.max(axis=-1)))
        nz = (s != 0).all(axis=-1)
        assert nz.any(), (name, "no pixel with all sums nonzero")
        rel_v = float(np.median((var[nz] / (s[nz] * s[nz] / (n * n))).max(axis=-1)))
        assert abs_v >= 0 and rel_v >= 0 and np.isfinite(abs_v) and np.isfinite(rel_v)
        _cache[key] = {"world": world, "cam": cam, "at": at, "rules": {"abs": (abs_v, 0.0), "rel": (0.0, rel_v)}}
    return _cache[key]


def _expected(Y, S, a, r):
    """(counts, sums, sq) the rule (a, r) must give, from the yardstick's renders."""
    s_end, q_end = Y["at"][S]
    counts = np.full(s_end.shape[:2], S, dtype=np.uint32)
    sums, sq = s_end.copy(), q_end.copy()
    running = np.ones(counts.shape, dtype=bool)
    for k in _checkpoints(S):
        s, q = Y["at"][k]
        stop = running & _ok(k, s, q, a, r)
        counts[stop], sums[stop], sq[stop] = k, s[stop], q[stop]
        running &= ~stop
    return counts, sums, sq


def _device(rl, cam, world, a, r, first_sample=0, row_first=0, row_step=1, min_samples=MIN, check_every=EVERY):
    """render_adaptive_device into NaN-filled / 0xFFFFFFFF-filled device buffers on a stream of its own -> (sums, sq, counts) on the host."""
    import torch
    dev = torch.device("cuda", 0)
    nrows = rl.api.rows_for(cam.c.image_height, row_first, row_step)
    d_s = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    d_q = torch.full((nrows, cam.c.image_width, 3), float("nan"), dtype=torch.float64, device=dev)
    d_n = torch.full((nrows, cam.c.image_width), -1, dtype=torch.int32, device=dev)
    stream = torch.cuda.Stream(dev)
    torch.cuda.synchronize(dev)
    cam.render_adaptive_device(world, min_samples, check_every, d_s.data_ptr(), d_q.data_ptr(), d_n.data_ptr(), abs_variance=a, rel_variance=r,
                               stream=stream.cuda_stream, row_first=row_first, row_step=row_step, first_sample=first_sample)
    rl.api.render_status(world, allow_degenerate=True)
    torch.cuda.synchronize(dev)
    return d_s.cpu().numpy(), d_q.cpu().numpy(), d_n.cpu().numpy().view(np.uint32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _check(got, want, what):
    """Counts first (the message then names the wrong stop), then both moments, byte for byte; every element written."""
    sums, sq, counts = got
    w_counts, w_sums, w_sq = want
    assert not (counts == 0xFFFFFFFF).any() and not np.isnan(sums).any() and not np.isnan(sq).any(), (what, "not fully written")
    assert _same(counts, w_counts), (what, "counts", np.argwhere(counts != w_counts)[:4].tolist(), counts[counts != w_counts][:4], w_counts[counts != w_counts][:4])
    assert _same(sums, w_sums), (what, "sums")
    assert _same(sq, w_sq), (what, "sq")


def _restore(rl):
    rl.api.set_coop(True), rl.api.set_fast_traversal(True), rl.api.set_lpt(True)


@pytest.mark.parametrize("name", SCENES)
def test_every_route_stops_where_the_yardstick_stops(rl, name):
    """Case 1: S = 24, checkpoints 4, 8, ..., 20, first_sample 0 and 3, the abs and the rel rule, the device form on every route."""
    S = 24
    for F in (0, 3):
        Y = _yardstick(rl, name, S, F)
        world, cam = Y["world"], Y["cam"]
        for rule, (a, r) in Y["rules"].items():
            want = _expected(Y, S, a, r)
            vals = set(np.unique(want[0]).tolist())
            print(name, F, rule, (a, r), {int(v): int((want[0] == v).sum()) for v in sorted(vals)})
            if name in SPHERE_SCENES:  # the condition that lets the test see a wrong stop
                assert len(vals) >= 3 and MIN in vals and S in vals, (name, F, rule, sorted(vals))
            try:
                for coop, fast in _routes(name):
                    rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
                    _check(_device(rl, cam, world, a, r, first_sample=F), want, (name, F, rule, coop, fast))
            finally:
                _restore(rl)
        # the counting host form (the reference-order kernel), once per F
        a, r = Y["rules"]["abs"]
        got = cam.render_adaptive(world, MIN, EVERY, abs_variance=a, first_sample=F, allow_degenerate=True)
        _check((got.sums, got.sq, got.counts), _expected(Y, S, a, r), (name, F, "host form"))


@pytest.mark.parametrize("name", ["bouncing_spheres", "cornell_smoke"])
def test_two_launch_render_stops_where_the_single_launch_stops(rl, name):
    """Case 2: S = 72 takes the cost-sorted two-launch render (samples [0, 8), sort, resume) with set_lpt(True) and a single launch with
    set_lpt(False).  A pixel that stopped in the first launch (counts 4 and 8) must not be resumed, and one that goes on must count from its
    true n: both settings equal the yardstick, whose counts hold values below 8, equal to 8 and above 8."""
    S = 72
    Y = _yardstick(rl, name, S, 0)
    world, cam = Y["world"], Y["cam"]
    for rule, (a, r) in Y["rules"].items():
        want = _expected(Y, S, a, r)
        counts = want[0]
        print(name, rule, (a, r), {int(v): int((counts == v).sum()) for v in np.unique(counts)})
        assert (counts < 8).any() and (counts == 8).any() and (counts > 8).any(), (name, rule, np.unique(counts).tolist())
        try:
            for coop, fast in _routes(name):
                for lpt in (True, False):
                    rl.api.set_coop(coop), rl.api.set_fast_traversal(fast), rl.api.set_lpt(lpt)
                    _check(_device(rl, cam, world, a, r), want, (name, rule, coop, fast, "lpt", lpt))
        finally:
            _restore(rl)
    # the counting host form through both as well
    a, r = Y["rules"]["abs"]
    want = _expected(Y, S, a, r)
    try:
        for lpt in (True, False):
            rl.api.set_lpt(lpt)
            got = cam.render_adaptive(world, MIN, EVERY, abs_variance=a, allow_degenerate=True)
            _check((got.sums, got.sq, got.counts), want, (name, "host form, lpt", lpt))
    finally:
        _restore(rl)


@pytest.mark.parametrize("name", SCENES)
def test_row_shards_are_rows_of_the_full_result(rl, name):
    """Case 3: row_first = 1, row_step = 3 gives rows 1, 4, 7, ... of the full result's sums, sq and counts."""
    S = 24
    Y = _yardstick(rl, name, S, 0)
    world, cam = Y["world"], Y["cam"]
    a, r = Y["rules"]["abs"]
    counts, sums, sq = _expected(Y, S, a, r)
    want = (counts[1::3], sums[1::3], sq[1::3])
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            got = _device(rl, cam, world, a, r, row_first=1, row_step=3)
            assert got[0].shape[0] == len(range(1, cam.c.image_height, 3))
            _check(got, want, (name, coop, fast))
    finally:
        _restore(rl)
    got = cam.render_adaptive(world, MIN, EVERY, abs_variance=a, row_first=1, row_step=3, allow_degenerate=True)
    _check((got.sums, got.sq, got.counts), want, (name, "host form"))


@pytest.mark.parametrize("name", SCENES)
def test_no_checkpoint_is_the_moments_call_and_zero_bounds_stop_only_exact_pixels(rl, name):
    """Case 4: min_samples >= S never reaches a checkpoint: render_moments' bytes, counts all S.  With abs_variance = rel_variance = 0 only
    pixels with lhs <= 0 stop — still the yardstick."""
    S = 24
    Y = _yardstick(rl, name, S, 0)
    world, cam = Y["world"], Y["cam"]
    s_end, q_end = Y["at"][S]
    full = (np.full(s_end.shape[:2], S, dtype=np.uint32), s_end, q_end)
    zero = _expected(Y, S, 0.0, 0.0)
    print(name, "zero bounds", {int(v): int((zero[0] == v).sum()) for v in np.unique(zero[0])})
    try:
        for coop, fast in _routes(name):
            rl.api.set_coop(coop), rl.api.set_fast_traversal(fast)
            for m in (S, S + 5):
                _check(_device(rl, cam, world, 1e300, 1e300, min_samples=m), full, (name, coop, fast, "min_samples", m))
            _check(_device(rl, cam, world, 0.0, 0.0), zero, (name, coop, fast, "zero bounds"))
    finally:
        _restore(rl)
    m = cam.render_moments(world, allow_degenerate=True)
    assert _same(m.sums, s_end) and _same(m.sq, q_end)


@pytest.mark.parametrize("name", SCENES)
def test_counters_are_those_of_the_samples_rendered(rl, name):
    """Cases 5 and 6: the _rows form's seven counters equal the sum, over the distinct count values k, of Camera(samples_per_pixel=k)
    .render_pixels(..., stats) on the pixels that have that count; and the call's sums and sq equal render_pixels_moments of each group."""
    S = 24
    Y = _yardstick(rl, name, S, 3)
    world, cam = Y["world"], Y["cam"]
    a, r = Y["rules"]["abs"]
    gs = {}
    got = cam.render_adaptive(world, MIN, EVERY, abs_variance=a, first_sample=3, stats=gs, allow_degenerate=True)
    _check((got.sums, got.sq, got.counts), _expected(Y, S, a, r), (name, "host form"))
    total = dict.fromkeys(COUNTERS, 0)
    for k in np.unique(got.counts):
        ys, xs = np.nonzero(got.counts == k)
        camk = rl.Camera(dataclasses.replace(cam.params, samples_per_pixel=int(k)))
        ps = {}
        plain = camk.render_pixels(world, xs, ys, first_sample=3, stats=ps, allow_degenerate=True)
        for c in COUNTERS:
            total[c] += ps[c]
        lsums, lsq = camk.render_pixels_moments(world, xs, ys, first_sample=3, allow_degenerate=True)
        assert _same(got.sums[ys, xs], plain) and _same(got.sums[ys, xs], lsums) and _same(got.sq[ys, xs], lsq), (name, int(k))
    for c in COUNTERS:
        assert gs[c] == total[c], (name, c, gs[c], total[c])
    assert gs["rays"] > 0 and gs["rng_words"] > 0
    # the device form with stats is synchronous and counts too
    import torch
    d_s = torch.zeros((cam.c.image_height, cam.c.image_width, 3), dtype=torch.float64, device="cuda:0")
    d_q = torch.zeros_like(d_s)
    d_n = torch.zeros((cam.c.image_height, cam.c.image_width), dtype=torch.int32, device="cuda:0")
    ds = {}
    cam.render_adaptive_device(world, MIN, EVERY, d_s.data_ptr(), d_q.data_ptr(), d_n.data_ptr(), abs_variance=a, first_sample=3, stats=ds)
    for c in COUNTERS:
        assert ds[c] == total[c], (name, "device form", c, ds[c], total[c])
    assert _same(d_n.cpu().numpy().view(np.uint32), got.counts)


def test_invalid_rules_and_null_buffers_touch_nothing_on_the_device(rl):
    api = rl.api
    lib = api.render_lib()
    Y = _yardstick(rl, "golden_test_scene", 24, 0)
    world, cam = Y["world"], Y["cam"]
    npix = cam.c.image_width * cam.c.image_height
    s, q, n = np.full(npix * 3, np.nan), np.full(npix * 3, np.nan), np.full(npix, 0xFFFFFFFF, dtype=np.uint32)
    c = C.byref(cam.c)
    R = api.RtiowAdaptive
    good = R(4, 4, 1.0, 0.0)
    for rule in (R(1, 4, 1.0, 0.0), R(4, 0, 1.0, 0.0), R(4, 4, -1.0, 0.0), R(4, 4, 0.0, float("nan"))):
        assert lib.rl_rtiow_render_adaptive_rows(world.device(), c, 0, 0, 1, C.byref(rule), s.ctypes.data, q.ctypes.data, n.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_adaptive_rows(world.device(), c, 0, 0, 1, None, s.ctypes.data, q.ctypes.data, n.ctypes.data, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_adaptive_rows(world.device(), c, 0, 0, 1, C.byref(good), s.ctypes.data, q.ctypes.data, None, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_adaptive_rows(world.device(), c, 0, 0, 0, C.byref(good), s.ctypes.data, q.ctypes.data, n.ctypes.data, None) == api.RL_E_INVALID  # row_step 0
    rw = rl.RtcWorld.test_csg_scene(24, 16)
    assert lib.rl_rtiow_render_adaptive_rows(rw.device(), c, 0, 0, 1, C.byref(good), s.ctypes.data, q.ctypes.data, n.ctypes.data, None) == api.RL_E_INVALID  # an RTC scene
    st = api.Stats()
    st.rays = 77  # row_first past the last row: RL_OK, nothing touched, the stats zeroed
    assert lib.rl_rtiow_render_adaptive_rows(world.device(), c, 0, cam.c.image_height, 1, C.byref(good), s.ctypes.data, q.ctypes.data, n.ctypes.data,
                                             C.byref(st)) == api.RL_OK and st.rays == 0
    assert np.isnan(s).all() and np.isnan(q).all() and (n == 0xFFFFFFFF).all()


def test_cpp_mirror_renders_adaptive(rl):
    H = rl.api.host_lib()
    H.rlh_render_adaptive_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    # the mirror's golden_test_scene at the test's width and samples, with its own max_depth: compare with a camera of that depth
    world = rl.World.golden_test_scene()
    cam = rl.Camera(dataclasses.replace(world.params, image_width=24, samples_per_pixel=24))
    W, Hh = cam.c.image_width, cam.c.image_height
    a = _yardstick(rl, "golden_test_scene", 24, 0)["rules"]["abs"][0]
    want = cam.render_adaptive(world, MIN, EVERY, abs_variance=a)
    assert len(np.unique(want.counts)) >= 2
    sums, sq, counts = np.zeros((Hh, W, 3)), np.zeros((Hh, W, 3)), np.zeros((Hh, W), dtype=np.uint32)
    assert H.rlh_render_adaptive_probe(W, 24, MIN, EVERY, a, 0.0, sums.ctypes.data, sq.ctypes.data, counts.ctypes.data) == 0, H.rlh_last_error()
    assert _same(sums, want.sums) and _same(sq, want.sq) and _same(counts, want.counts)
