"""GPU tier: what the host-buffer forms of the renders do around their _device forms (csrc/rl_host_api.h), seen through the C ABI itself.
The Python wrappers always pass a zeroed rl_stats and a scene of the right family, so they cannot observe

  * that a rows form returns the bytes its _device form leaves in device memory, for the frame, the sample-parallel and the RTC render;
  * that accumulate = 1 continues the caller's sums, and that the _rgb8 forms are the _device render followed by the device encode;
  * that row_first == height touches no buffer and zeroes opt_stats, and that a scene of the other family is refused with the
    buffer and opt_stats left as they were;
  * that the pixels do not depend on whether opt_stats was passed.

Shapes: the golden test scene at 5x3, 2 samples, depth 3 and the mirror scene at 6x4, aa 1 — the whole frame, and the row set
row_first = 1, row_step = 2 (one row of the 5x3 frame, two of the 6x4 one)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROW_SETS = [(0, 1), (1, 2)]
COUNTERS = ("rays", "node_tests", "sphere_tests", "planar_tests", "instance_enters", "rng_words", "flagged")
FILL = -7.25  # what an untouched f64 buffer holds


def _ff_stats(api):
    st = api.Stats()
    assert C.sizeof(st) == 64
    C.memset(C.byref(st), 0xFF, 64)
    return st


def _stats_bytes(st):
    return bytes((C.c_ubyte * 64).from_buffer_copy(st))


@pytest.fixture(scope="module")
def scenes(rl):
    rl.init(0)
    world = rl.World.golden_test_scene()
    p = dataclasses.replace(world.params, aspect_ratio=1.6, image_width=5, samples_per_pixel=2, max_depth=3)
    cam = rl.Camera(p)
    assert (cam.c.image_width, cam.c.image_height) == (5, 3)
    mirror = rl.RtcWorld.test_mirror_scene(6, 4)
    assert (mirror.camera.hsize, mirror.camera.vsize) == (6, 4)
    return dict(world=world, rt=world.device(), cam=cam.c, mirror=mirror, rc=mirror.device(), rcam=mirror.camera)


def _forms(rl, s):
    """name -> (height, width, rows form(row_first, row_step, out pointer, stats), _device form(..., device pointer, stream, stats))"""
    lib = rl.api.render_lib()
    rt, cam, rc, rcam = s["rt"], C.byref(s["cam"]), s["rc"], C.byref(s["rcam"])
    return {
        "frame": (3, 5, lambda rf, rs, out, st: lib.rl_rtiow_render_rows(rt, cam, 0, rf, rs, out, st),
                  lambda rf, rs, d, stream, st: lib.rl_rtiow_render_device(rt, cam, 0, rf, rs, d, stream, st)),
        "independent": (3, 5, lambda rf, rs, out, st: lib.rl_rtiow_render_independent_rows(rt, cam, 0, rf, rs, 0, out, st),
                        lambda rf, rs, d, stream, st: lib.rl_rtiow_render_independent_device(rt, cam, 0, rf, rs, 0, d, stream, st)),
        "rtc": (4, 6, lambda rf, rs, out, st: lib.rl_rtc_render_rows(rc, rcam, 1, rf, rs, out, st),
                lambda rf, rs, d, stream, st: lib.rl_rtc_render_device(rc, rcam, 1, rf, rs, d, stream, st)),
    }


def _device_buffer(shape, dtype, fill):
    import torch
    return torch.full(shape, fill, dtype=dtype, device="cuda:0"), torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("rows", ROW_SETS)
@pytest.mark.parametrize("name", ["frame", "independent", "rtc"])
def test_rows_form_returns_its_device_forms_buffer(rl, scenes, name, rows):
    import torch
    api = rl.api
    H, W, host, device = _forms(rl, scenes)[name]
    nrows = api.rows_for(H, *rows)
    assert nrows == {(0, 1): H, (1, 2): H // 2}[rows]
    buf, stream = _device_buffer((nrows, W, 3), torch.float64, FILL)
    ds = _ff_stats(api)
    assert device(*rows, buf.data_ptr(), stream, C.byref(ds)) == api.RL_OK
    want = buf.cpu().numpy()
    assert np.isfinite(want).all() and (want != FILL).all() and want.any()
    out, hs = np.full((nrows, W, 3), FILL), _ff_stats(api)
    assert host(*rows, out.ctypes.data, C.byref(hs)) == api.RL_OK
    assert out.tobytes() == want.tobytes()
    for k in COUNTERS:
        assert getattr(hs, k) == getattr(ds, k), k
    assert hs.rays > 0 and 0.0 <= hs.kernel_ms < 60e3
    bare = np.full((nrows, W, 3), FILL)  # opt_stats NULL: the same pixels
    assert host(*rows, bare.ctypes.data, None) == api.RL_OK
    assert bare.tobytes() == want.tobytes()
    # and the asynchronous _device form (opt_stats NULL) leaves them too
    buf2, stream = _device_buffer((nrows, W, 3), torch.float64, FILL)
    assert device(*rows, buf2.data_ptr(), stream, None) == api.RL_OK
    st = api.render_status(scenes["world"] if name != "rtc" else scenes["mirror"])
    assert buf2.cpu().numpy().tobytes() == want.tobytes() and st["rays"] == ds.rays


def test_whole_frame_forms_are_the_rows_forms_from_row_zero(rl, scenes):
    api, lib = rl.api, rl.api.render_lib()
    forms = _forms(rl, scenes)
    for name, call in (("frame", lambda out, st: lib.rl_rtiow_render(scenes["rt"], C.byref(scenes["cam"]), 0, out, st)),
                       ("rtc", lambda out, st: lib.rl_rtc_render(scenes["rc"], C.byref(scenes["rcam"]), 1, out, st))):
        H, W, host, _ = forms[name]
        want, got = np.full((H, W, 3), FILL), np.full((H, W, 3), FILL)
        assert host(0, 1, want.ctypes.data, None) == api.RL_OK
        st = _ff_stats(api)
        assert call(got.ctypes.data, C.byref(st)) == api.RL_OK
        assert got.tobytes() == want.tobytes() and st.rays > 0, name


@pytest.mark.parametrize("rows", ROW_SETS)
def test_accumulate_continues_the_callers_sums(rl, scenes, rows):
    """accumulate = 1 folds the samples into the caller's sums left to right, ((p + c0) + c1), where accumulate = 0 returns
    (0 + c0) + c1 = c0 + c1.  Every term is >= 0, so each of the two roundings on either side is a relative error of at most
    u = 2^-53 of the exact total T: |((p + c0) + c1) - (p + (c0 + c1))| <= 2 ((1 + u)^2 - 1) T <= 4 u (1 + u) T.  The bit-exact
    composition of two real renders is tests/test_gpu_independent_samples.py's."""
    api, lib = rl.api, rl.api.render_lib()
    rt, cam = scenes["rt"], C.byref(scenes["cam"])
    nrows = api.rows_for(3, *rows)
    fresh = np.full((nrows, 5, 3), FILL)
    assert lib.rl_rtiow_render_independent_rows(rt, cam, 0, *rows, 0, fresh.ctypes.data, None) == api.RL_OK
    assert (fresh >= 0.0).all() and fresh.any()
    pre = 0.5 + np.arange(fresh.size, dtype=np.float64).reshape(fresh.shape) / 3.0
    sums = pre.copy()
    assert lib.rl_rtiow_render_independent_rows(rt, cam, 0, *rows, 1, sums.ctypes.data, None) == api.RL_OK
    want = pre + fresh
    u = 2.0 ** -53
    err = np.abs(sums - want)
    print("accumulate: max |difference| / (u T) =", float((err / (u * want)).max()))
    assert (err <= 4 * u * (1 + 4 * u) * want).all()
    assert not np.array_equal(sums, fresh)


def test_rgb8_forms_are_the_device_render_followed_by_the_device_encode(rl, scenes):
    import torch
    api, lib = rl.api, rl.api.render_lib()
    rt, cam, rc, rcam = scenes["rt"], scenes["cam"], scenes["rc"], scenes["rcam"]
    cases = {
        "rtiow": (3, 5, lambda out, st: lib.rl_rtiow_render_rgb8(rt, C.byref(cam), 0, out, st),
                  lambda d, stream: lib.rl_rtiow_render_device(rt, C.byref(cam), 0, 0, 1, d, stream, None),
                  lambda d, d8, stream: lib.rl_rtiow_encode_rgb8_device(d, 15, cam.samples_per_pixel, d8, stream)),
        "rtc": (4, 6, lambda out, st: lib.rl_rtc_render_rgb8(rc, C.byref(rcam), 1, out, st),
                lambda d, stream: lib.rl_rtc_render_device(rc, C.byref(rcam), 1, 0, 1, d, stream, None),
                lambda d, d8, stream: lib.rl_rtc_encode_rgb8_device(d, 24, d8, stream)),
    }
    for name, (H, W, rgb8, render, encode) in cases.items():
        buf, stream = _device_buffer((H, W, 3), torch.float64, FILL)
        u8, _ = _device_buffer((H, W, 3), torch.uint8, 0xAB)
        assert render(buf.data_ptr(), stream) == api.RL_OK
        assert encode(buf.data_ptr(), u8.data_ptr(), stream) == api.RL_OK
        torch.cuda.synchronize()
        want = u8.cpu().numpy()
        assert len(np.unique(want)) > 2, name
        st = _ff_stats(api)
        got, bare = np.full((H, W, 3), 0xAB, dtype=np.uint8), np.full((H, W, 3), 0xAB, dtype=np.uint8)
        assert rgb8(got.ctypes.data, C.byref(st)) == api.RL_OK
        assert rgb8(bare.ctypes.data, None) == api.RL_OK
        assert got.tobytes() == want.tobytes() and bare.tobytes() == want.tobytes(), name
        assert st.rays > 0 and st.flagged == 0, name
        api.render_status(scenes["world"] if name == "rtiow" else scenes["mirror"])  # collect the asynchronous render above


@pytest.mark.parametrize("name", ["frame", "independent", "rtc"])
def test_row_first_at_the_height_touches_nothing_and_zeroes_opt_stats(rl, scenes, name):
    api = rl.api
    H, W, host, _ = _forms(rl, scenes)[name]
    out, st = np.full((1, W, 3), FILL), _ff_stats(api)
    assert host(H, 1, out.ctypes.data, C.byref(st)) == api.RL_OK
    assert (out == FILL).all() and _stats_bytes(st) == bytes(64)
    assert host(H, 1, out.ctypes.data, None) == api.RL_OK
    assert (out == FILL).all()


def test_a_scene_of_the_other_family_is_refused_before_anything_is_written(rl, scenes):
    api, lib = rl.api, rl.api.render_lib()
    rt, cam, rc, rcam = scenes["rt"], C.byref(scenes["cam"]), scenes["rc"], C.byref(scenes["rcam"])
    calls = {  # every host form, with the other family's scene
        "rtiow_render": lambda out, st: lib.rl_rtiow_render(rc, cam, 0, out, st),
        "rtiow_render_rows": lambda out, st: lib.rl_rtiow_render_rows(rc, cam, 0, 1, 2, out, st),
        "rtiow_render_independent_rows": lambda out, st: lib.rl_rtiow_render_independent_rows(rc, cam, 0, 1, 2, 0, out, st),
        "rtiow_render_independent_rows, accumulate": lambda out, st: lib.rl_rtiow_render_independent_rows(rc, cam, 0, 0, 1, 1, out, st),
        "rtiow_render_rgb8": lambda out, st: lib.rl_rtiow_render_rgb8(rc, cam, 0, out, st),
        "rtiow_render_multi": lambda out, st: lib.rl_rtiow_render_multi(rc, cam, 0, out, st),
        "rtc_render": lambda out, st: lib.rl_rtc_render(rt, rcam, 1, out, st),
        "rtc_render_rows": lambda out, st: lib.rl_rtc_render_rows(rt, rcam, 1, 1, 2, out, st),
        "rtc_render_rgb8": lambda out, st: lib.rl_rtc_render_rgb8(rt, rcam, 1, out, st),
        "rtc_render_multi": lambda out, st: lib.rl_rtc_render_multi(rt, rcam, 1, out, st),
    }
    for name, call in calls.items():
        out = np.full((4, 6, 3), FILL)  # room for either family's frame, in doubles
        st = _ff_stats(api)
        assert call(out.ctypes.data, C.byref(st)) == api.RL_E_INVALID, name
        assert _stats_bytes(st) == b"\xff" * 64, name
        assert (out == FILL).all(), name
        assert call(out.ctypes.data, None) == api.RL_E_INVALID, name
    # ... also for a render of no rows
    out, st = np.full((1, 6, 3), FILL), _ff_stats(api)
    assert lib.rl_rtiow_render_rows(rc, cam, 0, 3, 1, out.ctypes.data, C.byref(st)) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_independent_rows(rc, cam, 0, 3, 1, 0, out.ctypes.data, C.byref(st)) == api.RL_E_INVALID
    assert lib.rl_rtc_render_rows(rt, rcam, 1, 4, 1, out.ctypes.data, C.byref(st)) == api.RL_E_INVALID
    assert _stats_bytes(st) == b"\xff" * 64 and (out == FILL).all()
