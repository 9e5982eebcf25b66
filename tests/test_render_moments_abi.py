"""CPU tier: the renders with second moments (rl_rtiow_render_moments_rows / _device, rl_rtiow_render_pixels_moments / _device; include/rl_render.h
"Second moments") are exported, declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and
C++ layers, and fail LOUDLY (RL_E_NO_DEVICE, no CPU fallback) when no GPU is present; api.Moments' host arithmetic on hand-made arrays."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_moments_rows": 8, "rl_rtiow_render_moments_device": 9, "rl_rtiow_render_pixels_moments": 9, "rl_rtiow_render_pixels_moments_device": 10}
PROBE_ARGS = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p]


def test_render_moments_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_render_moments_probe")
    for m in ("render_moments", "render_moments_device", "render_pixels_moments", "render_pixels_moments_device"):
        assert callable(getattr(rl.Camera, m)), m
    assert rl.Moments is rl.api.Moments


def test_shape_errors_are_caught_before_the_library(rl):
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    for xs, ys in (([0, 1, 2], [0, 1]),                                  # unequal lengths
                   (np.array([0.0, 1.0]), np.array([0, 1])),            # not integers
                   (np.array([0, 1]), np.array([0.5, 1.0])),
                   (np.array([0, -1]), np.array([0, 1])),               # negative
                   (np.array([0, 1]), np.array([-3, 1], dtype=np.int64)),
                   (np.array([0, 1 << 32], dtype=np.int64), np.array([0, 1])),  # beyond a uint32
                   (np.zeros((2, 2), dtype=np.uint32), np.zeros((2, 2), dtype=np.uint32))):  # not a list
        with pytest.raises(ValueError):
            cam.render_pixels_moments(world, xs, ys)


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_render_moments_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    for call in (lambda: cam.render_moments(world),
                 lambda: cam.render_moments(world, first_sample=3, row_first=1, row_step=3, stats={}),
                 lambda: cam.render_moments_device(world, 0x1000, 0x2000),
                 lambda: cam.render_pixels_moments(world, [0, 1], [0, 1]),
                 lambda: cam.render_pixels_moments(world, [0, 1], [0, 1], stats={}),
                 lambda: cam.render_pixels_moments_device(world, 0x1000, 0x2000, 2, 0x3000, 0x4000)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers: both outputs untouched
    xs, ys = np.array([0, 1], dtype=np.uint32), np.array([0, 1], dtype=np.uint32)
    n = cam.c.image_width * cam.c.image_height * 3
    sums, sq = np.zeros(n), np.zeros(n)
    c = ctypes.byref(cam.c)
    assert lib.rl_rtiow_render_moments_rows(None, c, 0, 0, 1, sums.ctypes.data, sq.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_render_moments_device(None, c, 0, 0, 1, sums.ctypes.data, sq.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_render_pixels_moments(None, c, 0, xs.ctypes.data, ys.ctypes.data, 2, sums.ctypes.data, sq.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_render_pixels_moments_device(None, c, 0, xs.ctypes.data, ys.ctypes.data, 2, sums.ctypes.data, sq.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert not sums.any() and not sq.any()
    # the C++ mirror reaches the same wall, frame and list
    H = api.host_lib()
    H.rlh_render_moments_probe.argtypes = PROBE_ARGS
    assert H.rlh_render_moments_probe(12, 2, None, None, 0, sums.ctypes.data, sq.ctypes.data) == -1
    assert H.rlh_render_moments_probe(12, 2, xs.ctypes.data, ys.ctypes.data, 2, sums.ctypes.data, sq.ctypes.data) == -1
    assert not sums.any() and not sq.any()


def test_moments_merge_canvas_and_variance_of_mean_on_hand_made_arrays(rl):
    Moments = rl.api.Moments
    # two pixels, samples {1, 2, 3, 4} in channel 0, {2, 2, 2, 2} in channel 1, {0, 0, 0, 8} in channel 2; second pixel all zero
    a = Moments(2, np.array([[[3.0, 4.0, 0.0], [0.0, 0.0, 0.0]]]), np.array([[[5.0, 8.0, 0.0], [0.0, 0.0, 0.0]]]))     # samples 1, 2
    b = Moments(2, np.array([[[7.0, 4.0, 8.0], [0.0, 0.0, 0.0]]]), np.array([[[25.0, 8.0, 64.0], [0.0, 0.0, 0.0]]]))  # samples 3, 4
    m = a.merge(b)
    assert m.samples == 4
    assert m.sums.tobytes() == np.array([[[10.0, 8.0, 8.0], [0.0, 0.0, 0.0]]]).tobytes()
    assert m.sq.tobytes() == np.array([[[30.0, 16.0, 64.0], [0.0, 0.0, 0.0]]]).tobytes()
    cv = m.canvas()
    assert (cv.samples, cv.width, cv.height) == (4, 2, 1) and cv.data is m.sums
    # sample variances 5/3, 0, 16 over n = 4: exact in binary64 up to the one division by 3
    want = np.array([[[(30.0 - 100.0 / 4) / 3 / 4, 0.0, (64.0 - 64.0 / 4) / 3 / 4], [0.0, 0.0, 0.0]]])
    assert m.variance_of_mean().tobytes() == want.tobytes()
    assert want[0, 0, 2] == 4.0 and want[0, 0, 1] == 0.0
    # n < 2 has no sample variance
    for n in (0, 1):
        with pytest.raises(ValueError):
            Moments(n, np.zeros((1, 1, 3)), np.zeros((1, 1, 3))).variance_of_mean()
    # round-off: three equal samples of 0.1 — sq = fl(fl(0.01 + 0.01) + 0.01) and sums^2 / 3 differ by an ulp or so either way; never negative
    c = np.float64(0.1)
    s1 = (c + c) + c
    q1 = (c * c + c * c) + c * c
    neg = Moments(3, np.array([[[s1, 0.3, 1e8 + 1.0]]]), np.array([[[q1, 0.03 - 1e-17, (1e8 + 1.0) ** 2 / 3 * (1 - 2e-16)]]]))
    raw = (neg.sq - neg.sums * neg.sums / 3) / 2 / 3
    assert (raw < 0).any()  # the un-clipped formula does go below zero here
    v = neg.variance_of_mean()
    assert (v >= 0).all() and v[raw < 0].tobytes() == np.zeros(int((raw < 0).sum())).tobytes()
