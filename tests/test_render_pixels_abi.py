"""CPU tier: the pixel-list render entry points (rl_rtiow_render_pixels, rl_rtc_render_pixels and their _device forms) are exported,
declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers, and fail LOUDLY (RL_E_NO_DEVICE, no
CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_pixels": 8, "rl_rtiow_render_pixels_device": 9, "rl_rtc_render_pixels": 8, "rl_rtc_render_pixels_device": 9}
PROBE_ARGS = [ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]


def test_render_pixels_entry_points_are_exported_declared_and_listed(rl):
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
    assert hasattr(rl.api.host_lib(), "rlh_render_pixels_probe")
    for cls in (rl.Camera, rl.RtcWorld):
        for m in ("render_pixels", "render_pixels_device"):
            assert callable(getattr(cls, m)), (cls, m)


def test_shape_errors_are_caught_before_the_library(rl):
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    rw = rl.RtcWorld.test_mirror_scene(12, 8)
    for render in (lambda xs, ys: cam.render_pixels(world, xs, ys), lambda xs, ys: rw.render_pixels(xs, ys)):
        for xs, ys in (([0, 1, 2], [0, 1]),                                  # unequal lengths
                       (np.array([0.0, 1.0]), np.array([0, 1])),            # not integers
                       (np.array([0, 1]), np.array([0.5, 1.0])),
                       (np.array([0, -1]), np.array([0, 1])),               # negative
                       (np.array([0, 1]), np.array([-3, 1], dtype=np.int64)),
                       (np.array([0, 1 << 32], dtype=np.int64), np.array([0, 1])),  # beyond a uint32
                       (np.zeros((2, 2), dtype=np.uint32), np.zeros((2, 2), dtype=np.uint32))):  # not a list
            with pytest.raises(ValueError):
                render(xs, ys)


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_render_pixels_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    rw = rl.RtcWorld.test_mirror_scene(12, 8)
    for call in (lambda: cam.render_pixels(world, [0, 1], [0, 1]),
                 lambda: cam.render_pixels(world, [0, 1], [0, 1], stats={}),
                 lambda: cam.render_pixels_device(world, 0x1000, 0x2000, 2, 0x3000),
                 lambda: rw.render_pixels([0, 1], [0, 1]),
                 lambda: rw.render_pixels_device(0x1000, 0x2000, 2, 0x3000)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    xs, ys, out = np.array([0, 1], dtype=np.uint32), np.array([0, 1], dtype=np.uint32), np.zeros((2, 3))
    assert lib.rl_rtiow_render_pixels(None, ctypes.byref(cam.c), 0, xs.ctypes.data, ys.ctypes.data, 2, out.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_render_pixels_device(None, ctypes.byref(cam.c), 0, xs.ctypes.data, ys.ctypes.data, 2, out.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_render_pixels(None, ctypes.byref(rw.camera), 1, xs.ctypes.data, ys.ctypes.data, 2, out.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_render_pixels_device(None, ctypes.byref(rw.camera), 1, xs.ctypes.data, ys.ctypes.data, 2, out.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert not out.any()
    # the C++ mirror reaches the same wall, in both families
    H = api.host_lib()
    H.rlh_render_pixels_probe.argtypes = PROBE_ARGS
    for family in (0, 1):
        assert H.rlh_render_pixels_probe(family, 12, 1, xs.ctypes.data, ys.ctypes.data, 2, out.ctypes.data) == -1
