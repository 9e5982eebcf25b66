"""CPU tier: the batched ray-query entry points (rl_rtiow_hit_rays, rl_rtc_intersect_rays, rl_rtc_color_at_rays and their _device forms)
are exported, declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers, and fail LOUDLY
(RL_E_NO_DEVICE, no CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_hit_rays": 7, "rl_rtiow_hit_rays_device": 8, "rl_rtc_intersect_rays": 8, "rl_rtc_intersect_rays_device": 9,
       "rl_rtc_color_at_rays": 5, "rl_rtc_color_at_rays_device": 6}


def test_query_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_ray_query_probe")
    for m in ("hit_rays", "hit_rays_device"):
        assert callable(getattr(rl.World, m)), m
    for m in ("intersect_rays", "intersect_rays_device", "color_at_rays", "color_at_rays_device"):
        assert callable(getattr(rl.RtcWorld, m)), m


def test_query_record_layouts_match_header(rl):
    api = rl.api
    assert api.RAY.itemsize == 56 and api.RTIOW_HIT.itemsize == 88 and api.RTC_ISECT.itemsize == 40
    assert api.RTIOW_HIT.fields["hit"][1] == 72 and api.RTIOW_HIT.fields["material"][1] == 80
    assert api.RTC_ISECT.fields["object"][1] == 32
    assert api.NO_HIT == 0xFFFFFFFF


def test_ray_shape_errors_are_caught_before_the_library(rl):
    api = rl.api
    with pytest.raises(ValueError):
        api.pack_rays(np.zeros((4, 3)), np.zeros((5, 3)))
    with pytest.raises(ValueError):
        api.pack_rays(np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        api.pack_rays(np.zeros((4, 3)), np.zeros((4, 3)), times=np.zeros(3))
    r = api.pack_rays([[1, 2, 3]], [[0, 0, -1]], times=[0.5])
    assert r.dtype == api.RAY and tuple(r["origin"][0]) == (1.0, 2.0, 3.0) and tuple(r["dir"][0]) == (0.0, 0.0, -1.0) and r["time"][0] == 0.5


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_queries_without_a_device_fail_loudly(rl, golden):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    o, d = np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1))
    world = rl.World.golden_test_scene()
    with pytest.raises(ValueError):  # argument errors come first
        world.hit_rays(np.zeros((2, 3)), np.zeros((3, 3)))
    with pytest.raises(rl.RLError) as e:
        world.hit_rays(o, d)
    assert e.value.code == api.RL_E_NO_DEVICE
    with pytest.raises(rl.RLError) as e:
        world.hit_rays_device(0x1000, 0x2000, 2)
    assert e.value.code == api.RL_E_NO_DEVICE
    rw = rl.RtcWorld.test_mirror_scene(30, 20)
    for call in (lambda: rw.intersect_rays(o, d), lambda: rw.color_at_rays(o, d), lambda: rw.color_at_rays_device(0x1000, 0x2000, 2),
                 lambda: rw.intersect_rays_device(0x1000, 2, 0, 0, 0x2000)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    rays = api.pack_rays(o, d)
    hits = np.zeros(2, dtype=api.RTIOW_HIT)
    counts = np.zeros(2, dtype=np.uint32)
    rgb = np.zeros((2, 3))
    assert lib.rl_rtiow_hit_rays(None, rays.ctypes.data, 2, 1e-10, float("inf"), hits.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_hit_rays_device(None, rays.ctypes.data, 2, 1e-10, float("inf"), hits.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_intersect_rays(None, rays.ctypes.data, 2, 0, None, counts.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_intersect_rays_device(None, rays.ctypes.data, 2, 0, None, counts.ctypes.data, None, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_color_at_rays(None, rays.ctypes.data, 2, rgb.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_color_at_rays_device(None, rays.ctypes.data, 2, rgb.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_ray_query_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    assert H.rlh_ray_query_probe(0, rays.ctypes.data, 2, 1e-10, float("inf"), hits.ctypes.data) == -1
