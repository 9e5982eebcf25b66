"""CPU tier: the seeded path-query entry points (rl_rtiow_camera_rays, rl_rtiow_ray_color_rays and their _device forms) are exported,
declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers, and fail LOUDLY (RL_E_NO_DEVICE,
no CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_camera_rays": 7, "rl_rtiow_camera_rays_device": 8, "rl_rtiow_ray_color_rays": 11, "rl_rtiow_ray_color_rays_device": 12}


def test_path_query_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert re.search(r"typedef\s+struct\s+rl_rng_cursor\s*\{\s*uint64_t\s+stream;\s*uint64_t\s+word_pos;\s*\}\s*rl_rng_cursor;", header)
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_path_query_probe")
    for m in ("ray_color_rays", "ray_color_rays_device"):
        assert callable(getattr(rl.World, m)), m
    for m in ("get_rays", "get_rays_device"):
        assert callable(getattr(rl.Camera, m)), m


def test_cursor_record_layout_matches_header(rl):
    api = rl.api
    assert api.RNG_CURSOR.itemsize == 16
    assert api.RNG_CURSOR.fields["stream"][1] == 0 and api.RNG_CURSOR.fields["word_pos"][1] == 8
    c = api.pack_cursors([3, 2 ** 40], word_pos=[0, 6])
    assert c.dtype == api.RNG_CURSOR and c["stream"].tolist() == [3, 2 ** 40] and c["word_pos"].tolist() == [0, 6]
    assert api.pack_cursors(np.arange(4, dtype=np.uint64), 8)["word_pos"].tolist() == [8] * 4


def test_cursor_shape_errors_are_caught_before_the_library(rl):
    api = rl.api
    for bad in (lambda: api.pack_cursors(np.zeros((4, 2), dtype=np.uint64)), lambda: api.pack_cursors(np.zeros(4)),
                lambda: api.pack_cursors([1, 2, 3], word_pos=[0, 0]), lambda: api.pack_cursors([1, 2], word_pos=0.5),
                lambda: api.pack_cursors([-1, 2]), lambda: api.pack_cursors([1, 2], word_pos=-2)):
        with pytest.raises(ValueError):
            bad()
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    o, d = np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1))
    with pytest.raises(ValueError):  # three cursors for two rays
        world.ray_color_rays(o, d, None, api.pack_cursors([0, 1, 2]), 0, 5, (0, 0, 0))
    with pytest.raises(ValueError):  # not cursor records
        world.ray_color_rays(o, d, None, np.zeros((2, 2), dtype=np.uint64), 0, 5, (0, 0, 0))
    with pytest.raises(ValueError):
        cam.get_rays([0, 1], [0], api.pack_cursors([0, 1]))
    with pytest.raises(ValueError):
        cam.get_rays([0, 1], [0, 0], api.pack_cursors([0]))


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_path_queries_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    o, d = np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1))
    cur = api.pack_cursors([0, 1])
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    for call in (lambda: world.ray_color_rays(o, d, None, cur, 0, 5, (0.5, 0.5, 0.5)),
                 lambda: world.ray_color_rays_device(0x1000, 0x2000, 2, 0, 5, (0.5, 0.5, 0.5), 0x3000),
                 lambda: cam.get_rays([0, 1], [0, 0], cur), lambda: cam.get_rays_device(0x1000, 0x2000, 0x3000, 0x4000, 0x3000, 2)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    rays = api.pack_rays(o, d)
    px, py = np.zeros(2, dtype=np.uint32), np.zeros(2, dtype=np.uint32)
    rgb = np.zeros((2, 3))
    bg = (ctypes.c_double * 3)(0.5, 0.5, 0.5)
    cnt = np.zeros(2, dtype=np.uint32)
    assert lib.rl_rtiow_camera_rays(ctypes.byref(cam.c), 2, px.ctypes.data, py.ctypes.data, cur.ctypes.data, rays.ctypes.data, cur.ctypes.data) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_camera_rays_device(ctypes.byref(cam.c), 2, px.ctypes.data, py.ctypes.data, cur.ctypes.data, rays.ctypes.data, cur.ctypes.data,
                                           None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_ray_color_rays(None, rays.ctypes.data, cur.ctypes.data, 2, 0, 5, bg, rgb.ctypes.data, cur.ctypes.data, cnt.ctypes.data,
                                       None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_ray_color_rays_device(None, rays.ctypes.data, cur.ctypes.data, 2, 0, 5, bg, rgb.ctypes.data, None, None, None,
                                              None) == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_path_query_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    assert H.rlh_path_query_probe(0, None, cur.ctypes.data, 2, rays.ctypes.data) == -1
    assert H.rlh_path_query_probe(1, rays.ctypes.data, cur.ctypes.data, 2, rgb.ctypes.data) == -1
