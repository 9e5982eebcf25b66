"""CPU tier: the seeded hit-query entry points (rl_rtiow_hit_rays_seeded and its _device form) are exported, declared in
include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers, and fail LOUDLY (RL_E_NO_DEVICE, no CPU
fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_hit_rays_seeded": 10, "rl_rtiow_hit_rays_seeded_device": 11}
PROBE_ARGS = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]


def test_seeded_hit_query_entry_points_are_exported_declared_and_listed(rl):
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
    assert hasattr(rl.api.host_lib(), "rlh_seeded_hit_query_probe")
    for m in ("hit_rays_seeded", "hit_rays_seeded_device"):
        assert callable(getattr(rl.World, m)), m


def test_shape_errors_are_caught_before_the_library(rl):
    api = rl.api
    world = rl.World.example_scene("cornell_smoke")
    rays = api.pack_rays(np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1)))
    cur = api.pack_cursors([0, 1])
    for bad in (lambda: world.hit_rays_seeded(rays, cur[:1], 0),                                # one cursor for two rays
                lambda: world.hit_rays_seeded(rays, api.pack_cursors([0, 1, 2]), 0),            # three cursors
                lambda: world.hit_rays_seeded(rays, np.zeros((2, 2), dtype=np.uint64), 0),      # not cursor records
                lambda: world.hit_rays_seeded(np.zeros((2, 7)), cur, 0),                        # not ray records
                lambda: world.hit_rays_seeded(rays.reshape(1, 2), cur, 0)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_seeded_hit_queries_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.example_scene("cornell_smoke")
    rays = api.pack_rays(np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1)))
    cur = api.pack_cursors([0, 1])
    for call in (lambda: world.hit_rays_seeded(rays, cur, 0),
                 lambda: world.hit_rays_seeded_device(0x1000, 0x2000, 2, 0, 0x3000, 0x2000)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    out = np.zeros(2, dtype=api.RTIOW_HIT)
    inf = float("inf")
    assert lib.rl_rtiow_hit_rays_seeded(None, rays.ctypes.data, cur.ctypes.data, 2, 0, 1e-10, inf, out.ctypes.data, cur.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_hit_rays_seeded_device(None, rays.ctypes.data, cur.ctypes.data, 2, 0, 1e-10, inf, out.ctypes.data, None, None,
                                               None) == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_seeded_hit_query_probe.argtypes = PROBE_ARGS
    assert H.rlh_seeded_hit_query_probe(rays.ctypes.data, cur.ctypes.data, 2, 1e-10, inf, out.ctypes.data) == -1
