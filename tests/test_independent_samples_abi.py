"""CPU tier: the sample-parallel entry points (rl_rtiow_render_independent_rows / _device) are exported, declared, wired into the
Python and C++ layers, and fail LOUDLY (RL_E_NO_DEVICE, no CPU fallback) when no GPU is present."""
import ctypes

import numpy as np
import pytest
from pixel_family_abi import gpu_present

NEW = ("rl_rtiow_render_independent_rows", "rl_rtiow_render_independent_device")


def test_independent_entry_points_are_exported_and_listed(rl):
    lib = rl.api.render_lib()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
    assert len(lib.rl_rtiow_render_independent_rows.argtypes) == 8
    assert len(lib.rl_rtiow_render_independent_device.argtypes) == 9
    assert lib.rl_abi_version() == 6
    for s in ("rl_debug_set_indep_cap", "rl_debug_set_indep_k"):  # test / tool switches, not part of the ABI
        assert hasattr(lib, s), s
    assert hasattr(rl.api.host_lib(), "rlh_rtiow_golden_independent")
    for m in ("render_independent", "render_independent_rows", "render_independent_device"):
        assert callable(getattr(rl.Camera, m)), m


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_independent_renders_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    p = world.params
    p.image_width, p.samples_per_pixel = 16, 2
    cam = rl.Camera(p)
    with pytest.raises(rl.RLError) as e:
        cam.render_independent(world)
    assert e.value.code == api.RL_E_NO_DEVICE
    with pytest.raises(rl.RLError) as e:
        cam.render_independent_device(world, 0x1000)
    assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with a valid host buffer
    out = np.zeros((cam.c.image_height, cam.c.image_width, 3))
    rc = lib.rl_rtiow_render_independent_rows(None, ctypes.byref(cam.c), 0, 0, 1, 0, out.ctypes.data, None)
    assert rc == api.RL_E_NO_DEVICE
    # accumulate without the sums to continue from is the caller's error, caught before the library is reached
    with pytest.raises(ValueError):
        cam.render_independent_rows(world, 0, 1, accumulate=True)
