"""CPU tier: the occlusion-query entry points (rl_rtiow_occluded_rays and its _device form) are exported, declared in include/rl_render.h,
listed in api.RENDER_SYMBOLS, wired into the Python module (occlusion.py) and the C++ mirror, hand their arguments on as given, and fail
LOUDLY (RL_E_NO_DEVICE, no CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest

import binding_model as bm
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_occluded_rays": 7, "rl_rtiow_occluded_rays_device": 8}
INF = float("inf")


def test_occlusion_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_occlusion_probe")
    for m in ("occluded_rays", "occluded_rays_device"):
        assert callable(getattr(rl, m)) and getattr(rl, m) is getattr(rl.occlusion, m), m


def test_ray_shape_errors_are_caught_before_the_library(rl, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(rl.api, "render_lib", no_library)
    world = object()  # never looked at: the rays are packed first
    with pytest.raises(ValueError):
        rl.occluded_rays(world, np.zeros((4, 3)), np.zeros((5, 3)))
    with pytest.raises(ValueError):
        rl.occluded_rays(world, np.zeros((4, 2)), np.zeros((4, 2)))
    with pytest.raises(ValueError):
        rl.occluded_rays(world, np.zeros((4, 3)), np.zeros((4, 3)), times=np.zeros(3))


def test_the_wrappers_hand_their_arguments_on_as_given(rl, monkeypatch):
    """binding_model's recorder stands in for render_lib(): opt_stats is NULL exactly when `stats` is None, the scalars arrive as given."""
    api = rl.api
    rec = bm.Recorder()
    monkeypatch.setattr(api, "render_lib", lambda: rec)
    monkeypatch.setattr(api, "_inited", False)
    world = rl.World.golden_test_scene()
    try:
        o, d = np.zeros((3, 3)), np.tile((0.0, 0.0, -1.0), (3, 1))

        def last(name):
            calls = [c for c in rec.calls if c[0] == name]
            assert len(calls) == 1, rec.calls
            rec.calls = []
            return calls[0][1]

        out = rl.occluded_rays(world, o, d)
        assert out.dtype == np.bool_ and out.shape == (3,) and not out.any()
        assert last("rl_rtiow_occluded_rays") == ["ptr", "ptr", 3, 1e-10, INF, "ptr", "null"]
        st = {}
        rl.occluded_rays(world, o, d, times=[0.0, 0.5, 1.0], tmin=0.25, tmax=7.5, stats=st)
        a = last("rl_rtiow_occluded_rays")
        assert a[:6] == ["ptr", "ptr", 3, 0.25, 7.5, "ptr"] and isinstance(a[6], dict) and sorted(a[6]) == sorted(k for k, _ in api.Stats._fields_)
        assert st["rc"] == api.RL_OK and "rays" in st and "flagged" in st
        rl.occluded_rays_device(world, 0x1000, 0x2000, 5)
        assert last("rl_rtiow_occluded_rays_device") == ["ptr", "ptr", 5, 1e-10, INF, "ptr", "null", "null"]
        st = {}
        rl.occluded_rays_device(world, 0x1000, 0x2000, 5, tmin=0.0, tmax=1.0, stream=0x3000, stats=st)
        a = last("rl_rtiow_occluded_rays_device")
        assert a[:7] == ["ptr", "ptr", 5, 0.0, 1.0, "ptr", "ptr"] and isinstance(a[7], dict)
        assert st["rc"] == api.RL_OK
        # a reached panic site: raised unless allowed, and then reported in the dict
        rec.rc = api.RL_E_DEGENERATE
        with pytest.raises(rl.RLError) as e:
            rl.occluded_rays(world, o, d)
        assert e.value.code == api.RL_E_DEGENERATE
        st = {}
        rl.occluded_rays(world, o, d, stats=st, allow_degenerate=True)
        assert st["rc"] == api.RL_E_DEGENERATE
    finally:
        world._device = None  # the recorder's fake handle: never destroyed through the real library


def test_last_query_names_the_occlusion_kernels(rl, monkeypatch):
    api = rl.api

    class Lib:
        def __init__(self, kid):
            self.kid = kid

        def rl_debug_last_query(self, out):
            out[0], out[1] = self.kid, 3
            return 0
    for kid, name in ((5, "occlusion_reference"), (6, "occlusion_fast")):
        monkeypatch.setattr(api, "render_lib", lambda kid=kid: Lib(kid))
        assert api.last_query() == {"kernel": name, "retraced": 3}


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_occlusion_queries_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    o, d = np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1))
    world = rl.World.golden_test_scene()
    with pytest.raises(ValueError):  # argument errors come first
        rl.occluded_rays(world, np.zeros((2, 3)), np.zeros((3, 3)))
    for call in (lambda: rl.occluded_rays(world, o, d), lambda: rl.occluded_rays(world, o, d, stats={}),
                 lambda: rl.occluded_rays_device(world, 0x1000, 0x2000, 2), lambda: rl.occluded_rays_device(world, 0x1000, 0x2000, 2, stats={})):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    rays = api.pack_rays(o, d)
    out = np.full(2, 7, dtype=np.uint8)
    st = api.Stats()
    assert lib.rl_rtiow_occluded_rays(None, rays.ctypes.data, 2, 1e-10, INF, out.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_occluded_rays(None, rays.ctypes.data, 2, 1e-10, INF, out.ctypes.data, ctypes.byref(st)) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_occluded_rays_device(None, rays.ctypes.data, 2, 1e-10, INF, out.ctypes.data, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_occluded_rays(None, rays.ctypes.data, 0, 1e-10, INF, out.ctypes.data, None) == api.RL_E_NO_DEVICE  # n = 0 is no way round it
    assert list(out) == [7, 7]  # nothing was written
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_occlusion_probe.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double, ctypes.c_double, ctypes.c_void_p]
    assert H.rlh_occlusion_probe(rays.ctypes.data, 2, 1e-10, INF, out.ctypes.data) == -1
    assert list(out) == [7, 7]
