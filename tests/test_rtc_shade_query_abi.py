"""CPU tier: the RTC shading-query entry points (rl_rtc_prepare_rays, rl_rtc_shade_hits, rl_rtc_shadow_attenuation, rl_rtc_lighting and
their _device forms) are exported, declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers,
and fail LOUDLY (RL_E_NO_DEVICE, no CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtc_prepare_rays": 5, "rl_rtc_prepare_rays_device": 6, "rl_rtc_shade_hits": 6, "rl_rtc_shade_hits_device": 7,
       "rl_rtc_shadow_attenuation": 6, "rl_rtc_shadow_attenuation_device": 7, "rl_rtc_lighting": 7, "rl_rtc_lighting_device": 8}


def test_rtc_shade_query_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert re.search(r"typedef\s+struct\s+rl_rtc_comps\s*\{\s*double\s+t,\s*point\[3\],\s*eye_v\[3\],\s*normal_v\[3\],\s*over_point\[3\],\s*"
                     r"under_point\[3\],\s*reflect_v\[3\];\s*double\s+n1,\s*n2;\s*double\s+object_color\[3\];\s*uint32_t\s+hit;\s*"
                     r"uint32_t\s+inside;\s*uint32_t\s+object;\s*uint32_t\s+material;\s*\}\s*rl_rtc_comps;", header)
    assert re.search(r"typedef\s+struct\s+rl_rtc_shade\s*\{\s*double\s+surface\[3\];\s*double\s+schlick;\s*rl_ray\s+reflected;\s*"
                     r"rl_ray\s+refracted;\s*uint32_t\s+reflect;\s*uint32_t\s+refract;\s*\}\s*rl_rtc_shade;", header)
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_rtc_shade_query_probe")
    for m in ("prepare_rays", "shade_hits", "shadow_attenuation", "lighting"):
        assert callable(getattr(rl.RtcWorld, m)) and callable(getattr(rl.RtcWorld, m + "_device")), m


def test_comps_and_shade_record_layouts_match_the_header(rl):
    api = rl.api
    assert api.RTC_COMPS.itemsize == 208 and api.RTC_SHADE.itemsize == 152
    for field, off in (("t", 0), ("point", 8), ("eye_v", 32), ("normal_v", 56), ("over_point", 80), ("under_point", 104), ("reflect_v", 128),
                       ("n1", 152), ("n2", 160), ("object_color", 168), ("hit", 192), ("inside", 196), ("object", 200), ("material", 204)):
        assert api.RTC_COMPS.fields[field][1] == off, field
    for field, off in (("surface", 0), ("schlick", 24), ("reflected", 32), ("refracted", 88), ("reflect", 144), ("refract", 148)):
        assert api.RTC_SHADE.fields[field][1] == off, field
    assert api.RTC_SHADE.fields["reflected"][0] == api.RAY and api.RTC_SHADE.fields["refracted"][0] == api.RAY


def test_rtc_scene_tables_are_readable(rl):
    """RtcWorld.materials / lights: the tables RTC_COMPS.material indexes and shade_hits sums over."""
    api = rl.api
    w = rl.RtcWorld.test_mirror_scene(90, 60)
    m, lt = w.materials(), w.lights()
    assert m.dtype == api.RTC_MATERIAL and m.shape[0] > 1 and lt.dtype == api.RTC_LIGHT and lt.shape == (1,)
    assert tuple(lt["position"][0]) == (-10.0, 10.0, -10.0) and tuple(lt["intensity"][0]) == (1.0, 1.0, 1.0)
    assert (m["reflectivity"] > 0).any() and (m["refractive_index"] > 0).all()


def test_shape_errors_are_caught_before_the_library(rl):
    api = rl.api
    world = rl.RtcWorld.test_mirror_scene(90, 60)
    comps = np.zeros(2, dtype=api.RTC_COMPS)
    v3 = np.zeros((2, 3))
    for bad in (lambda: world.prepare_rays(np.zeros((2, 3)), np.zeros((3, 3))),          # two origins, three directions
                lambda: world.prepare_rays(np.zeros((2, 4)), np.zeros((2, 4))),
                lambda: world.shade_hits(np.zeros((2, 26))),                               # not comps records
                lambda: world.shade_hits(comps.reshape(1, 2)),
                lambda: world.shade_hits(np.zeros(2, dtype=api.RTC_SHADE)),
                lambda: world.shadow_attenuation(np.zeros((2, 2)), v3),                    # points are [n, 3]
                lambda: world.shadow_attenuation(v3, np.zeros((3, 3))),                    # three lights for two points
                lambda: world.shadow_attenuation(np.zeros(3), np.zeros(3)),
                lambda: world.lighting(np.zeros((2, 26)), v3, v3, np.ones(2)),
                lambda: world.lighting(comps, np.zeros((3, 3)), v3, np.ones(2)),
                lambda: world.lighting(comps, v3, np.zeros((2, 2)), np.ones(2)),
                lambda: world.lighting(comps, v3, v3, np.ones(3)),                         # three attenuations for two records
                lambda: world.lighting(comps, v3, v3, np.ones((2, 1)))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_rtc_shade_queries_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.RtcWorld.test_mirror_scene(90, 60)
    o, d = np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1))
    rays = api.pack_rays(o, d)
    comps = np.zeros(2, dtype=api.RTC_COMPS)
    v3, att = np.zeros((2, 3)), np.ones(2)
    for call in (lambda: world.prepare_rays(o, d),
                 lambda: world.prepare_rays_device(0x1000, 2, 0x2000),
                 lambda: world.shade_hits(comps),
                 lambda: world.shade_hits_device(0x1000, 2, 0x2000, 0x3000),
                 lambda: world.shadow_attenuation(v3, v3),
                 lambda: world.shadow_attenuation_device(0x1000, 0x2000, 2, 0x3000),
                 lambda: world.lighting(comps, v3, v3, att),
                 lambda: world.lighting_device(0x1000, 0x2000, 0x3000, 0x4000, 2, 0x5000)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    shade = np.zeros(2, dtype=api.RTC_SHADE)
    out1, rgb = np.zeros(2), np.zeros((2, 3))
    p = lambda a: a.ctypes.data  # noqa: E731
    assert lib.rl_rtc_prepare_rays(None, p(rays), 2, p(comps), None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_prepare_rays_device(None, p(rays), 2, p(comps), None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_shade_hits(None, p(comps), 2, p(shade), None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_shade_hits_device(None, p(comps), 2, p(shade), None, None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_shadow_attenuation(None, p(v3), p(v3), 2, p(out1), None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_shadow_attenuation_device(None, p(v3), p(v3), 2, p(out1), None, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_lighting(None, p(comps), p(v3), p(v3), p(att), 2, p(rgb)) == api.RL_E_NO_DEVICE
    assert lib.rl_rtc_lighting_device(None, p(comps), p(v3), p(v3), p(att), 2, p(rgb), None) == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_rtc_shade_query_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64,
                                            ctypes.c_void_p]
    assert H.rlh_rtc_shade_query_probe(0, p(rays), None, None, None, 2, p(comps)) == -1
    assert H.rlh_rtc_shade_query_probe(1, p(comps), None, None, None, 2, p(shade)) == -1
    assert H.rlh_rtc_shade_query_probe(2, p(v3), p(v3), None, None, 2, p(out1)) == -1
    assert H.rlh_rtc_shade_query_probe(3, p(comps), p(v3), p(v3), p(att), 2, p(rgb)) == -1
