"""CPU tier: the material-query entry points (rl_rtiow_scatter_rays, rl_rtiow_texture_values and their _device forms) are exported,
declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers, and fail LOUDLY (RL_E_NO_DEVICE,
no CPU fallback) when no GPU is present."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_scatter_rays": 9, "rl_rtiow_scatter_rays_device": 10, "rl_rtiow_texture_values": 6, "rl_rtiow_texture_values_device": 7}


def test_material_query_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert re.search(r"typedef\s+struct\s+rl_rtiow_scatter\s*\{\s*double\s+attenuation\[3\];\s*double\s+emitted\[3\];\s*rl_ray\s+scattered;\s*"
                     r"uint32_t\s+scatter;\s*uint32_t\s+_pad;\s*\}\s*rl_rtiow_scatter;", header)
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_material_query_probe")
    for m in ("scatter_rays", "scatter_rays_device", "texture_values", "texture_values_device"):
        assert callable(getattr(rl.World, m)), m


def test_scatter_record_layout_matches_header(rl):
    api = rl.api
    assert api.SCATTER.itemsize == 112
    for field, off in (("attenuation", 0), ("emitted", 24), ("scattered", 48), ("scatter", 104)):
        assert api.SCATTER.fields[field][1] == off, field
    assert api.SCATTER.fields["scattered"][0] == api.RAY


def test_scene_tables_are_readable(rl):
    """World.materials / textures / perlins: the tables RTIOW_HIT.material and texture_values index."""
    api = rl.api
    w = rl.World.golden_test_scene()
    c = w.counts()
    m, t = w.materials(), w.textures()
    assert m.dtype == api.MATERIAL and m.shape == (c["materials"],) and t.dtype == api.TEXTURE and t.shape == (c["textures"],)
    assert set(m["kind"].tolist()) == {api.MAT_LAMBERTIAN, api.MAT_DIELECTRIC, api.MAT_METAL}
    assert (m["texture"][m["kind"] == api.MAT_LAMBERTIAN] < t.shape[0]).all()
    pw = rl.World.perlin_spheres()
    assert pw.textures()["kind"].tolist() == [api.TEX_NOISE] and pw.perlins().shape == (1,)
    assert sorted(pw.perlins()[0]["perm_x"].tolist()) == list(range(256))


def test_shape_errors_are_caught_before_the_library(rl):
    api = rl.api
    world = rl.World.golden_test_scene()
    rays = api.pack_rays(np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1)))
    hits = np.zeros(2, dtype=api.RTIOW_HIT)
    cur = api.pack_cursors([0, 1])
    for bad in (lambda: world.scatter_rays(rays, hits[:1], cur, 0),                              # one hit for two rays
                lambda: world.scatter_rays(rays, hits, api.pack_cursors([0, 1, 2]), 0),          # three cursors
                lambda: world.scatter_rays(rays, hits, np.zeros((2, 2), dtype=np.uint64), 0),    # not cursor records
                lambda: world.scatter_rays(np.zeros((2, 7)), hits, cur, 0),                      # not ray records
                lambda: world.scatter_rays(rays, np.zeros((2, 11)), cur, 0),                     # not hit records
                lambda: world.scatter_rays(rays.reshape(1, 2), hits, cur, 0),
                lambda: world.texture_values([0, 1], np.zeros((2, 3)), np.zeros((2, 3))),        # uv is [n, 2]
                lambda: world.texture_values([0, 1], np.zeros((2, 2)), np.zeros((3, 3))),
                lambda: world.texture_values([[0, 1]], np.zeros((2, 2)), np.zeros((2, 3))),
                lambda: world.texture_values([0.5, 1.0], np.zeros((2, 2)), np.zeros((2, 3))),
                lambda: world.texture_values([-1, 1], np.zeros((2, 2)), np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_material_queries_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    rays = api.pack_rays(np.zeros((2, 3)), np.tile((0.0, 0.0, -1.0), (2, 1)))
    hits = np.zeros(2, dtype=api.RTIOW_HIT)
    cur = api.pack_cursors([0, 1])
    tex, uv, p = np.zeros(2, dtype=np.uint32), np.zeros((2, 2)), np.zeros((2, 3))
    for call in (lambda: world.scatter_rays(rays, hits, cur, 0),
                 lambda: world.scatter_rays_device(0x1000, 0x2000, 0x3000, 2, 0, 0x4000, 0x3000),
                 lambda: world.texture_values(tex, uv, p),
                 lambda: world.texture_values_device(0x1000, 0x2000, 0x3000, 2, 0x4000)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers
    out = np.zeros(2, dtype=api.SCATTER)
    rgb = np.zeros((2, 3))
    assert lib.rl_rtiow_scatter_rays(None, rays.ctypes.data, hits.ctypes.data, cur.ctypes.data, 2, 0, out.ctypes.data, cur.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_scatter_rays_device(None, rays.ctypes.data, hits.ctypes.data, cur.ctypes.data, 2, 0, out.ctypes.data, None, None,
                                            None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_texture_values(None, tex.ctypes.data, uv.ctypes.data, p.ctypes.data, 2, rgb.ctypes.data) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_texture_values_device(None, tex.ctypes.data, uv.ctypes.data, p.ctypes.data, 2, rgb.ctypes.data, None) == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_material_query_probe.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    assert H.rlh_material_query_probe(0, rays.ctypes.data, hits.ctypes.data, cur.ctypes.data, 2, out.ctypes.data) == -1
    assert H.rlh_material_query_probe(1, tex.ctypes.data, uv.ctypes.data, p.ctypes.data, 2, rgb.ctypes.data) == -1
