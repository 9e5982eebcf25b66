"""CPU tier: the direct-lighting entry points (rl_rtiow_render_direct_rows / _device, rl_rtiow_render_pixels_direct / _device) are
exported, declared in include/rl_render.h, listed in api.RENDER_SYMBOLS and wired into the Python module (direct.py) and the C++ mirror;
what is particular to them is refused with RL_E_INVALID before a device is looked at; and without a GPU they fail LOUDLY (RL_E_NO_DEVICE, no
CPU fallback).  Outputs stay untouched in both cases.  pack_lights and DirectLight's arithmetic need no library."""
import math
import os
import re

import numpy as np
import pytest
from pixel_family_abi import camera as _camera, forms, gpu_present, the_family_check_comes_first_and_the_device_before_every_later_rule as family_check_comes_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_direct_rows": 13, "rl_rtiow_render_direct_device": 14, "rl_rtiow_render_pixels_direct": 14, "rl_rtiow_render_pixels_direct_device": 15}
INF = float("inf")
NAN = float("nan")
GOOD = [0.0, 4.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0, 5.0, 4.0, 3.0]  # Q, u, v, E


def test_direct_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    text = open(os.path.join(ROOT, "include", "rl_render.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert "Direct-lighting renders" in text and re.search(r"#define\s+RL_DIRECT_MAX_LIGHTS\s+16u\b", header)
    assert "rl_rtiow_direct" not in header and "rl_light" not in header  # scalars and plain pointers: no new struct type in the prototypes
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_direct_probe")
    for m in ("render_direct", "render_direct_device", "render_pixels_direct", "render_pixels_direct_device", "DirectLight", "pack_lights"):
        assert callable(getattr(rl, m)) and getattr(rl, m) is getattr(rl.direct, m), m
    assert rl.direct.MAX_LIGHTS == 16 and rl.direct.SEG_TMAX == 1.0 - 1e-6
    # not on api.Camera and not in api
    assert not any("direct" in n.split("_") for n in dir(rl.api.Camera)) and not hasattr(rl.api, "render_direct")


def test_what_is_particular_to_the_calls_is_refused_before_a_device_is_looked_at(rl):
    """n_lights == 0 or > 16, lights == NULL, light_samples == 0, S L K >= 2^32, a light component that is not finite, u x v == 0, seg_tmax
    NaN, <= 1e-10 or > 1, all three outputs NULL: RL_E_INVALID from every form, whether or not the library has a device (nothing here
    initialises one), outputs untouched.  Calls that get past these rules reach RL_E_NO_DEVICE on a machine without a GPU and the NULL
    scene's RL_E_INVALID otherwise."""
    api = rl.api
    lib = api.render_lib()
    cam, big = _camera(rl), _camera(rl, spp=1 << 16)
    direct, unsh, hits = np.full((24, 3), 7.0), np.full((24, 3), 8.0), np.full(24, 9, dtype=np.uint32)
    d, u, h = direct.ctypes.data, unsh.ctypes.data, hits.ctypes.data
    arr = lambda rows: np.array(rows, dtype=np.float64).reshape(-1, 12)
    one = arr([GOOD])
    seventeen = arr([GOOD] * 17)

    def bad(i, v):
        a = arr([GOOD, GOOD])
        a[1, i] = v
        return a
    parallel = arr([GOOD])
    parallel[0, 6:9] = (-4.0, 0.0, 0.0)  # v = -2 u: u x v == 0
    zero_u = arr([GOOD])
    zero_u[0, 3:6] = 0.0
    T = 1.0 - 1e-6
    refused = [(0, one, 1, T, d, u, h), (17, seventeen, 1, T, d, u, h), (1, None, 1, T, d, u, h), (1, one, 0, T, d, u, h),
               (2, bad(0, NAN), 1, T, d, u, h), (2, bad(4, INF), 1, T, d, u, h), (2, bad(8, -INF), 1, T, d, u, h), (2, bad(11, NAN), 1, T, d, u, h),
               (1, parallel, 1, T, d, u, h), (1, zero_u, 1, T, d, u, h),
               (1, one, 1, NAN, d, u, h), (1, one, 1, 1e-10, d, u, h), (1, one, 1, 0.0, d, u, h), (1, one, 1, -0.5, d, u, h),
               (1, one, 1, math.nextafter(1.0, 2.0), d, u, h), (1, one, 1, INF, d, u, h), (1, one, 1, T, None, None, None)]
    for name, f in forms(lib, "direct", cam).items():
        for L, li, k, t, pd, pu, ph in refused:
            assert f(L, None if li is None else li.ctypes.data, k, t, pd, pu, ph) == api.RL_E_INVALID, (name, L, k, t)
            assert b"bad argument" in lib.rl_last_error(), (name, L, k, t, lib.rl_last_error())
    sixteen = arr([GOOD] * 16)
    for name, f in forms(lib, "direct", big).items():  # S = 2^16, L = 16: K = 2^12 is S L K = 2^32, one less is legal
        assert f(16, sixteen.ctypes.data, 1 << 12, T, d, u, h) == api.RL_E_INVALID, name
        assert b"bad argument" in lib.rl_last_error(), name
    for name, f in forms(lib, "direct", cam).items():  # L K alone beyond 32 bits
        assert f(16, sixteen.ctypes.data, 0xFFFFFFFF, T, d, u, h) == api.RL_E_INVALID, name
    assert (direct == 7.0).all() and (unsh == 8.0).all() and (hits == 9).all()
    if not gpu_present():
        assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
        legal = [(cam, 1, one, 4, T, d, u, h), (big, 16, sixteen, (1 << 12) - 1, T, d, u, h), (cam, 16, sixteen, 3, 1.0, d, u, h),
                 (cam, 1, one, 4, math.nextafter(1e-10, 1.0), d, u, h), (cam, 1, one, 4, T, d, None, None), (cam, 1, one, 4, T, None, u, None),
                 (cam, 1, one, 4, T, None, None, h)]
        for cm, L, li, k, t, pd, pu, ph in legal:
            for name, f in forms(lib, "direct", cm).items():
                assert f(L, li.ctypes.data, k, t, pd, pu, ph) == api.RL_E_NO_DEVICE, (name, L, k, t)
        assert (direct == 7.0).all() and (unsh == 8.0).all() and (hits == 9).all()


def test_the_family_check_comes_first_and_the_device_before_every_later_rule(rl):
    """pixel_family_abi's statement of the order, over this family's refused and legal arguments."""
    direct, unsh, hits = np.full((24, 3), 7.0), np.full((24, 3), 8.0), np.full(24, 9, dtype=np.uint32)
    d, u, h = direct.ctypes.data, unsh.ctypes.data, hits.ctypes.data
    one = np.array([GOOD], dtype=np.float64)
    li = one.ctypes.data
    refused = [(0, li, 1, 0.5, d, u, h), (1, None, 1, 0.5, d, u, h), (1, li, 0, 0.5, d, u, h), (1, li, 1, NAN, d, u, h), (1, li, 1, 0.5, None, None, None)]
    legal = [(1, li, 1, 0.5, d, u, h), (1, li, 3, 1.0, None, None, h)]
    untouched = lambda: (direct == 7.0).all() and (unsh == 8.0).all() and (hits == 9).all()
    family_check_comes_first(rl, "direct", refused, legal, untouched)


def test_pack_lights_shape_dtype_and_refusals(rl):
    one = rl.pack_lights([((0, 4, 0), (2, 0, 0), (0, 0, 2), (5, 4, 3))])
    assert one.shape == (1, 12) and one.dtype == np.float64 and one.flags["C_CONTIGUOUS"]
    assert one.tolist() == [GOOD]
    two = rl.pack_lights([((0, 4, 0), (2, 0, 0), (0, 0, 2), 15.0), (np.zeros(3), np.ones(3), (1.0, 0.0, 0.0), (1, 2, 3))])
    assert two.shape == (2, 12) and two[0, 9:].tolist() == [15.0, 15.0, 15.0] and two[1].tolist() == [0, 0, 0, 1, 1, 1, 1, 0, 0, 1, 2, 3]
    again = rl.pack_lights(two.astype(np.float32))
    assert again.dtype == np.float64 and np.array_equal(again, two)
    for wrong in ([], [((0, 0, 0), (1, 0, 0), (0, 1, 0))], [((0, 0), (1, 0, 0), (0, 1, 0), 1.0)], np.zeros((2, 11)), np.zeros((17, 12)),
                  [((0, 4, 0), (2, 0, 0), (0, 0, 2), 1.0)] * 17):
        with pytest.raises(ValueError):
            rl.pack_lights(wrong)


def test_want_and_the_direct_light_arithmetic_are_checked_in_python(rl, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(rl.api, "render_lib", no_library)
    cam = _camera(rl)
    with pytest.raises(ValueError):
        rl.render_direct(cam, object(), np.array([GOOD]), 4, want=())
    with pytest.raises(ValueError):
        rl.render_direct(cam, object(), np.array([GOOD]), 4, want=("direct", "albedo"))
    with pytest.raises(ValueError):
        rl.render_pixels_direct(cam, object(), [0, 1], [0], np.array([GOOD]), 4)
    with pytest.raises(ValueError):
        rl.render_direct(cam, object(), np.zeros((0, 12)), 4)
    f = lambda *rows: np.array(rows, dtype=np.float64)
    u32 = lambda *v: np.array(v, dtype=np.uint32)
    a = rl.DirectLight(f((8.0, 4.0, 0.0), (0.0, 0.0, 0.0), (3.0, 3.0, 3.0)), f((16.0, 4.0, 0.0), (0.0, 0.0, 0.0), (6.0, 3.0, 12.0)), u32(2, 0, 1), 2)
    assert a.irradiance().tolist() == [[2.0, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 1.5, 1.5]]
    assert a.irradiance(miss=-1.0)[1].tolist() == [-1.0, -1.0, -1.0]
    assert a.shadow().tolist() == [[0.5, 1.0, 1.0], [1.0, 1.0, 1.0], [0.5, 1.0, 0.25]]  # 1 where unshadowed == 0
    rad = a.radiance(f((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.0, 0.0, 2.0)))
    assert np.array_equal(rad, f((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.0, 0.0, 2.0)) * a.irradiance() / math.pi) and rad[2, 2] == 2.0 * 1.5 / math.pi
    b = rl.DirectLight(f((1.0, 0.0, 0.0), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0)), f((1.0, 0.0, 0.0), (2.0, 2.0, 4.0), (0.0, 0.0, 0.0)), u32(1, 1, 0), 2)
    m = a.merge(b)
    assert m.light_samples == 2 and m.hits.tolist() == [3, 1, 1] and m.hits.dtype == np.uint32
    assert m.direct.tolist() == [[9.0, 4.0, 0.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]] and m.unshadowed[1].tolist() == [2.0, 2.0, 4.0]
    assert m.irradiance()[0].tolist() == [1.5, 4.0 / 6.0, 0.0]
    with pytest.raises(ValueError):
        a.merge(rl.DirectLight(b.direct, b.unshadowed, b.hits, 3))
    with pytest.raises(ValueError):
        a.merge(rl.DirectLight(None, b.unshadowed, b.hits, 2))
    with pytest.raises(ValueError):
        a.merge(rl.DirectLight(b.direct[:2], b.unshadowed[:2], b.hits[:2], 2))
    with pytest.raises(OverflowError):
        rl.DirectLight(None, None, u32(0xFFFFFFFF), 2).merge(rl.DirectLight(None, None, u32(1), 2))
    with pytest.raises(ValueError):
        rl.DirectLight(None, a.unshadowed, a.hits, 2).irradiance()
    with pytest.raises(ValueError):
        rl.DirectLight(a.direct, None, a.hits, 2).shadow()


def test_last_query_names_the_direct_kernels(rl, monkeypatch):
    api = rl.api

    class Lib:
        def __init__(self, kid):
            self.kid = kid

        def rl_debug_last_query(self, out):
            out[0], out[1] = self.kid, 3
            return 0
    for kid, name in ((9, "direct_reference"), (10, "direct_fast")):
        monkeypatch.setattr(api, "render_lib", lambda kid=kid: Lib(kid))
        assert api.last_query() == {"kernel": name, "retraced": 3}


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_direct_renders_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    cam = _camera(rl)
    lights = [((0, 4, 0), (2, 0, 0), (0, 0, 2), 5.0)]
    for call in (lambda: rl.render_direct(cam, world, lights, 4), lambda: rl.render_direct(cam, world, lights, 4, 0.5, stats={}),
                 lambda: rl.render_pixels_direct(cam, world, [0, 1], [0, 1], lights, 4),
                 lambda: rl.render_direct_device(cam, world, lights, 4, d_direct=0x1000),
                 lambda: rl.render_pixels_direct_device(cam, world, 0x1000, 0x2000, 2, lights, 4, d_hits=0x3000, stats={})):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    with pytest.raises(rl.RLError) as e:
        rl.direct.cpp_mirror_probe(6, 2, 0, lights, 4)
    assert "rl_init has not succeeded" in str(e.value)  # (the mirror creates its scene first)
