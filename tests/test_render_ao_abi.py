"""CPU tier: the ambient-occlusion entry points (rl_rtiow_render_ao_rows / _device, rl_rtiow_render_pixels_ao / _device) are exported,
declared in include/rl_render.h, listed in api.RENDER_SYMBOLS and wired into the Python module (ao.py) and the C++ mirror; what is
particular to them is refused with RL_E_INVALID before a device is looked at; and without a GPU they fail LOUDLY (RL_E_NO_DEVICE, no CPU
fallback).  Outputs stay untouched in both cases."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from pixel_family_abi import camera as _camera, forms, gpu_present, the_family_check_comes_first_and_the_device_before_every_later_rule as family_check_comes_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_ao_rows": 10, "rl_rtiow_render_ao_device": 11, "rl_rtiow_render_pixels_ao": 11, "rl_rtiow_render_pixels_ao_device": 12}
INF = float("inf")
NAN = float("nan")


def test_ao_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rl_render.h")).read(), flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert "rl_rtiow_ao" not in header  # scalars and plain pointers: no new struct type in the prototypes
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_ao_probe")
    for m in ("render_ao", "render_ao_device", "render_pixels_ao", "render_pixels_ao_device", "AmbientOcclusion"):
        assert callable(getattr(rl, m)) and getattr(rl, m) is getattr(rl.ao, m), m
    # not on api.Camera and not in api
    assert not any("ao" in n.split("_") for n in dir(rl.api.Camera)) and not hasattr(rl.api, "render_ao")


def test_what_is_particular_to_the_calls_is_refused_before_a_device_is_looked_at(rl):
    """ao_rays == 0, S * ao_rays >= 2^32, a radius that is NaN or <= 0, both outputs NULL: RL_E_INVALID from every form, whether or not the
    library has a device (nothing here initialises one), outputs untouched.  +inf is a legal radius, and one output is enough: those calls
    get past these rules, to RL_E_NO_DEVICE on a machine without a GPU and to the NULL scene's RL_E_INVALID otherwise."""
    api = rl.api
    lib = api.render_lib()
    cam, big = _camera(rl), _camera(rl, spp=1 << 16)
    op, hits = np.full(24, 7, dtype=np.uint32), np.full(24, 9, dtype=np.uint32)
    o, h = op.ctypes.data, hits.ctypes.data
    for name, f in forms(lib, "ao", cam).items():
        for k, r, po, ph in ((0, 1.0, o, h), (4, NAN, o, h), (4, 0.0, o, h), (4, -0.0, o, h), (4, -1.0, o, h), (4, -INF, o, h), (4, 1.0, None, None)):
            assert f(k, r, po, ph) == api.RL_E_INVALID, (name, k, r)
            assert b"bad argument" in lib.rl_last_error(), (name, k, r, lib.rl_last_error())
    for name, f in forms(lib, "ao", big).items():  # S = 2^16: K = 2^16 is S K = 2^32, one less is legal
        assert f(1 << 16, 1.0, o, h) == api.RL_E_INVALID, name
        assert b"bad argument" in lib.rl_last_error(), name
    assert (op == 7).all() and (hits == 9).all()
    if not gpu_present():
        assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
        for cm, k in ((cam, 4), (big, (1 << 16) - 1), (cam, 0xFFFFFFFF >> 1)):
            for name, f in forms(lib, "ao", cm).items():
                for r, po, ph in ((INF, o, h), (1e-300, o, h), (2.0, o, None), (2.0, None, h)):
                    assert f(k, r, po, ph) == api.RL_E_NO_DEVICE, (name, k, r)
        assert (op == 7).all() and (hits == 9).all()


def test_the_family_check_comes_first_and_the_device_before_every_later_rule(rl):
    """pixel_family_abi's statement of the order, over this family's refused and legal arguments."""
    op, hits = np.full(24, 7, dtype=np.uint32), np.full(24, 9, dtype=np.uint32)
    o, h = op.ctypes.data, hits.ctypes.data
    refused = [(0, 1.0, o, h), (4, NAN, o, h), (4, 1.0, None, None)]
    legal = [(4, 1.0, o, h), (1, INF, None, h)]
    untouched = lambda: (op == 7).all() and (hits == 9).all()
    family_check_comes_first(rl, "ao", refused, legal, untouched)


def test_want_and_merge_are_checked_in_python(rl, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(rl.api, "render_lib", no_library)
    cam = _camera(rl)
    with pytest.raises(ValueError):
        rl.render_ao(cam, object(), 4, 1.0, want=())
    with pytest.raises(ValueError):
        rl.render_ao(cam, object(), 4, 1.0, want=("open", "bent_normal"))
    with pytest.raises(ValueError):
        rl.render_pixels_ao(cam, object(), [0, 1], [0], 4, 1.0)
    u = lambda *v: np.array(v, dtype=np.uint32)
    a, b = rl.AmbientOcclusion(u(3, 0, 8), u(1, 0, 2), 4), rl.AmbientOcclusion(u(1, 0, 0), u(1, 0, 1), 4)
    m = a.merge(b)
    assert m.ao_rays == 4 and list(m.open) == [4, 0, 8] and list(m.hits) == [2, 0, 3] and m.open.dtype == np.uint32
    assert list(m.visibility()) == [0.5, 1.0, 8 / 12] and list(m.visibility(miss=0.25))[1] == 0.25
    with pytest.raises(ValueError):
        a.merge(rl.AmbientOcclusion(u(1, 0, 0), u(1, 0, 1), 5))
    with pytest.raises(ValueError):
        a.merge(rl.AmbientOcclusion(None, u(1, 0, 1), 4))
    with pytest.raises(OverflowError):
        rl.AmbientOcclusion(u(0xFFFFFFFF), u(1), 4).merge(rl.AmbientOcclusion(u(1), u(1), 4))
    with pytest.raises(ValueError):
        rl.AmbientOcclusion(None, u(1), 4).visibility()


def test_last_query_names_the_ao_kernels(rl, monkeypatch):
    api = rl.api

    class Lib:
        def __init__(self, kid):
            self.kid = kid

        def rl_debug_last_query(self, out):
            out[0], out[1] = self.kid, 3
            return 0
    for kid, name in ((7, "ao_reference"), (8, "ao_fast")):
        monkeypatch.setattr(api, "render_lib", lambda kid=kid: Lib(kid))
        assert api.last_query() == {"kernel": name, "retraced": 3}


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_ao_renders_without_a_device_fail_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    cam = _camera(rl)
    for call in (lambda: rl.render_ao(cam, world, 4, INF), lambda: rl.render_ao(cam, world, 4, 0.5, stats={}),
                 lambda: rl.render_pixels_ao(cam, world, [0, 1], [0, 1], 4, 1.0), lambda: rl.render_ao_device(cam, world, 4, 1.0, d_open=0x1000),
                 lambda: rl.render_pixels_ao_device(cam, world, 0x1000, 0x2000, 2, 4, 1.0, d_hits=0x3000, stats={})):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_ao_probe.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p, C.c_void_p]
    H.rlh_ao_probe.restype = C.c_int
    op, hits = np.full(24, 7, dtype=np.uint32), np.full(24, 9, dtype=np.uint32)
    assert H.rlh_ao_probe(6, 2, 0, 4, INF, op.ctypes.data, hits.ctypes.data) == -1
    assert b"rl_init has not succeeded" in H.rlh_last_error()  # (the mirror creates its scene first)
    assert (op == 7).all() and (hits == 9).all()
