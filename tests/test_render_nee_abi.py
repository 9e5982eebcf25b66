"""CPU tier: the NEE path entry points (rl_rtiow_render_nee_rows / _device, rl_rtiow_render_pixels_nee / _device) are exported, declared
in include/rl_render.h, listed in api.RENDER_SYMBOLS and wired into the Python module (nee.py) and the C++ mirror; what is particular to
them is refused with RL_E_INVALID before a device is looked at; a media scene is refused; and without a GPU they fail LOUDLY
(RL_E_NO_DEVICE, no CPU fallback).  Outputs stay untouched in every case."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from pixel_family_abi import camera as _camera, forms, gpu_present, the_family_check_comes_first_and_the_device_before_every_later_rule as family_check_comes_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_nee_rows": 12, "rl_rtiow_render_nee_device": 13, "rl_rtiow_render_pixels_nee": 13, "rl_rtiow_render_pixels_nee_device": 14}
INF = float("inf")
NAN = float("nan")
GOOD = [0.0, 4.0, 0.0, 2.0, 0.0, 0.0, 0.0, 0.0, 2.0, 5.0, 4.0, 3.0]  # Q, u, v, E


def test_nee_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    text = open(os.path.join(ROOT, "include", "rl_render.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert len(getattr(lib, s).argtypes) == nargs, s
    # the signatures: the direct-lighting renders' with two double outputs in place of their three
    _I, _P, _U32, _U64, _D = C.c_int, C.c_void_p, C.c_uint32, C.c_uint64, C.c_double
    rows = lib.rl_rtiow_render_nee_rows
    assert rows.restype is _I and list(rows.argtypes[2:11]) == [_U64, _U32, _U32, _U32, _P, _U32, _D, _P, _P]
    pix = lib.rl_rtiow_render_pixels_nee_device
    assert list(pix.argtypes[2:13]) == [_U64, _P, _P, _U64, _U32, _P, _U32, _D, _P, _P, _P]
    assert "NEE path renders" in text and "LISTS EVERY DiffuseLight" in text
    assert "rl_rtiow_nee" not in header  # scalars and plain pointers: no new struct type in the prototypes
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_nee_probe")
    for m in ("render_nee", "render_nee_device", "render_pixels_nee", "render_pixels_nee_device", "PathNEE"):
        assert callable(getattr(rl, m)) and getattr(rl, m) is getattr(rl.nee, m), m
    # not on api.Camera and not in api
    assert not any("nee" in n.split("_") for n in dir(rl.api.Camera)) and not hasattr(rl.api, "render_nee")


def test_what_is_particular_to_the_calls_is_refused_before_a_device_is_looked_at(rl):
    """The direct-lighting renders' rules (n_lights == 0 or > 16, lights == NULL, light_samples == 0, S L K >= 2^32, a light component that
    is not finite, u x v == 0, seg_tmax NaN, <= 1e-10 or > 1), max_depth == 0 and both outputs NULL: RL_E_INVALID from every form, whether
    or not the library has a device (nothing here initialises one), outputs untouched.  Calls that get past these rules reach
    RL_E_NO_DEVICE on a machine without a GPU."""
    api = rl.api
    lib = api.render_lib()
    cam, big, flat = _camera(rl), _camera(rl, spp=1 << 16), _camera(rl, max_depth=0)
    sums, sq = np.full((24, 3), 7.0), np.full((24, 3), 8.0)
    s, q = sums.ctypes.data, sq.ctypes.data
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
    refused = [(0, one, 1, T, s, q), (17, seventeen, 1, T, s, q), (1, None, 1, T, s, q), (1, one, 0, T, s, q),
               (2, bad(0, NAN), 1, T, s, q), (2, bad(4, INF), 1, T, s, q), (2, bad(8, -INF), 1, T, s, q), (2, bad(11, NAN), 1, T, s, q),
               (1, parallel, 1, T, s, q), (1, zero_u, 1, T, s, q),
               (1, one, 1, NAN, s, q), (1, one, 1, 1e-10, s, q), (1, one, 1, 0.0, s, q), (1, one, 1, -0.5, s, q),
               (1, one, 1, math.nextafter(1.0, 2.0), s, q), (1, one, 1, INF, s, q), (1, one, 1, T, None, None)]
    for name, f in forms(lib, "nee", cam).items():
        for L, li, k, t, ps, pq in refused:
            assert f(L, None if li is None else li.ctypes.data, k, t, ps, pq) == api.RL_E_INVALID, (name, L, k, t)
            assert b"bad argument" in lib.rl_last_error(), (name, L, k, t, lib.rl_last_error())
    for name, f in forms(lib, "nee", flat).items():  # a path has at least one vertex
        assert f(1, one.ctypes.data, 1, T, s, q) == api.RL_E_INVALID, name
        assert b"bad argument" in lib.rl_last_error(), name
    sixteen = arr([GOOD] * 16)
    for name, f in forms(lib, "nee", big).items():  # S = 2^16, L = 16: K = 2^12 is S L K = 2^32, one less is legal
        assert f(16, sixteen.ctypes.data, 1 << 12, T, s, q) == api.RL_E_INVALID, name
        assert b"bad argument" in lib.rl_last_error(), name
    for name, f in forms(lib, "nee", cam).items():  # L K alone beyond 32 bits
        assert f(16, sixteen.ctypes.data, 0xFFFFFFFF, T, s, q) == api.RL_E_INVALID, name
    assert (sums == 7.0).all() and (sq == 8.0).all()
    if not gpu_present():
        assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
        legal = [(cam, 1, one, 4, T, s, q), (big, 16, sixteen, (1 << 12) - 1, T, s, q), (cam, 16, sixteen, 3, 1.0, s, q),
                 (cam, 1, one, 4, math.nextafter(1e-10, 1.0), s, q), (cam, 1, one, 4, T, s, None), (cam, 1, one, 4, T, None, q),
                 (_camera(rl, max_depth=1), 1, one, 1, T, s, q)]
        for cm, L, li, k, t, ps, pq in legal:
            for name, f in forms(lib, "nee", cm).items():
                assert f(L, li.ctypes.data, k, t, ps, pq) == api.RL_E_NO_DEVICE, (name, L, k, t)
        assert (sums == 7.0).all() and (sq == 8.0).all()


def test_the_family_check_comes_first_and_the_device_before_every_later_rule(rl):
    """pixel_family_abi's statement of the order, over this family's refused and legal arguments."""
    sums, sq = np.full((24, 3), 7.0), np.full((24, 3), 8.0)
    s, q = sums.ctypes.data, sq.ctypes.data
    one = np.array([GOOD], dtype=np.float64)
    li = one.ctypes.data
    refused = [(0, li, 1, 0.5, s, q), (1, None, 1, 0.5, s, q), (1, li, 0, 0.5, s, q), (1, li, 1, NAN, s, q), (1, li, 1, 0.5, None, None)]
    legal = [(1, li, 1, 0.5, s, q), (1, li, 3, 1.0, None, q)]
    untouched = lambda: (sums == 7.0).all() and (sq == 8.0).all()
    family_check_comes_first(rl, "nee", refused, legal, untouched)


def test_want_and_path_nee_are_checked_in_python(rl, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(rl.api, "render_lib", no_library)
    cam = _camera(rl)
    with pytest.raises(ValueError):
        rl.render_nee(cam, object(), np.array([GOOD]), 4, want=())
    with pytest.raises(ValueError):
        rl.render_nee(cam, object(), np.array([GOOD]), 4, want=("sums", "direct"))
    with pytest.raises(ValueError):
        rl.render_pixels_nee(cam, object(), [0, 1], [0], np.array([GOOD]), 4)
    with pytest.raises(ValueError):
        rl.render_nee(cam, object(), np.zeros((0, 12)), 4)
    f = lambda *rows: np.array(rows, dtype=np.float64)
    a = rl.PathNEE(f((8.0, 4.0, 0.0), (2.0, 2.0, 2.0)), f((40.0, 10.0, 0.0), (2.0, 2.0, 2.0)), 2, 3)
    m = a.moments()
    assert isinstance(m, rl.api.Moments) and m.samples == 2 and m.sums is a.sums and m.sq is a.sq
    assert m.variance_of_mean().tolist() == [[(40.0 - 64.0 / 2) / 1 / 2, (10.0 - 16.0 / 2) / 1 / 2, 0.0], [0.0, 0.0, 0.0]]
    assert a.mean().tolist() == [[4.0, 2.0, 0.0], [1.0, 1.0, 1.0]]
    both = m.merge(rl.PathNEE(a.sums, a.sq, 2, 3).moments())
    assert both.samples == 4 and both.sums.tolist() == (a.sums + a.sums).tolist()
    with pytest.raises(ValueError):
        rl.PathNEE(a.sums, None, 2, 3).moments()
    with pytest.raises(ValueError):
        rl.PathNEE(None, a.sq, 2, 3).mean()


def test_last_query_names_the_nee_kernels(rl, monkeypatch):
    api = rl.api

    class Lib:
        def __init__(self, kid):
            self.kid = kid

        def rl_debug_last_query(self, out):
            out[0], out[1] = self.kid, 3
            return 0
    for kid, name in ((11, "nee_reference"), (12, "nee_fast")):
        monkeypatch.setattr(api, "render_lib", lambda kid=kid: Lib(kid))
        assert api.last_query() == {"kernel": name, "retraced": 3}


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_nee_renders_without_a_device_fail_loudly_and_media_scenes_come_after(rl):
    """Without a device every call that passes the argument rules ends at RL_E_NO_DEVICE, a media scene included: the media refusal
    (RL_E_UNSUPPORTED) is a rule about the compiled scene and is asserted on the device (tests/test_gpu_render_nee.py)."""
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    smoke = rl.World.example_scene("cornell_smoke")
    cam = _camera(rl)
    lights = [((0, 4, 0), (2, 0, 0), (0, 0, 2), 5.0)]
    for call in (lambda: rl.render_nee(cam, world, lights, 4), lambda: rl.render_nee(cam, world, lights, 4, 0.5, stats={}),
                 lambda: rl.render_pixels_nee(cam, world, [0, 1], [0, 1], lights, 4),
                 lambda: rl.render_nee_device(cam, world, lights, 4, d_sums=0x1000),
                 lambda: rl.render_pixels_nee_device(cam, world, 0x1000, 0x2000, 2, lights, 4, d_sq=0x3000, stats={}),
                 lambda: rl.render_nee(cam, smoke, lights, 4)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C++ mirror reaches the same wall
    with pytest.raises(rl.RLError) as e:
        rl.nee.cpp_mirror_probe(6, 2, 0, lights, 4)
    assert "rl_init has not succeeded" in str(e.value)  # (the mirror creates its scene first)
