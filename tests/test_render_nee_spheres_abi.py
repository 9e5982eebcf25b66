"""CPU tier: the entry points of the NEE path renders with sphere lights (rl_rtiow_render_nee_mis_spheres_rows / _device,
rl_rtiow_render_pixels_nee_mis_spheres / _device) are exported, declared in include/rl_render.h, listed in api.RENDER_SYMBOLS and wired
into the Python module (nee.py) and the C++ mirror; every refusal of the family ends in RL_E_INVALID before a device is looked at;
without a GPU they fail LOUDLY (RL_E_NO_DEVICE, no CPU fallback).  Outputs stay untouched in every case."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
from test_render_nee_mis_abi import GOOD, _camera
from pixel_family_abi import forms, gpu_present, the_family_check_comes_first_and_the_device_before_every_later_rule as family_check_comes_first

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_nee_mis_spheres_rows": 15, "rl_rtiow_render_nee_mis_spheres_device": 16, "rl_rtiow_render_pixels_nee_mis_spheres": 16,
       "rl_rtiow_render_pixels_nee_mis_spheres_device": 17}
INF = float("inf")
NAN = float("nan")
BALL = [0.0, 7.0, 0.0, 2.0, 4.0, 4.0, 4.0]  # C, r, E
T = 1.0 - 1e-6


def test_sphere_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    text = open(os.path.join(ROOT, "include", "rl_render.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert len(getattr(lib, s).argtypes) == nargs, s
        mis = getattr(lib, s.replace("_spheres", ""))
        # the MIS signature with (uint32_t n_sphere_lights, const double *sphere_lights) behind `lights`
        at, mt = list(getattr(lib, s).argtypes), list(mis.argtypes)
        i = at.index(C.c_double) - 3  # n_sphere_lights, sphere_lights, light_samples, seg_tmax
        assert at[i] is C.c_uint32 and at[i + 1] is C.c_void_p and at[:i] + at[i + 2:] == mt, s
        assert mt[i - 2] is C.c_uint32 and mt[i - 1] is C.c_void_p  # behind n_lights, lights
    assert "NEE path renders with sphere lights" in text
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    assert hasattr(rl.api.host_lib(), "rlh_nee_spheres_probe") and "rlh_nee_spheres_probe" in rl.api.HOST_SIGNATURES
    assert callable(rl.pack_sphere_lights) and rl.pack_sphere_lights is rl.nee.pack_sphere_lights
    import inspect
    for m in ("render_nee_mis", "render_nee_mis_device", "render_pixels_nee_mis", "render_pixels_nee_mis_device"):
        assert inspect.signature(getattr(rl, m)).parameters["sphere_lights"].default is None, m
    # "sphere lights" has left the MIS renders' Not offered line and stays on the direct-lighting and the plain NEE renders'
    lines = [l for l in text.splitlines() if "Not offered: sphere and textured lights" in l]
    assert len(lines) == 2


def test_every_refusal_comes_before_a_device_is_looked_at(rl):
    """A total of 0 or above 16, a null array with a nonzero count, a component that is not finite, !(r > 0), A not finite,
    S (L + Ls) K >= 2^32 and the MIS renders' rules (light_samples, seg_tmax, max_depth == 0, both outputs NULL, a third heuristic, the
    quads' own rules): RL_E_INVALID "bad argument" from every form, outputs untouched.  Calls past these rules reach RL_E_NO_DEVICE on a
    machine without a GPU: n_lights == 0 with a sphere, a sphere with 15 quads, no sphere at all."""
    api = rl.api
    lib = api.render_lib()
    cam, big, flat = _camera(rl), _camera(rl, spp=1 << 16), _camera(rl, max_depth=0)
    sums, sq = np.full((24, 3), 7.0), np.full((24, 3), 8.0)
    s, q = sums.ctypes.data, sq.ctypes.data
    quads = lambda n: np.array([GOOD] * n, dtype=np.float64).reshape(-1, 12)
    balls = lambda n: np.array([BALL] * n, dtype=np.float64).reshape(-1, 7)
    p = lambda a: None if a is None or a.shape[0] == 0 else a.ctypes.data

    def bad(i, v):
        a = balls(2)
        a[1, i] = v
        return a
    bad_quad = quads(2)
    bad_quad[1, 4] = NAN
    parallel = quads(1)
    parallel[0, 6:9] = (-4.0, 0.0, 0.0)
    huge = balls(1)
    huge[0, 3] = 1e160  # r * r overflows: A is not finite
    refused = [(0, None, 0, None, 1, T, 0, s, q), (0, quads(1), 0, balls(1), 1, T, 0, s, q),          # a total of 0 (arrays given or not)
               (16, quads(16), 1, balls(1), 1, T, 0, s, q), (0, None, 17, balls(17), 1, T, 0, s, q), (9, quads(9), 8, balls(8), 1, T, 0, s, q),
               (0xFFFFFFFF, quads(1), 1, balls(1), 1, T, 0, s, q), (1, quads(1), 0xFFFFFFFF, balls(1), 1, T, 0, s, q),
               (0xFFFFFFFF, quads(1), 0xFFFFFFFF, balls(1), 1, T, 0, s, q),
               (1, None, 1, balls(1), 1, T, 0, s, q), (1, quads(1), 1, None, 1, T, 0, s, q), (0, None, 1, None, 1, T, 0, s, q),   # null with a count
               (0, None, 2, bad(0, NAN), 1, T, 0, s, q), (0, None, 2, bad(2, INF), 1, T, 0, s, q), (0, None, 2, bad(3, NAN), 1, T, 0, s, q),
               (0, None, 2, bad(3, INF), 1, T, 0, s, q), (0, None, 2, bad(5, -INF), 1, T, 0, s, q), (0, None, 2, bad(6, NAN), 1, T, 0, s, q),
               (0, None, 2, bad(3, 0.0), 1, T, 0, s, q), (0, None, 2, bad(3, -0.0), 1, T, 0, s, q), (0, None, 2, bad(3, -2.0), 1, T, 0, s, q),
               (0, None, 1, huge, 1, T, 0, s, q),
               (2, bad_quad, 1, balls(1), 1, T, 0, s, q), (1, parallel, 1, balls(1), 1, T, 0, s, q),                 # the quads' own rules
               (0, None, 1, balls(1), 0, T, 0, s, q), (0, None, 1, balls(1), 1, NAN, 0, s, q), (0, None, 1, balls(1), 1, 1e-10, 0, s, q),
               (0, None, 1, balls(1), 1, math.nextafter(1.0, 2.0), 0, s, q), (0, None, 1, balls(1), 1, T, 0, None, None),
               (0, None, 1, balls(1), 1, T, 2, s, q), (1, quads(1), 1, balls(1), 1, T, 0xFFFFFFFF, s, q)]
    for name, f in forms(lib, "nee_mis_spheres", cam).items():
        for L, li, Ls, sp, k, t, h, ps, pq in refused:
            assert f(L, p(li), Ls, p(sp), k, t, h, ps, pq) == api.RL_E_INVALID, (name, L, Ls, k, t, h)
            assert b"bad argument" in lib.rl_last_error(), (name, L, Ls, k, t, h, lib.rl_last_error())
    for name, f in forms(lib, "nee_mis_spheres", flat).items():  # a path has at least one vertex
        assert f(0, None, 1, p(balls(1)), 1, T, 0, s, q) == api.RL_E_INVALID, name
    keep = (quads(8), balls(8))
    for name, f in forms(lib, "nee_mis_spheres", big).items():  # S = 2^16, L + Ls = 16: K = 2^12 is S (L + Ls) K = 2^32
        assert f(8, p(keep[0]), 8, p(keep[1]), 1 << 12, T, 1, s, q) == api.RL_E_INVALID, name
        assert f(0, None, 8, p(keep[1]), 1 << 13, T, 1, s, q) == api.RL_E_INVALID, name
    for name, f in forms(lib, "nee_mis_spheres", cam).items():  # (L + Ls) K alone beyond 32 bits
        assert f(8, p(keep[0]), 8, p(keep[1]), 0xFFFFFFFF, T, 0, s, q) == api.RL_E_INVALID, name
    assert (sums == 7.0).all() and (sq == 8.0).all()
    if not gpu_present():
        assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
        tiny = balls(1)
        tiny[0, 3] = 5e-324  # r > 0, A = 0: finite
        legal = [(cam, 0, None, 1, balls(1), 4, T, 0, s, q), (cam, 15, quads(15), 1, balls(1), 1, 1.0, 1, s, q), (cam, 0, None, 16, balls(16), 2, T, 0, None, q),
                 (cam, 1, quads(1), 0, None, 4, T, 1, s, None), (cam, 1, quads(1), 0, balls(1), 4, T, 0, s, q), (cam, 0, quads(1), 1, balls(1), 4, T, 0, s, q),
                 (big, 8, quads(8), 8, balls(8), (1 << 12) - 1, T, 0, s, q), (cam, 0, None, 1, tiny, 1, T, 0, s, q),
                 (_camera(rl, max_depth=1), 0, None, 1, balls(1), 1, T, 0, s, q)]
        for cm, L, li, Ls, sp, k, t, h, ps, pq in legal:
            for name, f in forms(lib, "nee_mis_spheres", cm).items():
                assert f(L, p(li), Ls, p(sp), k, t, h, ps, pq) == api.RL_E_NO_DEVICE, (name, L, Ls, k, t, h)
        assert (sums == 7.0).all() and (sq == 8.0).all()


def test_the_family_check_comes_first_and_the_device_before_every_later_rule(rl):
    """pixel_family_abi's statement of the order, over this family's refused and legal arguments."""
    sums, sq = np.full((24, 3), 7.0), np.full((24, 3), 8.0)
    s, q = sums.ctypes.data, sq.ctypes.data
    one, ball = np.array([GOOD], dtype=np.float64), np.array([BALL], dtype=np.float64)
    none = np.array([[0.0, 7.0, 0.0, 0.0, 4.0, 4.0, 4.0]])
    li, sp = one.ctypes.data, ball.ctypes.data
    refused = [(0, None, 0, None, 1, 0.5, 0, s, q), (1, li, 1, None, 1, 0.5, 1, s, q), (1, li, 1, none.ctypes.data, 1, 0.5, 0, s, q), (1, li, 16, sp, 1, 0.5, 0, s, q),
               (0, None, 1, sp, 0, 0.5, 0, s, q), (0, None, 1, sp, 1, NAN, 1, s, q), (0, None, 1, sp, 1, 0.5, 0, None, None), (0, None, 1, sp, 1, 0.5, 2, s, q)]
    legal = [(0, None, 1, sp, 1, 0.5, 0, s, q), (1, li, 1, sp, 3, 1.0, 1, None, q), (1, li, 0, None, 3, 1.0, 1, s, None)]
    untouched = lambda: (sums == 7.0).all() and (sq == 8.0).all()
    family_check_comes_first(rl, "nee_mis_spheres", refused, legal, untouched)


def test_pack_sphere_lights_and_its_value_errors(rl):
    a = rl.pack_sphere_lights([((0, 7, 0), 2, 4.0), ((1.0, 2.0, 3.0), 0.5, (1.0, 2.0, 3.0))])
    assert a.dtype == np.float64 and a.shape == (2, 7) and a.flags["C_CONTIGUOUS"]
    assert a.tolist() == [[0.0, 7.0, 0.0, 2.0, 4.0, 4.0, 4.0], [1.0, 2.0, 3.0, 0.5, 1.0, 2.0, 3.0]]
    assert rl.pack_sphere_lights([]).shape == (0, 7)
    b = rl.pack_sphere_lights(a[:, :])
    assert b.shape == (2, 7) and (b == a).all()
    assert rl.pack_sphere_lights(np.zeros((0, 7))).shape == (0, 7)
    for wrong in ([((0, 7), 2, 4.0)], [((0, 7, 0, 1), 2, 4.0)], [((0, 7, 0), (2, 2), 4.0)], [((0, 7, 0), 2, (4.0, 4.0))], [((0, 7, 0), 2)], [(0, 7, 0, 2, 4, 4, 4)],
                  [((0, 7, 0), 2, "bright")], [5.0], np.zeros((2, 6)), np.zeros(7), np.zeros((1, 1, 7))):
        with pytest.raises(ValueError):
            rl.pack_sphere_lights(wrong)


def test_sphere_lights_and_the_rest_are_checked_in_python(rl, monkeypatch):
    def no_library():
        raise AssertionError("the library was reached")
    cam = _camera(rl)
    monkeypatch.setattr(rl.api, "render_lib", no_library)
    monkeypatch.setattr(rl.api, "host_lib", no_library)
    one = np.array([GOOD])
    for call in (lambda: rl.render_nee_mis(cam, object(), one, 4, sphere_lights=[((0, 7), 2, 4.0)]),
                 lambda: rl.render_pixels_nee_mis(cam, object(), [0], [0], [], 4, sphere_lights=np.zeros((1, 6))),
                 lambda: rl.render_nee_mis_device(cam, object(), [], 4, d_sums=0x1000, sphere_lights=[(1, 2, 3)]),
                 lambda: rl.render_pixels_nee_mis_device(cam, object(), 0x1000, 0x2000, 1, one, 4, d_sq=0x3000, sphere_lights=[((0, 7, 0), 2)]),
                 lambda: rl.render_nee_mis(cam, object(), [], 4, heuristic="max", sphere_lights=[BALL[:3], 2.0, 4.0]),
                 lambda: rl.render_nee_mis(cam, object(), [], 4, want=(), sphere_lights=np.array([BALL]))):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):  # without sphere_lights: today's checks, an empty `lights` is refused in Python
        rl.render_nee_mis(cam, object(), np.zeros((0, 12)), 4)


def test_last_query_names_the_sphere_kernels(rl, monkeypatch):
    api = rl.api

    class Lib:
        def __init__(self, kid):
            self.kid = kid

        def rl_debug_last_query(self, out):
            out[0], out[1] = self.kid, 3
            return 0
    for kid, name in ((13, "nee_mis_reference"), (14, "nee_mis_fast"), (15, "nee_spheres_reference"), (16, "nee_spheres_fast")):
        monkeypatch.setattr(api, "render_lib", lambda kid=kid: Lib(kid))
        assert api.last_query() == {"kernel": name, "retraced": 3}


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_sphere_renders_without_a_device_fail_loudly_and_media_scenes_come_after(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.simple_light()
    smoke = rl.World.example_scene("cornell_smoke")
    cam = _camera(rl)
    quad = [((3, 1, -2), (2, 0, 0), (0, 2, 0), 4.0)]
    ball = [((0, 7, 0), 2.0, 4.0)]
    for call in (lambda: rl.render_nee_mis(cam, world, quad, 4, sphere_lights=ball), lambda: rl.render_nee_mis(cam, world, [], 4, 0.5, "power", stats={}, sphere_lights=ball),
                 lambda: rl.render_nee_mis(cam, world, quad, 4, sphere_lights=[]),
                 lambda: rl.render_pixels_nee_mis(cam, world, [0, 1], [0, 1], quad, 4, heuristic="power", sphere_lights=ball),
                 lambda: rl.render_nee_mis_device(cam, world, [], 4, d_sums=0x1000, sphere_lights=ball),
                 lambda: rl.render_pixels_nee_mis_device(cam, world, 0x1000, 0x2000, 2, quad, 4, heuristic="power", d_sq=0x3000, stats={}, sphere_lights=ball),
                 lambda: rl.render_nee_mis(cam, smoke, quad, 4, sphere_lights=ball)):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    with pytest.raises(rl.RLError) as e:  # the C++ mirror reaches the same wall
        rl.nee.cpp_mirror_probe_spheres(6, 2, 0, quad, ball, 4, heuristic="power")
    assert "rl_init has not succeeded" in str(e.value)
