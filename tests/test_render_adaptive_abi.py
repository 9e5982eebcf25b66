"""CPU tier: the adaptive renders (rl_rtiow_render_adaptive_rows / _device; include/rl_render.h "Adaptive renders") are
exported, declared in include/rl_render.h, listed in api.RENDER_SYMBOLS, wired into the Python and C++ layers, refuse every invalid rule
with RL_E_INVALID whether or not a device is present, and fail LOUDLY (RL_E_NO_DEVICE, no CPU fallback) when no GPU is present;
api.Adaptive's host arithmetic on hand-made arrays."""
import ctypes
import os
import re

import numpy as np
import pytest
from pixel_family_abi import gpu_present

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"rl_rtiow_render_adaptive_rows": 10, "rl_rtiow_render_adaptive_device": 11}
PROBE_ARGS = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_double, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p,
              ctypes.c_void_p]


def test_render_adaptive_entry_points_are_exported_declared_and_listed(rl):
    lib = rl.api.render_lib()
    text = open(os.path.join(ROOT, "include", "rl_render.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s, nargs in NEW.items():
        assert hasattr(lib, s), s
        assert s in rl.api.RENDER_SYMBOLS, s
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % s, header)
        assert m, s
        assert len(m.group(1).split(",")) == nargs, (s, m.group(1))
        assert len(getattr(lib, s).argtypes) == nargs, s
    assert lib.rl_abi_version() == 6  # the additions are backward compatible
    # the rule's struct: four fields in the header's order, 24 bytes, mirrored by the ctypes structure
    m = re.search(r"typedef\s+struct\s+rl_rtiow_adaptive\s*\{([^}]*)\}\s*rl_rtiow_adaptive\s*;", header)
    assert m
    assert re.findall(r"\b(\w+)\s*;", m.group(1)) == ["min_samples", "check_every", "abs_variance", "rel_variance"]
    assert [f[0] for f in rl.api.RtiowAdaptive._fields_] == ["min_samples", "check_every", "abs_variance", "rel_variance"]
    assert ctypes.sizeof(rl.api.RtiowAdaptive) == 24
    assert hasattr(rl.api.host_lib(), "rlh_render_adaptive_probe")
    for name in ("render_adaptive", "render_adaptive_device"):
        assert callable(getattr(rl.Camera, name)), name
    assert rl.Adaptive is rl.api.Adaptive
    assert callable(rl.api.set_lpt)
    rl.api.set_lpt(True)  # the default; a switch of the library, no device needed


def _rules(api):
    R = api.RtiowAdaptive
    return {"min_samples 0": R(0, 4, 1.0, 0.0), "min_samples 1": R(1, 4, 1.0, 0.0), "check_every 0": R(4, 0, 1.0, 0.0),
            "negative abs": R(4, 4, -1e-300, 0.0), "negative rel": R(4, 4, 0.0, -1.0), "NaN abs": R(4, 4, float("nan"), 0.0),
            "NaN rel": R(4, 4, 0.0, float("nan")), "-inf abs": R(4, 4, float("-inf"), 0.0)}


def test_every_invalid_rule_is_refused_with_outputs_untouched(rl):
    """RL_E_INVALID for a NULL rule, a NULL output, min_samples < 2, check_every == 0 and a negative or NaN bound — the rule is looked at
    before anything else, so the answer is the same with and without a device."""
    api = rl.api
    lib = api.render_lib()
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    npix = cam.c.image_width * cam.c.image_height
    sums, sq, counts = np.full(npix * 3, 7.0), np.full(npix * 3, 7.0), np.full(npix, 7, dtype=np.uint32)
    c = ctypes.byref(cam.c)
    dev = None  # without a device there is no scene either: the rule is still looked at first
    if gpu_present():
        rl.init(0)
        dev = world.device()
    S, Q, N = sums.ctypes.data, sq.ctypes.data, counts.ctypes.data
    good = api.RtiowAdaptive(4, 4, 1.0, 0.0)
    for what, rule in _rules(api).items():
        assert lib.rl_rtiow_render_adaptive_rows(dev, c, 0, 0, 1, ctypes.byref(rule), S, Q, N, None) == api.RL_E_INVALID, what
        assert lib.rl_rtiow_render_adaptive_device(dev, c, 0, 0, 1, ctypes.byref(rule), S, Q, N, None, None) == api.RL_E_INVALID, what
    assert lib.rl_rtiow_render_adaptive_rows(dev, c, 0, 0, 1, None, S, Q, N, None) == api.RL_E_INVALID
    assert lib.rl_rtiow_render_adaptive_device(dev, c, 0, 0, 1, None, S, Q, N, None, None) == api.RL_E_INVALID
    for outs in ((None, Q, N), (S, None, N), (S, Q, None)):
        assert lib.rl_rtiow_render_adaptive_rows(dev, c, 0, 0, 1, ctypes.byref(good), *outs, None) == api.RL_E_INVALID, outs
        assert lib.rl_rtiow_render_adaptive_device(dev, c, 0, 0, 1, ctypes.byref(good), *outs, None, None) == api.RL_E_INVALID, outs
    assert (sums == 7.0).all() and (sq == 7.0).all() and (counts == 7).all()
    if dev is None:
        return
    # the Python layer raises what the library returns (it creates the scene first, which takes a device)
    for kw in ({"min_samples": 1, "check_every": 4}, {"min_samples": 4, "check_every": 0}, {"min_samples": 4, "check_every": 4, "abs_variance": -1.0},
               {"min_samples": 4, "check_every": 4, "rel_variance": float("nan")}):
        with pytest.raises(rl.RLError) as e:
            cam.render_adaptive(world, **kw)
        assert e.value.code == api.RL_E_INVALID, kw


@pytest.mark.skipif(gpu_present(), reason="GPU present: the failure path is not reachable")
def test_render_adaptive_without_a_device_fails_loudly(rl):
    api = rl.api
    lib = api.render_lib()
    assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
    world = rl.World.golden_test_scene()
    cam = rl.Camera(world.params)
    for call in (lambda: cam.render_adaptive(world, 4, 4, abs_variance=1e-3),
                 lambda: cam.render_adaptive(world, 2, 1, rel_variance=1e-3, first_sample=3, row_first=1, row_step=3, stats={}),
                 lambda: cam.render_adaptive_device(world, 4, 4, 0x1000, 0x2000, 0x3000, abs_variance=1e-3),
                 lambda: cam.render_adaptive_device(world, 4, 4, 0x1000, 0x2000, 0x3000, stats={})):
        with pytest.raises(rl.RLError) as e:
            call()
        assert e.value.code == api.RL_E_NO_DEVICE
    # the C ABI itself, with valid host buffers and a valid rule: all three outputs untouched
    npix = cam.c.image_width * cam.c.image_height
    sums, sq, counts = np.zeros(npix * 3), np.zeros(npix * 3), np.zeros(npix, dtype=np.uint32)
    c = ctypes.byref(cam.c)
    rule = api.RtiowAdaptive(4, 4, 1e-3, 0.0)
    assert lib.rl_rtiow_render_adaptive_rows(None, c, 0, 0, 1, ctypes.byref(rule), sums.ctypes.data, sq.ctypes.data, counts.ctypes.data, None) == api.RL_E_NO_DEVICE
    assert lib.rl_rtiow_render_adaptive_device(None, c, 0, 0, 1, ctypes.byref(rule), sums.ctypes.data, sq.ctypes.data, counts.ctypes.data, None,
                                               None) == api.RL_E_NO_DEVICE
    assert not sums.any() and not sq.any() and not counts.any()
    # the C++ mirror reaches the same wall
    H = api.host_lib()
    H.rlh_render_adaptive_probe.argtypes = PROBE_ARGS
    assert H.rlh_render_adaptive_probe(12, 8, 4, 2, 1e-3, 0.0, sums.ctypes.data, sq.ctypes.data, counts.ctypes.data) == -1
    assert not sums.any() and not sq.any() and not counts.any()


def test_adaptive_mean_and_variance_of_mean_on_hand_made_arrays(rl):
    Adaptive = rl.api.Adaptive
    # pixel 0: samples {1, 2, 3, 4} in channel 0, {2, 2, 2, 2} in channel 1, {0, 0, 0, 8} in channel 2 (n = 4);
    # pixel 1: samples {1, 3} in every channel (n = 2)
    a = Adaptive(np.array([[[10.0, 8.0, 8.0], [4.0, 4.0, 4.0]]]), np.array([[[30.0, 16.0, 64.0], [10.0, 10.0, 10.0]]]), np.array([[4, 2]], dtype=np.uint32))
    assert a.mean().tobytes() == np.array([[[2.5, 2.0, 2.0], [2.0, 2.0, 2.0]]]).tobytes()
    # sample variances 5/3, 0, 16 over n = 4 and 2 over n = 2: exact in binary64 up to the one division by 3
    want = np.array([[[(30.0 - 100.0 / 4) / 3 / 4, 0.0, (64.0 - 64.0 / 4) / 3 / 4], [1.0, 1.0, 1.0]]])
    assert a.variance_of_mean().tobytes() == want.tobytes()
    assert want[0, 0, 2] == 4.0
    # the same numbers as Moments gives pixel by pixel
    for px, n in ((0, 4), (1, 2)):
        m = rl.api.Moments(n, a.sums[:, px:px + 1], a.sq[:, px:px + 1])
        assert m.variance_of_mean().tobytes() == a.variance_of_mean()[:, px:px + 1].tobytes()
    # a pixel with fewer than 2 samples has no sample variance
    with pytest.raises(ValueError):
        Adaptive(np.zeros((1, 2, 3)), np.zeros((1, 2, 3)), np.array([[4, 1]], dtype=np.uint32)).variance_of_mean()
    # round-off never takes the estimate below zero: three equal samples of 0.1
    c = np.float64(0.1)
    neg = Adaptive(np.array([[[(c + c) + c, 0.3, 0.3]]]), np.array([[[(c * c + c * c) + c * c, 0.03 - 1e-17, 0.03 - 1e-17]]]), np.array([[3]], dtype=np.uint32))
    assert (neg.variance_of_mean() >= 0).all()
