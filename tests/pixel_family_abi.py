"""What the no-device ABI tests of the pixel-render families share (tests/test_render_features_abi.py, test_render_ao_abi.py,
test_direct_abi.py, test_render_nee_abi.py, test_render_nee_mis_abi.py, test_render_nee_spheres_abi.py), and gpu_present() for every
tests/test_*_abi.py: the four entry forms of a family by its stem in the C symbols, each as f(*particular) -> rc, where `particular`
is what stands between the form's head and its trailing NULL stream / stats: the family's own arguments and its outputs."""
import ctypes as C

import numpy as np


def gpu_present():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def camera(rl, spp=2, max_depth=5):
    return rl.Camera(rl.CameraParams(aspect_ratio=1.5, image_width=6, samples_per_pixel=spp, max_depth=max_depth))


def _symbols(lib, stem):
    return (getattr(lib, "rl_rtiow_render_%s_rows" % stem), getattr(lib, "rl_rtiow_render_%s_device" % stem),
            getattr(lib, "rl_rtiow_render_pixels_%s" % stem), getattr(lib, "rl_rtiow_render_pixels_%s_device" % stem))


def forms(lib, stem, cam, scene=None):
    """The four entry points as f(*particular) -> rc with everything else valid but the scene (NULL: a later rule)."""
    rows, dev, pix, pixdev = _symbols(lib, stem)
    xs = np.arange(4, dtype=np.uint32)
    ys = np.zeros(4, dtype=np.uint32)
    c = C.byref(cam.c)
    return {
        "rows": lambda *p: rows(scene, c, 0, 0, 1, *p, None),
        "device": lambda *p: dev(scene, c, 0, 0, 1, *p, None, None),
        "pixels": lambda *p: pix(scene, c, 0, xs.ctypes.data, ys.ctypes.data, 4, *p, None),
        "pixels_device": lambda *p: pixdev(scene, c, 0, xs.ctypes.data, ys.ctypes.data, 4, *p, None, None),
    }


def with_a_later_defect(lib, stem, cam):
    """Every entry point of the family as f(*particular) -> rc, each time with ONE rule that comes later in its check sequence broken as
    well: no scene, no camera, row_step == 0, an image without pixels, row_first past the last row; a NULL list, the empty list, a list
    beyond the work counter.  -> {(form, defect): f}, and what the calls point into (to be kept alive)."""
    rows, dev, pix, pixdev = _symbols(lib, stem)
    xs, ys = np.arange(4, dtype=np.uint32), np.zeros(4, dtype=np.uint32)
    empty = type(cam.c).from_buffer_copy(cam.c)
    empty.image_width = 0
    c, e, X, Y = C.byref(cam.c), C.byref(empty), xs.ctypes.data, ys.ctypes.data
    row_heads = {"scene": (None, c, 0, 0, 1), "camera": (None, None, 0, 0, 1), "row_step": (None, c, 0, 0, 0), "empty image": (None, e, 0, 0, 1),
                 "row_first": (None, c, 0, cam.c.image_height, 1)}
    list_heads = {"scene": (None, c, 0, X, Y, 4), "camera": (None, None, 0, X, Y, 4), "xs": (None, c, 0, None, Y, 4), "ys": (None, c, 0, X, None, 4),
                  "empty list": (None, c, 0, None, None, 0), "empty image": (None, e, 0, X, Y, 4), "length": (None, c, 0, X, Y, 0xFFFF0000)}
    calls = {}
    for what, head in row_heads.items():
        calls["rows", what] = lambda *p, head=head: rows(*head, *p, None)
        calls["device", what] = lambda *p, head=head: dev(*head, *p, None, None)
    for what, head in list_heads.items():
        calls["pixels", what] = lambda *p, head=head: pix(*head, *p, None)
        calls["pixels_device", what] = lambda *p, head=head: pixdev(*head, *p, None, None)
    return calls, (xs, ys, empty)


def the_family_check_comes_first_and_the_device_before_every_later_rule(rl, stem, refused, legal, untouched, cam=None):
    """The order of each entry point's check sequence as far as a machine without a GPU shows it: what is particular to the family is
    refused first ("bad argument") whatever else is wrong with the call (no scene, no camera, row_step == 0, an empty image, row_first
    past the last row, a NULL, empty or too long list), and a call that is legal in that respect looks for the device before any of those.
    refused, legal: lists of `particular`; untouched() -> whether the outputs they point to are as they were."""
    api = rl.api
    lib = api.render_lib()
    calls, keep = with_a_later_defect(lib, stem, camera(rl) if cam is None else cam)
    assert len(calls) == 2 * 5 + 2 * 7
    for key, f in calls.items():
        for p in refused:
            assert f(*p) == api.RL_E_INVALID, (key, p)
            assert b"bad argument" in lib.rl_last_error(), (key, p, lib.rl_last_error())
    assert untouched()
    if not gpu_present():
        assert lib.rl_init(-1) == api.RL_E_NO_DEVICE
        for key, f in calls.items():
            for p in legal:
                assert f(*p) == api.RL_E_NO_DEVICE, (key, p)
                assert b"rl_init has not succeeded" in lib.rl_last_error(), (key, p, lib.rl_last_error())
        assert untouched()
