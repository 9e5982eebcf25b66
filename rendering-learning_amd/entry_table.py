"""The per-pixel entry table's time slices and its reuse across calls (csrc/rl_pixel_entry.h "Time slices"): the switches
and read-backs that tests and tools use.  api.set_pixel_entry / set_pixel_entry_sphere / pixel_entry_table are the table's older ones.
"""
import ctypes as C

import numpy as np

from . import api


def set_slices(slices):
    """rl_debug_set_pixel_entry_time: 1, 2, 4 or 8 entry words per pixel, one per slice of the shutter interval (any other value: the default,
    4); 1 is the one word for all times.  The same switch as RL_PIXEL_ENTRY_TIME."""
    api.render_lib().rl_debug_set_pixel_entry_time(int(slices))


def set_reuse(on):
    """rl_debug_set_pixel_entry_reuse: False makes every render call build its table; True (the default) lets a call that repeats the camera,
    rows and switches of the scene's last build read that table as it is.  The same switch as RL_PIXEL_ENTRY_REUSE."""
    api.render_lib().rl_debug_set_pixel_entry_reuse(int(bool(on)))


def builds():
    """rl_debug_pixel_entry_builds: how many table kernels this process has launched; a render that reuses its scene's table adds none."""
    return int(api.render_lib().rl_debug_pixel_entry_builds())


def sliced_table(world, n_pixels, slices):
    """rl_debug_pixel_entry_time_read: the [n_pixels, slices] words of the world's most recent fast-traversal render, built with that many slices."""
    out = np.zeros((int(n_pixels), int(slices)), dtype=np.uint32)
    api._check(api.render_lib().rl_debug_pixel_entry_time_read(world.device(), out.ctypes.data_as(C.c_void_p), int(n_pixels), int(slices)))
    return out


def census(world):
    """rl_debug_pixel_entry_census (verify build, after a counting render behind rl_debug_fast_stats): camera LEAF visits that ended at disc < 0 on
    a moving sphere; those of them, and of the ones on stationary spheres, whose leaf the all-times table holds for the pixel; and of the moving
    ones the table holds, those the ball of the sample's time slice leaves out, for 2, 4 and 8 slices."""
    out = (C.c_uint64 * 6)()
    api._check(api.render_lib().rl_debug_pixel_entry_census(world.device(), out))
    return {"moving": int(out[0]), "moving_in_table": int(out[1]), "static_in_table": int(out[2]), "sliced_out": {2: int(out[3]), 4: int(out[4]), 8: int(out[5])}}
