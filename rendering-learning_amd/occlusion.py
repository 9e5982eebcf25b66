"""Occlusion queries (include/rl_render.h rl_rtiow_occluded_rays*): "is anything in the way" for buffers of rays.

occluded[i] is Hittable::hit(&rays[i], &Interval{tmin, tmax}).is_some() on the scene root — the `hit` field of World.hit_rays' record for
the same ray and interval, at one byte per ray and without the closest hit.  Rays are used as given: dirs = targets - origins with
tmax = 1 tests the segments between the two point sets (shadow rays towards a sampled light, visibility between probes).
"""
import ctypes as C

import numpy as np

from . import api


def occluded_rays(world, origins, dirs, times=None, tmin=1e-10, tmax=float("inf"), stats=None, allow_degenerate=False):
    """-> bool[n].  Without `stats` the call is counter-free: the any-hit walk serves it where it applies (same bytes, see api.last_query());
    with a dict it runs the reference-order fold and fills in the counters World.hit_rays reports for the same batch."""
    rays = api.pack_rays(origins, dirs, times)
    out = np.zeros(rays.shape[0], dtype=np.uint8)
    api._call(api.render_lib().rl_rtiow_occluded_rays, world.device(), rays.ctypes.data, rays.shape[0], tmin, tmax, out.ctypes.data, stats=stats,
              allow_degenerate=allow_degenerate)
    return out.astype(bool)


def occluded_rays_device(world, d_rays, d_out, n, tmin=1e-10, tmax=float("inf"), stream=0, stats=None, allow_degenerate=False):
    """Device buffers (n rl_ray in, n bytes out; e.g. torch tensors' data_ptr).  Asynchronous unless stats is a dict."""
    api._call(api.render_lib().rl_rtiow_occluded_rays_device, world.device(), C.c_void_p(d_rays), n, tmin, tmax, C.c_void_p(d_out), C.c_void_p(stream),
              stats=stats, allow_degenerate=allow_degenerate)
