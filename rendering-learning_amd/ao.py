"""Ambient-occlusion renders (include/rl_render.h "Ambient-occlusion renders", rl_rtiow_render_ao*).

Per pixel, over the camera's samples_per_pixel jittered camera rays (those of render_independent and render_features), `hits` counts the rays
that hit and `open` counts, over the ao_rays directions (normal + random_unit_vector).normalize() drawn from the sample's own stream at each
first hit, the rays that find nothing within `radius` at the camera ray's time.  Both are integers, so renders that continue each other
(first_sample) add exactly: AmbientOcclusion.merge.
"""
import functools

import numpy as np

from . import api


class AmbientOcclusion:
    """open, hits: uint32 arrays of one shape (None where not asked for); ao_rays: the K of the render(s) they come from."""

    def __init__(self, open, hits, ao_rays):
        self.open, self.hits, self.ao_rays = open, hits, int(ao_rays)

    def visibility(self, miss=1.0):
        """open / (ao_rays * hits) as float64: 1 = nothing within the radius, 0 = closed in; `miss` where no camera ray hit."""
        if self.open is None or self.hits is None:
            raise ValueError("visibility needs both counts")
        den = self.hits.astype(np.float64) * float(self.ao_rays)
        return np.where(self.hits > 0, self.open / np.where(self.hits > 0, den, 1.0), float(miss))

    def merge(self, other):
        """The counts of two renders of the same pixels and ao_rays over disjoint sample ranges: exactly those of one render over both."""
        if other.ao_rays != self.ao_rays:
            raise ValueError(f"ao_rays differ: {self.ao_rays} and {other.ao_rays}")
        if (self.open is None) != (other.open is None) or (self.hits is None) != (other.hits is None):
            raise ValueError("the two renders hold different outputs")

        def add(a, b):
            if a is None:
                return None
            if a.shape != b.shape:
                raise ValueError(f"shapes differ: {a.shape} and {b.shape}")
            s = a.astype(np.uint64) + b
            if s.size and int(s.max()) > 0xFFFFFFFF:
                raise OverflowError("a merged count does not fit 32 bits")
            return s.astype(np.uint32)

        return AmbientOcclusion(add(self.open, other.open), add(self.hits, other.hits), self.ao_rays)


OUTPUTS = {"open": (np.uint32, ()), "hits": (np.uint32, ())}  # name -> (dtype, trailing shape), in the C order
_outputs = functools.partial(api.host_outputs, OUTPUTS)


def render_ao(camera, world, ao_rays, radius, first_sample=0, row_first=0, row_step=1, stats=None, want=None, allow_degenerate=False):
    """Compact shard rows -> AmbientOcclusion([nrows, W]).  Always a counting call (reference-order trace), as Camera.render_features."""
    a = api.rows_form("rl_rtiow_render_ao_rows", camera, world, first_sample, row_first, row_step, (int(ao_rays), float(radius)), _outputs, want,
                      stats=stats, allow_degenerate=allow_degenerate)
    return AmbientOcclusion(*a.values(), ao_rays)


def render_ao_device(camera, world, ao_rays, radius, stream=0, row_first=0, row_step=1, first_sample=0, stats=None, allow_degenerate=False, *, d_open=0,
                     d_hits=0):
    """Outputs stay in HBM: device pointers of nrows*W uint32 each; 0 = not wanted.  Async and counter-free unless stats is a dict."""
    api.rows_device_form("rl_rtiow_render_ao_device", camera, world, first_sample, row_first, row_step, (int(ao_rays), float(radius)), (d_open, d_hits),
                         stream, stats=stats, allow_degenerate=allow_degenerate)


def render_pixels_ao(camera, world, xs, ys, ao_rays, radius, first_sample=0, stats=None, want=None, allow_degenerate=False):
    """The counts of pixels (xs[i], ys[i]), [n]: what render_ao holds at [ys[i], xs[i]].  The list rules are render_pixels_features'.
    stats (a dict): a counting call; without it the call is counter-free and may take the fast walks (api.last_query())."""
    a = api.list_form("rl_rtiow_render_pixels_ao", camera, world, first_sample, xs, ys, (int(ao_rays), float(radius)), _outputs, want, stats=stats,
                      allow_degenerate=allow_degenerate)
    return AmbientOcclusion(*a.values(), ao_rays)


def render_pixels_ao_device(camera, world, d_xs, d_ys, n, ao_rays, radius, stream=0, first_sample=0, stats=None, allow_degenerate=False, *, d_open=0, d_hits=0):
    """d_xs / d_ys: device pointers of n uint32; outputs as render_ao_device with n pixels.  Async unless stats is a dict; an element outside
    the image is written as zeros in every given output."""
    api.list_device_form("rl_rtiow_render_pixels_ao_device", camera, world, first_sample, d_xs, d_ys, n, (int(ao_rays), float(radius)), (d_open, d_hits),
                         stream, stats=stats, allow_degenerate=allow_degenerate)
