"""Direct-lighting renders (include/rl_render.h "Direct-lighting renders", rl_rtiow_render_direct*).

Per pixel, over the camera's samples_per_pixel jittered camera rays (those of render_independent, render_features and render_ao), `hits` counts
the rays that hit and, over light_samples points drawn from the sample's own stream on each quad light at every first hit, `unshadowed` sums
E * cos cos_l area / |d|^2 and `direct` sums the same terms where the segment to the light point is free at the camera ray's time.  The sums
are DEMODULATED: no albedo and no 1/pi (DirectLight.radiance applies them).  hits of renders that continue each other (first_sample) add
exactly; the float sums of a call are that call's own fold.
"""
import ctypes as C
import functools
import math

import numpy as np

from . import api

MAX_LIGHTS = 16  # RL_DIRECT_MAX_LIGHTS: the lights travel by value in the launch
SEG_TMAX = 1.0 - 1e-6  # the segments' closed end: a light that is also geometry of the scene sits at t = 1


def pack_lights(lights):
    """[(Q, u, v, E), ..] -> float64 [L, 12]: the parallelogram Q + a u + b v (Quad::new(Q, u, v, ..)) and the radiance it emits; E may be
    a scalar (grey).  An [L, 12] array passes through.  Shape errors are the caller's: ValueError."""
    if isinstance(lights, np.ndarray) and lights.ndim == 2:
        out = np.ascontiguousarray(lights, dtype=np.float64)
    else:
        rows = []
        for light in lights:
            if len(light) != 4:
                raise ValueError("a light is (Q, u, v, E)")
            q, u, v, e = (np.asarray(p, dtype=np.float64) for p in light)
            if e.ndim == 0:
                e = np.full(3, float(e))
            if any(p.shape != (3,) for p in (q, u, v, e)):
                raise ValueError("Q, u, v and E have three components each")
            rows.append(np.concatenate([q, u, v, e]))
        out = np.array(rows, dtype=np.float64).reshape(len(rows), 12)
    if out.ndim != 2 or out.shape[1] != 12 or not 1 <= out.shape[0] <= MAX_LIGHTS:
        raise ValueError(f"lights must be [L, 12] with 1 <= L <= {MAX_LIGHTS}, not {out.shape}")
    return out


class DirectLight:
    """direct, unshadowed: float64 [..., 3]; hits: uint32 [...] (None where not asked for); light_samples: the K of the render(s)."""

    def __init__(self, direct, unshadowed, hits, light_samples):
        self.direct, self.unshadowed, self.hits, self.light_samples = direct, unshadowed, hits, int(light_samples)

    def irradiance(self, miss=0.0):
        """direct / (light_samples * hits), [..., 3]: the demodulated irradiance estimate at the first hits; `miss` where no camera ray hit."""
        if self.direct is None or self.hits is None:
            raise ValueError("irradiance needs direct and hits")
        den = self.hits.astype(np.float64) * float(self.light_samples)
        hit = (self.hits > 0)[..., None]
        return np.where(hit, self.direct / np.where(hit, den[..., None], 1.0), float(miss))

    def shadow(self):
        """direct / unshadowed, [..., 3]: 1 = fully lit, 0 = in shadow; 1 where unshadowed == 0 (nothing to shadow)."""
        if self.direct is None or self.unshadowed is None:
            raise ValueError("shadow needs direct and unshadowed")
        lit = self.unshadowed != 0.0
        return np.where(lit, self.direct / np.where(lit, self.unshadowed, 1.0), 1.0)

    def radiance(self, albedo):
        """albedo * irradiance / pi: the Lambertian direct radiance for an albedo [..., 3] (e.g. render_features' albedo / hit_count)."""
        return np.asarray(albedo, dtype=np.float64) * self.irradiance() / math.pi

    def merge(self, other):
        """Two renders of the same pixels, lights and light_samples over disjoint sample ranges.  hits are exactly those of one render over
        both ranges.  The float sums are the SUM OF TWO FOLDS, each rounded on its own: the same estimate, but not the bits one call
        over both ranges would give (that call folds all its terms in one chain)."""
        if other.light_samples != self.light_samples:
            raise ValueError(f"light_samples differ: {self.light_samples} and {other.light_samples}")
        mine, theirs = (self.direct, self.unshadowed, self.hits), (other.direct, other.unshadowed, other.hits)
        if any((a is None) != (b is None) for a, b in zip(mine, theirs)):
            raise ValueError("the two renders hold different outputs")
        if any(a is not None and a.shape != b.shape for a, b in zip(mine, theirs)):
            raise ValueError("shapes differ")
        hits = None
        if self.hits is not None:
            s = self.hits.astype(np.uint64) + other.hits
            if s.size and int(s.max()) > 0xFFFFFFFF:
                raise OverflowError("a merged count does not fit 32 bits")
            hits = s.astype(np.uint32)
        add = lambda a, b: None if a is None else a + b
        return DirectLight(add(self.direct, other.direct), add(self.unshadowed, other.unshadowed), hits, self.light_samples)


OUTPUTS = {"direct": (np.float64, (3,)), "unshadowed": (np.float64, (3,)), "hits": (np.uint32, ())}  # name -> (dtype, trailing shape), in the C order
_outputs = functools.partial(api.host_outputs, OUTPUTS)


def _light_args(lights, light_samples, seg_tmax):
    """-> (what must stay alive over the call, the C arguments n_lights, lights, light_samples, seg_tmax); also the NEE families'."""
    L = pack_lights(lights)
    return L, (L.shape[0], C.c_void_p(L.ctypes.data), int(light_samples), float(seg_tmax))


def render_direct(camera, world, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0, row_first=0, row_step=1, stats=None, want=None,
                  allow_degenerate=False):
    """Compact shard rows -> DirectLight([nrows, W(, 3)]).  Always a counting call (reference-order trace), as render_ao."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    a = api.rows_form("rl_rtiow_render_direct_rows", camera, world, first_sample, row_first, row_step, args, _outputs, want, stats=stats,
                      allow_degenerate=allow_degenerate)
    return DirectLight(*a.values(), light_samples)


def render_direct_device(camera, world, lights, light_samples, seg_tmax=SEG_TMAX, stream=0, row_first=0, row_step=1, first_sample=0, stats=None,
                         allow_degenerate=False, *, d_direct=0, d_unshadowed=0, d_hits=0):
    """Outputs stay in HBM: device pointers of nrows*W*3 float64 (direct, unshadowed) and nrows*W uint32 (hits); 0 = not wanted.  Async and
    counter-free unless stats is a dict.  The lights are copied into the launch: nothing of `lights` is read after the call returns."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    api.rows_device_form("rl_rtiow_render_direct_device", camera, world, first_sample, row_first, row_step, args, (d_direct, d_unshadowed, d_hits), stream,
                         stats=stats, allow_degenerate=allow_degenerate)


def render_pixels_direct(camera, world, xs, ys, lights, light_samples, seg_tmax=SEG_TMAX, first_sample=0, stats=None, want=None, allow_degenerate=False):
    """The values of pixels (xs[i], ys[i]), [n(, 3)]: what render_direct holds at [ys[i], xs[i]].  The list rules are render_pixels_ao's.
    stats (a dict): a counting call; without it the call is counter-free and may take the fast walks (api.last_query())."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    a = api.list_form("rl_rtiow_render_pixels_direct", camera, world, first_sample, xs, ys, args, _outputs, want, stats=stats,
                      allow_degenerate=allow_degenerate)
    return DirectLight(*a.values(), light_samples)


def render_pixels_direct_device(camera, world, d_xs, d_ys, n, lights, light_samples, seg_tmax=SEG_TMAX, stream=0, first_sample=0, stats=None,
                                allow_degenerate=False, *, d_direct=0, d_unshadowed=0, d_hits=0):
    """d_xs / d_ys: device pointers of n uint32; outputs as render_direct_device with n pixels.  Async unless stats is a dict; an element
    outside the image is written as zeros in every given output."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    api.list_device_form("rl_rtiow_render_pixels_direct_device", camera, world, first_sample, d_xs, d_ys, n, args, (d_direct, d_unshadowed, d_hits),
                         stream, stats=stats, allow_degenerate=allow_degenerate)


def cpp_mirror_probe(width, spp, first_sample, lights, light_samples, seg_tmax=SEG_TMAX):
    """rtiow::render_direct of the C++ mirror on golden_test_scene at image_width = width -> DirectLight([H, W(, 3)]) (the height is the
    scene's aspect ratio's).  For tests of the mirror; RLError carries rlh_last_error."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    return api.mirror_probe(api.World.golden_test_scene, width, spp, "rlh_direct_probe", (int(first_sample), *args), _outputs, DirectLight, light_samples)
