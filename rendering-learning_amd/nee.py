"""NEE path renders (include/rl_render.h "NEE path renders", rl_rtiow_render_nee*).

Camera::ray_color with next-event estimation: per pixel, over the camera's samples_per_pixel jittered camera rays (those of render_independent,
render_features, render_ao and render_direct), a path of at most max_depth vertices that, at every Lambertian vertex but the last, connects to
light_samples points drawn on each quad light from the sample's own stream (render_direct's draws, geometry term and shadow segment) and in
exchange does not count the emission its scattered ray finds.  `lights` must list every DiffuseLight surface of the scene for the estimate
to have ray_color's expectation.  The outputs are render_moments': the sum of the sample colours and the sum of their squares.

render_nee_mis* weight the light points against the scattered ray and connect that ray to the lights it crosses (multiple importance
sampling): the same expectation, and no sample larger than what the lights emit.  With sphere_lights= they also take
sphere lights (pack_sphere_lights): stationary spheres that emit outward only.
"""
import ctypes as C
import functools

import numpy as np

from . import api
from .direct import SEG_TMAX, _light_args, pack_lights


class PathNEE:
    """sums, sq: float64 [..., 3] (None where not asked for); samples: the camera's samples_per_pixel; light_samples: the K of the render."""

    def __init__(self, sums, sq, samples, light_samples):
        self.sums, self.sq, self.samples, self.light_samples = sums, sq, int(samples), int(light_samples)

    def moments(self):
        """-> api.Moments(samples, sums, sq): what variance_of_mean, merge and denoise_render take from render_moments."""
        if self.sums is None or self.sq is None:
            raise ValueError("moments needs sums and sq")
        return api.Moments(self.samples, self.sums, self.sq)

    def mean(self):
        if self.sums is None:
            raise ValueError("mean needs sums")
        return self.sums / float(self.samples)


OUTPUTS = {"sums": (np.float64, (3,)), "sq": (np.float64, (3,))}  # name -> (dtype, trailing shape), in the C order
_outputs = functools.partial(api.host_outputs, OUTPUTS)


def render_nee(camera, world, lights, light_samples=1, seg_tmax=SEG_TMAX, first_sample=0, row_first=0, row_step=1, stats=None, want=None,
               allow_degenerate=False):
    """Compact shard rows -> PathNEE([nrows, W, 3]).  Always a counting call (reference-order trace), as render_direct."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    a = api.rows_form("rl_rtiow_render_nee_rows", camera, world, first_sample, row_first, row_step, args, _outputs, want, stats=stats,
                      allow_degenerate=allow_degenerate)
    return PathNEE(*a.values(), camera.c.samples_per_pixel, light_samples)


def render_nee_device(camera, world, lights, light_samples=1, seg_tmax=SEG_TMAX, stream=0, row_first=0, row_step=1, first_sample=0, stats=None,
                      allow_degenerate=False, *, d_sums=0, d_sq=0):
    """Outputs stay in HBM: device pointers of nrows*W*3 float64 each; 0 = not wanted.  Async and counter-free unless stats is a dict.  The
    lights are copied into the launch: nothing of `lights` is read after the call returns."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    api.rows_device_form("rl_rtiow_render_nee_device", camera, world, first_sample, row_first, row_step, args, (d_sums, d_sq), stream, stats=stats,
                         allow_degenerate=allow_degenerate)


def render_pixels_nee(camera, world, xs, ys, lights, light_samples=1, seg_tmax=SEG_TMAX, first_sample=0, stats=None, want=None, allow_degenerate=False):
    """The values of pixels (xs[i], ys[i]), [n, 3]: what render_nee holds at [ys[i], xs[i]].  The list rules are render_pixels_direct's.
    stats (a dict): a counting call; without it the call is counter-free and may take the fast walks (api.last_query())."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    a = api.list_form("rl_rtiow_render_pixels_nee", camera, world, first_sample, xs, ys, args, _outputs, want, stats=stats, allow_degenerate=allow_degenerate)
    return PathNEE(*a.values(), camera.c.samples_per_pixel, light_samples)


def render_pixels_nee_device(camera, world, d_xs, d_ys, n, lights, light_samples=1, seg_tmax=SEG_TMAX, stream=0, first_sample=0, stats=None,
                             allow_degenerate=False, *, d_sums=0, d_sq=0):
    """d_xs / d_ys: device pointers of n uint32; outputs as render_nee_device with n pixels.  Async unless stats is a dict; an element outside
    the image is written as zeros in every given output."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    api.list_device_form("rl_rtiow_render_pixels_nee_device", camera, world, first_sample, d_xs, d_ys, n, args, (d_sums, d_sq), stream, stats=stats,
                         allow_degenerate=allow_degenerate)


# ----------------------------------------------------------------------------- with multiple importance sampling
HEURISTICS = {"balance": 0, "power": 1}  # RL_MIS_BALANCE, RL_MIS_POWER


def _heuristic(heuristic):
    if not isinstance(heuristic, str) or heuristic not in HEURISTICS:
        raise ValueError(f"heuristic must be one of {tuple(HEURISTICS)}")
    return HEURISTICS[heuristic]


def pack_sphere_lights(sphere_lights):
    """[(C, r, E), ...] -> float64 [Ls, 7] = C[3], r, E[3], the layout of the sphere_lights argument; E may be a scalar (a grey light).  An
    [Ls, 7] array passes through.  Ls may be 0 (the call then is render_nee_mis' own)."""
    if isinstance(sphere_lights, np.ndarray):
        a = np.ascontiguousarray(sphere_lights, dtype=np.float64)
        if a.ndim != 2 or a.shape[1] != 7:
            raise ValueError(f"sphere_lights must be [Ls, 7] (C, r, E); got shape {a.shape}")
        return a
    rows = []
    for i, light in enumerate(sphere_lights):
        try:
            c, r, e = light
            c = np.asarray(c, dtype=np.float64).reshape(-1)
            r = np.asarray(r, dtype=np.float64)
            e = np.asarray(e, dtype=np.float64)
        except (TypeError, ValueError) as err:
            raise ValueError(f"sphere light {i}: expected (C, r, E)") from err
        if c.shape != (3,) or r.shape != () or e.shape not in ((), (3,)):
            raise ValueError(f"sphere light {i}: C is 3 numbers, r is one, E is one or 3")
        rows.append(np.concatenate([c, r.reshape(1), np.broadcast_to(e, (3,))]))
    return np.ascontiguousarray(np.array(rows, dtype=np.float64).reshape(len(rows), 7))


def _mis_args(lights, sphere_lights, light_samples, seg_tmax, heuristic):
    """-> (the family's stem in the C symbols, what must stay alive over the call, the C arguments from n_lights to heuristic):
    render_nee_mis*'s own symbols and checks without sphere_lights, else the _spheres symbols, where `lights` may be empty."""
    h = _heuristic(heuristic)
    if sphere_lights is None:
        keep, args = _light_args(lights, light_samples, seg_tmax)
        return "nee_mis", keep, (*args, h)
    Sp = pack_sphere_lights(sphere_lights)
    L = pack_lights(lights) if len(lights) else np.zeros((0, 12), dtype=np.float64)
    ptr = lambda a: C.c_void_p(a.ctypes.data) if a.shape[0] else None
    return "nee_mis_spheres", (L, Sp), (L.shape[0], ptr(L), Sp.shape[0], ptr(Sp), int(light_samples), float(seg_tmax), h)


def render_nee_mis(camera, world, lights, light_samples=1, seg_tmax=SEG_TMAX, heuristic="balance", first_sample=0, row_first=0, row_step=1, stats=None,
                   want=None, allow_degenerate=False, sphere_lights=None):
    """render_nee with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance sampling"; DESIGN.md
    §3.23): every light point is weighted against the scattered ray's density, and the scattered ray of a vertex that sampled the lights is
    connected to each light it crosses with the complementary weight.  heuristic: "balance" or "power" (exponent 2).  The same draws, the
    same path and the same expectation as render_nee; no single sample exceeds what the lights emit.  -> PathNEE([nrows, W, 3]).
    sphere_lights (pack_sphere_lights' input; include/rl_render.h "NEE path renders with sphere lights"): spheres that emit
    outward only, sampled by area and met by the scattered ray; `lights` may then be empty."""
    stem, keep, args = _mis_args(lights, sphere_lights, light_samples, seg_tmax, heuristic)
    a = api.rows_form(f"rl_rtiow_render_{stem}_rows", camera, world, first_sample, row_first, row_step, args, _outputs, want, stats=stats,
                      allow_degenerate=allow_degenerate)
    return PathNEE(*a.values(), camera.c.samples_per_pixel, light_samples)


def render_nee_mis_device(camera, world, lights, light_samples=1, seg_tmax=SEG_TMAX, heuristic="balance", stream=0, row_first=0, row_step=1, first_sample=0,
                          stats=None, allow_degenerate=False, *, d_sums=0, d_sq=0, sphere_lights=None):
    """render_nee_device's buffers and asynchrony, render_nee_mis's estimate."""
    stem, keep, args = _mis_args(lights, sphere_lights, light_samples, seg_tmax, heuristic)
    api.rows_device_form(f"rl_rtiow_render_{stem}_device", camera, world, first_sample, row_first, row_step, args, (d_sums, d_sq), stream, stats=stats,
                         allow_degenerate=allow_degenerate)


def render_pixels_nee_mis(camera, world, xs, ys, lights, light_samples=1, seg_tmax=SEG_TMAX, heuristic="balance", first_sample=0, stats=None, want=None,
                          allow_degenerate=False, sphere_lights=None):
    """The values of pixels (xs[i], ys[i]), [n, 3]: what render_nee_mis holds at [ys[i], xs[i]].  The list rules and the meaning of stats are
    render_pixels_nee's."""
    stem, keep, args = _mis_args(lights, sphere_lights, light_samples, seg_tmax, heuristic)
    a = api.list_form(f"rl_rtiow_render_pixels_{stem}", camera, world, first_sample, xs, ys, args, _outputs, want, stats=stats,
                      allow_degenerate=allow_degenerate)
    return PathNEE(*a.values(), camera.c.samples_per_pixel, light_samples)


def render_pixels_nee_mis_device(camera, world, d_xs, d_ys, n, lights, light_samples=1, seg_tmax=SEG_TMAX, heuristic="balance", stream=0, first_sample=0,
                                 stats=None, allow_degenerate=False, *, d_sums=0, d_sq=0, sphere_lights=None):
    """render_pixels_nee_device's buffers, list rules and asynchrony, render_nee_mis's estimate."""
    stem, keep, args = _mis_args(lights, sphere_lights, light_samples, seg_tmax, heuristic)
    api.list_device_form(f"rl_rtiow_render_pixels_{stem}_device", camera, world, first_sample, d_xs, d_ys, n, args, (d_sums, d_sq), stream, stats=stats,
                         allow_degenerate=allow_degenerate)


def cpp_mirror_probe(width, spp, first_sample, lights, light_samples, seg_tmax=SEG_TMAX):
    """rtiow::render_nee of the C++ mirror on golden_test_scene at image_width = width -> PathNEE([H, W, 3]) (the height is the scene's
    aspect ratio's).  For tests of the mirror; RLError carries rlh_last_error."""
    keep, args = _light_args(lights, light_samples, seg_tmax)
    return api.mirror_probe(api.World.golden_test_scene, width, spp, "rlh_nee_probe", (int(first_sample), *args), _outputs, PathNEE, spp, light_samples)


def cpp_mirror_probe_mis(width, spp, first_sample, lights, light_samples, seg_tmax=SEG_TMAX, heuristic="balance"):
    """rtiow::render_nee_mis of the C++ mirror, as cpp_mirror_probe."""
    stem, keep, args = _mis_args(lights, None, light_samples, seg_tmax, heuristic)
    return api.mirror_probe(api.World.golden_test_scene, width, spp, "rlh_nee_mis_probe", (int(first_sample), *args), _outputs, PathNEE, spp, light_samples)


def cpp_mirror_probe_spheres(width, spp, first_sample, lights, sphere_lights, light_samples, seg_tmax=SEG_TMAX, heuristic="balance"):
    """rtiow::render_nee_mis with sphere lights of the C++ mirror on simple_light at image_width = width, max_depth 6 -> PathNEE([H, W, 3])."""
    stem, keep, args = _mis_args(lights, sphere_lights, light_samples, seg_tmax, heuristic)
    return api.mirror_probe(api.World.simple_light, width, spp, "rlh_nee_spheres_probe", (int(first_sample), *args), _outputs, PathNEE, spp, light_samples,
                            max_depth=6)
