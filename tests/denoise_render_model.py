"""denoise_render on the device (include/rl_render.h "Denoising": rl_denoise_prepare_device, rl_denoise_finish_device, rl_denoise_render*) in
numpy, statement for statement: the yardstick the device's bytes are compared with (tests/test_gpu_denoise_render.py), itself pinned to the
host path api.denoise_render by tests/test_denoise_render_abi.py.  Every line is one correctly rounded binary64 operation on float64 arrays;
nothing is fused, sums run left to right, np.sum is not used, and uint32 inputs convert to float64 exactly.  sqrt is the one operation
beyond + - * /; IEEE 754 wants it correctly rounded, and np.sqrt is.

No input is scanned: a pixel whose count is 0 or 1 gets the non-finite values the arithmetic gives (x / 0, 0 / 0), and the passes spread
them to the pixels whose 25-tap footprints touch it and to no other (atrous_model.py, the header's rule for non-finite inputs)."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import atrous_model

GUIDE_ALBEDO, GUIDE_NORMAL, GUIDE_DEPTH, GUIDE_COVERAGE = 1, 2, 4, 8
GUIDE_ALL = 15


@dataclass
class Inputs:
    """rl_denoise_inputs with arrays in place of pointers."""
    sums: np.ndarray                         # [H, W, 3] f64
    sq: np.ndarray                           # [H, W, 3] f64
    albedo_sum: np.ndarray                   # [H, W, 3] f64
    feature_samples: int
    counts: Optional[np.ndarray] = None      # [H, W] uint32, or None: every pixel took `samples`
    samples: int = 0
    normal_sum: Optional[np.ndarray] = None  # [H, W, 3] f64
    depth_sum: Optional[np.ndarray] = None   # [H, W] f64
    hit_count: Optional[np.ndarray] = None   # [H, W] uint32
    want: int = GUIDE_ALL


def n_guides(want):
    return 3 * bool(want & GUIDE_ALBEDO) + 3 * bool(want & GUIDE_NORMAL) + bool(want & GUIDE_DEPTH) + bool(want & GUIDE_COVERAGE)


def _divisor(albedo_sum, feature_samples):
    """(alb, a): the albedo mean, and what the colour is divided by: the albedo where it is > 0, else 1 (a NaN albedo: 1)."""
    alb = albedo_sum * (1.0 / feature_samples)
    return alb, np.where(alb > 0.0, alb, 1.0)


def prepare(inp: Inputs):
    """-> (color [H, W, 3], variance [H, W, 3], guides [H, W, G])."""
    sums, sq = np.asarray(inp.sums, dtype=np.float64), np.asarray(inp.sq, dtype=np.float64)
    with np.errstate(all="ignore"):
        if inp.counts is not None:
            n = np.asarray(inp.counts, dtype=np.uint32).astype(np.float64)[..., None]
            mean = sums / n
        else:
            n = np.float64(inp.samples)
            mean = sums * (1.0 / inp.samples)
        raw = (((sq - (sums * sums) / n) / (n - 1.0)) / n)
        var = np.where(raw < 0.0, 0.0, raw)  # not np.fmax: a NaN stays NaN
        alb, a = _divisor(np.asarray(inp.albedo_sum, dtype=np.float64), inp.feature_samples)
        color, variance = mean / a, var / (a * a)
        groups = []
        if inp.want & GUIDE_ALBEDO:
            groups.append(alb)
        if inp.want & GUIDE_NORMAL:
            ns = np.asarray(inp.normal_sum, dtype=np.float64)
            l = np.sqrt((ns[..., 0] * ns[..., 0] + ns[..., 1] * ns[..., 1]) + ns[..., 2] * ns[..., 2])[..., None]
            groups.append(np.where(l != 0.0, ns / l, 0.0))
        if inp.want & (GUIDE_DEPTH | GUIDE_COVERAGE):
            k = np.asarray(inp.hit_count, dtype=np.uint32)
            if inp.want & GUIDE_DEPTH:
                groups.append((np.asarray(inp.depth_sum, dtype=np.float64) / np.maximum(k, 1).astype(np.float64))[..., None])
            if inp.want & GUIDE_COVERAGE:
                groups.append((k.astype(np.float64) / np.float64(inp.feature_samples))[..., None])
    guides = np.concatenate(groups, axis=-1) if groups else np.zeros(sums.shape[:2] + (0,))
    return np.ascontiguousarray(color), np.ascontiguousarray(variance), np.ascontiguousarray(guides, dtype=np.float64)


def finish(color_f, variance_f, albedo_sum, feature_samples):
    """-> (out_color, out_variance): the filtered images multiplied back by a and a * a; a is recomputed from albedo_sum."""
    _, a = _divisor(np.asarray(albedo_sum, dtype=np.float64), feature_samples)
    with np.errstate(all="ignore"):
        return color_f * a, variance_f * (a * a)


def raw_variance(inp: Inputs):
    """raw of the definition, before the clip: the tests ask it where a pixel is clipped."""
    sums, sq = inp.sums, inp.sq
    n = np.float64(inp.samples) if inp.counts is None else inp.counts.astype(np.float64)[..., None]
    with np.errstate(all="ignore"):
        return (((sq - (sums * sums) / n) / (n - 1.0)) / n)


HAND_COUNTS = np.array([[2, 3, 4, 5], [6, 7, 8, 9], [3, 2, 9, 5]], dtype=np.uint32)  # the adaptive variant's samples per pixel: 2 .. 9
HAND_SAMPLES, HAND_FEATURE_SAMPLES = 3, 4                                            # the moments variant's; the feature render's
CONSTANT_PIXEL = (0, 1)


def _accumulate(samples):
    """sums and second moments of one pixel's samples [n, 3], as the renders accumulate them: from 0.0, in sample order, the square rounded first."""
    s, q = np.zeros(3), np.zeros(3)
    for c in samples:
        s = s + c
        q = q + c * c
    return s, q


def hand_made(with_counts, want=GUIDE_ALL) -> Inputs:
    """A 3 x 4 frame of sums accumulated from seeded samples, holding a pixel of every kind the definition treats on its own: (0, 0) has an
    albedo of exactly 0 in one channel, (0, 2) an albedo above 1, (1, 2) was never hit (hit_count 0, normal_sum and depth_sum zero), (2, 0)
    has a normal_sum of zero though it was hit, and (0, 1) holds n equal samples of a colour chosen, per channel, so that round-off takes raw
    below 0 (the clipped pixel).  with_counts: an adaptive render with HAND_COUNTS; else a moments render of HAND_SAMPLES samples."""
    rng = np.random.default_rng(17)
    H, W = HAND_COUNTS.shape
    counts = HAND_COUNTS if with_counts else np.full((H, W), HAND_SAMPLES, dtype=np.uint32)
    sums, sq = np.zeros((H, W, 3)), np.zeros((H, W, 3))
    for y in range(H):
        for x in range(W):
            sums[y, x], sq[y, x] = _accumulate(rng.uniform(0.0, 2.0, (int(counts[y, x]), 3)))
    n = int(counts[CONSTANT_PIXEL])
    for colour in (0.1, 0.2, 0.3, 0.6, 0.7, 0.9, 1.1, 1.3, 1.7, 1.9):  # the first whose n squares sum to less than sum^2 / n in binary64
        s, q = _accumulate(np.full((n, 3), colour))
        if ((((q - (s * s) / n) / (n - 1.0)) / n) < 0.0).all():
            break
    sums[CONSTANT_PIXEL], sq[CONSTANT_PIXEL] = s, q  # (the tests assert that one was found)
    albedo_sum = rng.uniform(0.4, 3.6, (H, W, 3))
    albedo_sum[0, 0, 1] = 0.0
    albedo_sum[0, 2] = [6.0, 4.5, 8.0]
    normal_sum = rng.standard_normal((H, W, 3))
    depth_sum = rng.uniform(1.0, 9.0, (H, W))
    hit_count = np.array([[4, 3, 1, 2], [2, 4, 0, 4], [1, 3, 4, 2]], dtype=np.uint32)
    normal_sum[1, 2], depth_sum[1, 2] = 0.0, 0.0
    normal_sum[2, 0] = 0.0
    return Inputs(sums=sums, sq=sq, albedo_sum=albedo_sum, feature_samples=HAND_FEATURE_SAMPLES, counts=counts if with_counts else None,
                  samples=0 if with_counts else HAND_SAMPLES, normal_sum=normal_sum, depth_sum=depth_sum, hit_count=hit_count, want=want)


def tiled(inp: Inputs, H, W) -> Inputs:
    """`inp` repeated over an H x W frame."""
    def tile(a):
        if a is None:
            return None
        reps = (-(-H // a.shape[0]), -(-W // a.shape[1])) + (1,) * (a.ndim - 2)
        return np.ascontiguousarray(np.tile(a, reps)[:H, :W])
    return Inputs(sums=tile(inp.sums), sq=tile(inp.sq), albedo_sum=tile(inp.albedo_sum), feature_samples=inp.feature_samples, counts=tile(inp.counts),
                  samples=inp.samples, normal_sum=tile(inp.normal_sum), depth_sum=tile(inp.depth_sum), hit_count=tile(inp.hit_count), want=inp.want)


def with_short_pixels(inp: Inputs, one, zero) -> Inputs:
    """A copy of an adaptive `inp` in which pixel `one` (y, x) took one sample and pixel `zero` none, with the sums such renders leave: one
    colour and its square (raw = 0 / 0), and zeros (mean = 0 / 0)."""
    sums, sq, counts = inp.sums.copy(), inp.sq.copy(), inp.counts.copy()
    colour = np.array([0.3, 0.7, 1.1])
    sums[one], sq[one], counts[one] = colour, colour * colour, 1
    sums[zero], sq[zero], counts[zero] = 0.0, 0.0, 0
    return Inputs(sums=sums, sq=sq, albedo_sum=inp.albedo_sum, feature_samples=inp.feature_samples, counts=counts, samples=0, normal_sum=inp.normal_sum,
                  depth_sum=inp.depth_sum, hit_count=inp.hit_count, want=inp.want)


def render(inp: Inputs, params, iterations):
    """What rl_denoise_render* computes: finish(atrous(prepare(...))); params = (color_sigma2, variance_floor, guide_inv_sigma)."""
    color, variance, guides = prepare(inp)
    color, variance = atrous_model.atrous(color, variance, guides if guides.shape[2] else None, *params, iterations)
    return finish(color, variance, inp.albedo_sum, inp.feature_samples)
