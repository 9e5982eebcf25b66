"""The edge-avoiding a-trous filter of include/rl_render.h "Denoising" in numpy, statement for statement: the yardstick the device's bytes
are compared with (tests/test_gpu_denoise.py) and whose own worth tests/test_denoise_abi.py checks.  Every numpy operation on float64
arrays is one correctly rounded binary64 operation, so the bytes are those of the definition.  No np.sum: its pairwise order differs."""
import numpy as np

H5 = (1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0)


def atrous_pass(color, variance, guides, color_sigma2, variance_floor, guide_inv_sigma, step):
    """One pass: color, variance [H, W, 3], guides [H, W, G] or None -> (out_color, out_variance)."""
    H, W = color.shape[:2]
    G = 0 if guides is None else guides.shape[2]
    vsum = (variance[..., 0] + variance[..., 1]) + variance[..., 2]
    ys, xs = np.mgrid[0:H, 0:W]
    sw, ac, av = np.zeros((H, W)), np.zeros((H, W, 3)), np.zeros((H, W, 3))
    with np.errstate(all="ignore"):
        for j in range(-2, 3):
            for i in range(-2, 3):
                qy, qx = ys + j * step, xs + i * step
                inside = (qy >= 0) & (qy < H) & (qx >= 0) & (qx < W)
                qy, qx = np.where(inside, qy, 0), np.where(inside, qx, 0)  # the shifted images; what lies outside is masked below
                cq, vq = color[qy, qx], variance[qy, qx]
                d = color - cq
                d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                D = color_sigma2 * (vsum + vsum[qy, qx]) + variance_floor
                xg = np.zeros((H, W))
                for k in range(G):
                    e = (guides[..., k] - guides[qy, qx, k]) * guide_inv_sigma[k]
                    xg = xg + e * e
                w = ((H5[j + 2] * H5[i + 2]) * D) / ((D + d2) * (1.0 + xg))
                sw = np.where(inside, sw + w, sw)
                ac = np.where(inside[..., None], ac + w[..., None] * cq, ac)
                av = np.where(inside[..., None], av + (w * w)[..., None] * vq, av)
        return ac / sw[..., None], av / (sw * sw)[..., None]


def atrous(color, variance, guides, color_sigma2, variance_floor, guide_inv_sigma, iterations):
    """What rl_denoise_atrous computes: passes with step 1, 2, .., 2^(iterations-1), each on the one before's colour and variance."""
    color, variance = np.array(color, dtype=np.float64), np.array(variance, dtype=np.float64)
    for it in range(iterations):
        color, variance = atrous_pass(color, variance, guides, color_sigma2, variance_floor, guide_inv_sigma, 1 << it)
    return color, variance


def params_of(p):
    """(color_sigma2, variance_floor, guide_inv_sigma) of an api.AtrousParams."""
    return float(p.color_sigma2), float(p.variance_floor), [float(p.guide_inv_sigma[k]) for k in range(p.n_guides)]


def four_region_image(H=23, W=37, spp=4, seed=11, n_guides=0):
    """A synthetic render: four flat regions (quadrants split off-centre), `spp` noisy samples per pixel whose standard deviation differs
    by region (one region noise-free: its variances are exactly 0) -> (truth, mean, variance of the mean, guides).  guides: n_guides
    channels, channel 0 the region index, the others smooth ramps and noise."""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:H, 0:W]
    region = (ys >= (2 * H) // 5).astype(np.int64) * 2 + (xs >= (3 * W) // 5)
    palette = np.array([[0.9, 0.2, 0.1], [0.1, 0.6, 0.8], [0.3, 0.3, 0.3], [1.5, 1.2, 0.2]])
    sigma = np.array([0.3, 0.1, 0.0, 0.5])[region]
    truth = palette[region]
    samples = truth[None] + rng.standard_normal((spp, H, W, 3)) * sigma[None, ..., None]
    mean = samples[0].copy()
    for s in range(1, spp):
        mean = mean + samples[s]
    mean = mean / spp
    sq = np.zeros_like(mean)
    for s in range(spp):
        sq = sq + (samples[s] - mean) * (samples[s] - mean)
    variance = sq / (spp - 1) / spp
    guides = None
    if n_guides:
        chans = [region.astype(np.float64), xs / W, ys / H] + [rng.standard_normal((H, W)) for _ in range(max(0, n_guides - 3))]
        guides = np.ascontiguousarray(np.stack(chans[:n_guides], axis=-1))
    return truth, np.ascontiguousarray(mean), np.ascontiguousarray(variance), guides


def mse(a, b):
    return float(np.mean((a - b) ** 2))
