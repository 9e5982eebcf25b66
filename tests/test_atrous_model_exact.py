"""CPU tier: the yardstick against exact arithmetic.  tests/atrous_model.py restates the header's a-trous pass operation by operation, so
it pins the rounding order but is not an independent statement of WHAT is computed.  Here the pass (include/rl_render.h "Denoising") is
written a second time, as loops over pixels and taps in exact rational arithmetic (fractions.Fraction), sharing no code with the model,
and the model's binary64 outputs are held to the error its roundings can make.  The device equals the model in bytes
(tests/test_gpu_denoise.py), so this ties the device to the exact operation.

The bound.  u = 2^-53.  Inputs and parameters are binary64 numbers, hence exact.  Every colour, variance and guide is >= 0, so every
quantity below except the differences d and e is a sum or product of non-negative terms; d and e are differences of EXACT inputs, so they
carry one rounding however much cancels.  Count for each value the factors (1 + delta), |delta| <= u, that separate it from the exact
value (a product or quotient carries the sum of its operands' counts plus one; a sum of non-negative terms the larger count plus one;
x + 0.0 and x * 1.0 are exact).  Nothing underflows on the images used (a zero comes only from exact zeros).  Then for 25 taps and G >= 1:
    vsum 2;  vsum(p) + vsum(q) 3;  color_sigma2 * that 4;  D 5
    d 1;  d*d 3;  d0*d0 + d1*d1 4;  d2 5
    e 2;  e*e 5;  xg = 0 + e*e 5, then one more per further guide: G + 4;  1.0 + xg: G + 5
    (h*h) is exact;  (h*h) * D 6;  D + d2 6;  (D + d2) * (1.0 + xg): 6 + (G + 5) + 1 = G + 12;  w: 6 + (G + 12) + 1 = G + 19
    sw: the first tap is added to +0.0, 24 additions follow: G + 43
    w * color_q: G + 20;  ac: G + 44;  out_color = ac / sw: (G + 44) + (G + 43) + 1 = 2 G + 88
    w*w: 2 G + 39;  (w*w) * var_q: 2 G + 40;  av: 2 G + 64;  sw*sw: 2 G + 87;  out_variance: (2 G + 64) + (2 G + 87) + 1 = 4 G + 152
With G = 8: w 27, sw 51, colour 104, variance 184.  With G = 0, xg = 0 and 1.0 + xg = 1.0 exactly and the product with it is exact:
w 13, sw 37, colour 76, variance 128 (the formulas above with G = -6).  A quotient of (1 + delta)^a by (1 + delta)^b lies within
gamma(a + b) = (a + b) u / (1 - (a + b) u) of 1, which is the bound used: k u (1 + 2.1e-14) at most.  Fewer taps (borders, step 5) only
shorten the sums, so the 25-tap count holds for every pixel."""
from fractions import Fraction

import numpy as np
import pytest

import atrous_model as M

H, W = 7, 6
U = Fraction(1, 2 ** 53)
ROUNDINGS = {0: (76, 128), 8: (104, 184)}  # G: (out_color, out_variance), derived in the docstring
KERNEL = (Fraction(1, 16), Fraction(1, 4), Fraction(3, 8), Fraction(1, 4), Fraction(1, 16))


def _images(G):
    """Non-negative colours, variances and guides; rows 2 - 4 of columns 0 - 2 have exactly zero variance; two pixels there share a colour
    (d = 0 exactly: the case D = floor, d2 = 0)."""
    rng = np.random.default_rng(29 + G)
    color = rng.uniform(0.05, 2.0, (H, W, 3))
    variance = rng.uniform(1e-4, 0.2, (H, W, 3))
    variance[2:5, 0:3] = 0.0
    color[3, 1] = color[3, 2]
    guides = rng.uniform(0.0, 3.0, (H, W, G)) if G else None
    inv = [float(v) for v in rng.uniform(0.25, 4.0, G)]
    return color, variance, guides, inv


def _exact_pass(color, variance, guides, color_sigma2, variance_floor, inv, step):
    """The definition in exact rationals -> (out_color, out_variance) as nested lists [H][W][3] of Fraction."""
    G = 0 if guides is None else guides.shape[2]
    F = Fraction
    sigma2, floor = F(color_sigma2), F(variance_floor)
    out_c = [[None] * W for _ in range(H)]
    out_v = [[None] * W for _ in range(H)]
    for y in range(H):
        for x in range(W):
            weight_sum, colour_sum, variance_sum = F(0), [F(0)] * 3, [F(0)] * 3
            var_p = sum(F(float(variance[y, x, c])) for c in range(3))
            for j in range(5):
                ty = y + (j - 2) * step
                if ty < 0 or ty >= H:
                    continue
                for i in range(5):
                    tx = x + (i - 2) * step
                    if tx < 0 or tx >= W:
                        continue
                    dist = sum((F(float(color[y, x, c])) - F(float(color[ty, tx, c]))) ** 2 for c in range(3))
                    var_q = sum(F(float(variance[ty, tx, c])) for c in range(3))
                    scale = sigma2 * (var_p + var_q) + floor
                    guide_dist = sum(((F(float(guides[y, x, k])) - F(float(guides[ty, tx, k]))) * F(inv[k])) ** 2 for k in range(G))
                    weight = KERNEL[j] * KERNEL[i] * scale / ((scale + dist) * (1 + guide_dist))
                    weight_sum += weight
                    colour_sum = [colour_sum[c] + weight * F(float(color[ty, tx, c])) for c in range(3)]
                    variance_sum = [variance_sum[c] + weight * weight * F(float(variance[ty, tx, c])) for c in range(3)]
            out_c[y][x] = [s / weight_sum for s in colour_sum]
            out_v[y][x] = [s / (weight_sum * weight_sum) for s in variance_sum]
    return out_c, out_v


def _worst_ratio(got, exact, k):
    """max over the image of |got - exact| / (gamma(k) * exact); an exact zero must be a computed zero."""
    gamma = k * U / (1 - k * U)
    worst = Fraction(0)
    for y in range(H):
        for x in range(W):
            for c in range(3):
                g, e = Fraction(float(got[y, x, c])), exact[y][x][c]
                assert e >= 0
                if e == 0:
                    assert g == 0, (y, x, c)
                else:
                    worst = max(worst, abs(g - e) / (gamma * e))
    return float(worst)


@pytest.mark.parametrize("G", [0, 8])
@pytest.mark.parametrize("step", [1, 2, 5])
def test_model_is_the_exact_pass_within_its_roundings(step, G):
    color, variance, guides, inv = _images(G)
    color_sigma2, floor = 4.0, 1e-8
    got_c, got_v = M.atrous_pass(color, variance, guides, color_sigma2, floor, inv, step)
    want_c, want_v = _exact_pass(color, variance, guides, color_sigma2, floor, inv, step)
    k_c, k_v = ROUNDINGS[G]
    r_c, r_v = _worst_ratio(got_c, want_c, k_c), _worst_ratio(got_v, want_v, k_v)
    print(f"step {step} G {G}: worst error / bound: colour {r_c:.4f} (= {r_c * k_c:.2f} u of {k_c}), variance {r_v:.4f} (= {r_v * k_v:.2f} u of {k_v})")
    assert r_c <= 1.0 and r_v <= 1.0
    assert r_c > 0.0  # the comparison is live: binary64 does differ from the exact value somewhere
