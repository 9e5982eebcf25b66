"""CPU tier: the procedural textures against tests/procedural_model.py, which is written from the reference's text and shares nothing
with the oracle or the kernels.

  a. Perlin by hand: hand-made tables whose answers are dyadic sums worked out in the comments; the model is held to them first, then
     the oracle, both with ==.
  b. Oracle against model within the model's forward bound, on tables with asymmetric permutations and on points at every edge of the
     cell index (tests/procedural_model.py perlin_points).
  c. The host mirror of Perlin::new: each permutation is a single 256-cycle (permute draws gen_range(0..i), Sattolo's variant), the
     vectors are unit to a derived bound, the tables are a function of the seed.
  d. The reference's pattern unit tables (stripe.rs, ring.rs, gradient.rs, checker3d.rs, pattern/mod.rs, transformed.rs, material.rs),
     through the oracle's color_at on ambient-only worlds; the model is held to the same rows first.
"""
from fractions import Fraction

import numpy as np
import pytest

import procedural_model as P
from test_rtc_solids_oracle import S, T, WorldBuilder

NAN = float("nan")


# ----------------------------------------------------------------------------- a. Perlin by hand
X0 = {"vectors": {0: (1, 0, 0)}}
SHIFT = lambda by: (np.arange(256) + by) % 256  # noqa: E731

# Identity permutations: a corner's vector is randvec[(i + di) ^ (j + dj) ^ (k + dk)].  H(t) = t t (3 - 2t): H(1/4) = 5/32 = 0.15625,
# H(1/2) = 1/2, H(3/4) = 27/32 = 0.84375.  A corner's blend is the product over the axes of H (d = 1) or 1 - H (d = 0), its dot is
# vector . (u - di, v - dj, w - dk).  Every number below is a dyadic fraction of at most 20 bits: binary64 gets each exactly.
NOISE_BY_HAND = [
    # randvec[0] = (1, 0, 0), p = (1/4, 1/2, 1/2) in cell (0, 0, 0): the corners with di ^ dj ^ dk = 0 are 000, 011, 101, 110;
    # blends (27/32)(1/2)(1/2) for di = 0 and (5/32)(1/2)(1/2) for di = 1, dots 1/4 and -3/4:
    # 2 * 0.84375 * 0.25 * 0.25 - 2 * 0.15625 * 0.25 * 0.75 = 0.10546875 - 0.05859375
    (X0, (0.25, 0.5, 0.5), 0.046875),
    # a negative cell: floor(-3/4) = -1, u = 1/4 (a cast that truncates gives cell 0 and u = -3/4).  -1 & 255 = 255, so di = 0 reads
    # perm_x[255] and di = 1 reads perm_x[0]: with randvec[0] alone the corners are 100 and 111, 2 * (5/32)(1/4) * (-3/4)
    (X0, (-0.75, 0.5, 0.5), -0.05859375),
    # ... and with randvec[255] alone they are 000 and 011: 2 * (27/32)(1/4) * (1/4)
    ({"vectors": {255: (1, 0, 0)}}, (-0.75, 0.5, 0.5), 0.10546875),
    # the table wrap: cell 255, di = 1 reads (255 + 1) & 255 = 0: the same two answers
    (X0, (255.25, 0.5, 0.5), -0.05859375),
    ({"vectors": {255: (1, 0, 0)}}, (255.25, 0.5, 0.5), 0.10546875),
    # three different fractions, p = (1/4, 1/2, 3/4): blends 000: (27/32)(1/2)(5/32), 011: (27/32)(1/2)(27/32), 101: (5/32)(1/2)(27/32),
    # 110: (5/32)(1/2)(5/32) = 0.06591796875, 0.35595703125, 0.06591796875, 0.01220703125
    # vector along x: dots 1/4, 1/4, -3/4, -3/4: 0.0164794921875 + 0.0889892578125 - 0.0494384765625 - 0.0091552734375
    (X0, (0.25, 0.5, 0.75), 0.046875),
    # along y: dots v - dj = 1/2, -1/2, 1/2, -1/2: 0.032958984375 - 0.177978515625 + 0.032958984375 - 0.006103515625
    ({"vectors": {0: (0, 1, 0)}}, (0.25, 0.5, 0.75), -0.1181640625),
    # along z: dots w - dk = 3/4, -1/4, -1/4, 3/4: 0.0494384765625 - 0.0889892578125 - 0.0164794921875 + 0.0091552734375
    ({"vectors": {0: (0, 0, 1)}}, (0.25, 0.5, 0.75), -0.046875),
    # perm_z[i] = i + 1: the index is di ^ dj ^ (dk + 1), zero only for dk = 0 and di ^ dj = 1: corners 010 and 100,
    # (27/32)(1/2)(5/32)(1/4) + (5/32)(1/2)(5/32)(-3/4) = 0.0164794921875 - 0.0091552734375
    ({"vectors": {0: (1, 0, 0)}, "perms": [SHIFT(0), SHIFT(0), SHIFT(1)]}, (0.25, 0.5, 0.75), 0.00732421875),
    # perm_y[j] = j + 1 instead: corners 001 and 100, (27/32)(1/2)(27/32)(1/4) + (5/32)(1/2)(5/32)(-3/4)
    ({"vectors": {0: (1, 0, 0)}, "perms": [SHIFT(0), SHIFT(1), SHIFT(0)]}, (0.25, 0.5, 0.75), 0.079833984375),
]
# turb: |sum_k 2^-k noise(2^k p)|.  2 * (1/4, 1/2, 1/2) = (1/2, 1, 1): cell (0, 1, 1) with v = w = 0, so only dj = dk = 0 has a blend:
# corner 000 reads randvec[0 ^ 1 ^ 1 = 0] with blend 1/2 and dot 1/2 (0.25), corner 100 reads randvec[1] = 0.  4p and beyond are lattice
# points of cells whose index 0 corner has a zero blend or a zero dot: 0.  So depth 1: 0.046875; depth 2 and 7: 0.046875 + 0.25 / 2.
# Scaling the weight alone would give 0.046875 * 1.5.  From (1/4, 1/2, 3/4): (1/2, 1, 3/2) is cell (0, 1, 1) with w = 1/2: corner 000
# again, blend (1/2)(1)(1/2), dot 1/2: 0.125, and 0.046875 + 0.0625.  A vector of (-1, 0, 0) makes the sum negative: the same answers.
TURB_BY_HAND = [(X0, (0.25, 0.5, 0.5), 1, 0.046875), (X0, (0.25, 0.5, 0.5), 2, 0.171875), (X0, (0.25, 0.5, 0.5), 7, 0.171875),
                (X0, (0.25, 0.5, 0.75), 2, 0.109375), ({"vectors": {0: (-1, 0, 0)}}, (0.25, 0.5, 0.5), 2, 0.171875),
                ({"vectors": {0: (-1, 0, 0)}}, (0.25, 0.5, 0.75), 1, 0.046875)]

# turb(p, 7), which is what Noise::value reads.  For these dyadic points 4p and beyond are lattice points: turb7 = |noise(p) + noise(2p) / 2|.
# 2 * (-3/4, 1/2, 1/2) = (-3/2, 1, 1) is cell (-2, 1, 1) with u = 1/2, v = w = 0: only 000 and 100 have a blend, 1/2 each; they read
# randvec[254 ^ 1 ^ 1 = 254] and randvec[255 ^ 1 ^ 1 = 255] with dots 1/2 and -1/2: 0 with randvec[0] alone, -0.25 with randvec[255] alone;
# (510.5, 1, 1) is cell 510 & 255 = 254: the same.  2 * (1/4, 1/2, 3/4) = (1/2, 1, 3/2), cell (0, 1, 1), u = w = 1/2, v = 0: corners 000, 001,
# 100, 101 read randvec[0 ^ 1 ^ 1 = 0], [0 ^ 1 ^ 2 = 3], [1], [2]; 000 has blend 1/4 and dot (1/2, 0, 1/2) . vector: 0.125, 0, 0.125 for x, y, z.
# (9/4, 1/2, 1/2) and its doublings up to (144, 32, 32) never hash to index 0: turb is 0 and Noise::value 0.5 exactly; a lattice point likewise.
TURB7_BY_HAND = [(X0, (0.25, 0.5, 0.5), 0.171875), (X0, (-0.75, 0.5, 0.5), 0.05859375), ({"vectors": {255: (1, 0, 0)}}, (-0.75, 0.5, 0.5), 0.01953125),
                 (X0, (255.25, 0.5, 0.5), 0.05859375), ({"vectors": {255: (1, 0, 0)}}, (255.25, 0.5, 0.5), 0.01953125),
                 (X0, (0.25, 0.5, 0.75), 0.109375), ({"vectors": {0: (0, 1, 0)}}, (0.25, 0.5, 0.75), 0.1181640625),
                 ({"vectors": {0: (0, 0, 1)}}, (0.25, 0.5, 0.75), 0.015625), (X0, (2.25, 0.5, 0.5), 0.0), (X0, (3.0, -2.0, 7.0), 0.0),
                 # perm_z shifted by one: at (1/2, 1, 3/2) (v = 0: dj = 0 only) the index is di ^ 1 ^ (2 + dk), never 0: noise(p) alone.
                 # perm_y shifted by one: di ^ 2 ^ (1 + dk) is 0 for corner 001, blend (1/2)(1)(1/2), dot u = 1/2: 0.125, and
                 # 0.079833984375 + 0.0625
                 ({"vectors": {0: (1, 0, 0)}, "perms": [SHIFT(0), SHIFT(0), SHIFT(1)]}, (0.25, 0.5, 0.75), 0.00732421875),
                 ({"vectors": {0: (1, 0, 0)}, "perms": [SHIFT(0), SHIFT(1), SHIFT(0)]}, (0.25, 0.5, 0.75), 0.142333984375)]


def test_the_model_gives_the_by_hand_perlin_answers():
    for rows, p, want in NOISE_BY_HAND:
        assert P.noise(P.lattice_table(rows)[0], p)[0] == want, (rows["vectors"], p)
    for rows, p, depth, want in TURB_BY_HAND:
        assert P.turb(P.lattice_table(rows)[0], p, depth)[0] == want, (rows["vectors"], p, depth)
    for rows, p, want in TURB7_BY_HAND:
        assert P.turb(P.lattice_table(rows)[0], p, 7)[0] == want, (rows["vectors"], p)


def test_the_oracle_gives_the_by_hand_perlin_answers(oracle):
    for rows, p, want in NOISE_BY_HAND:
        assert oracle.perlin_noise(P.lattice_table(rows), p) == want, (rows["vectors"], p)
    for rows, p, depth, want in TURB_BY_HAND:
        assert oracle.perlin_turb(P.lattice_table(rows), p, depth) == want, (rows["vectors"], p, depth)
    for rows, p, want in TURB7_BY_HAND:
        assert oracle.perlin_turb(P.lattice_table(rows), p, 7) == want, (rows["vectors"], p)


def test_rust_casts_and_integer_arithmetic_by_hand():
    below = float(np.nextafter(2.0 ** 63, 0.0))
    assert below == 2.0 ** 63 - 1024.0
    for x, want in [(0.9, 0), (-0.9, 0), (-1.5, -1), (2147483646.5, 2147483646), (2147483647.0, 2 ** 31 - 1), (2147483648.0, 2 ** 31 - 1),
                    (1e300, 2 ** 31 - 1), (float("inf"), 2 ** 31 - 1), (-2147483648.0, -2 ** 31), (-2147483649.0, -2 ** 31), (-float("inf"), -2 ** 31),
                    (NAN, 0)]:
        assert P.rust_as_i32(x) == want, x
    for x, want in [(below, 2 ** 63 - 1024), (2.0 ** 63, 2 ** 63 - 1), (1e19, 2 ** 63 - 1), (float("inf"), 2 ** 63 - 1), (-2.0 ** 63, -2 ** 63),
                    (-1e19, -2 ** 63), (-float("inf"), -2 ** 63), (NAN, 0), (-0.5, 0), (1e15, 10 ** 15)]:
        assert P.rust_as_i64(x) == want, x
    assert P.wrap_i32(2 ** 31 - 1 + 1) == -2 ** 31 and P.wrap_i32(-2 ** 31) & 255 == 0 and (2 ** 31 - 1) & 255 == 255
    assert P.wrap_i64(2 ** 63 - 1 + 1) == -2 ** 63 and P.wrap_i64(2 * (2 ** 63 - 1)) == -2
    assert [P.rust_rem2(n) for n in (-3, -2, -1, 0, 1, 2 ** 63 - 1, -2 ** 63)] == [-1, 0, -1, 0, 1, 1, 0]


# ----------------------------------------------------------------------------- b. oracle against model
def test_the_oracle_meets_the_model_within_its_bound(oracle):
    pts, bad = P.perlin_points()
    worst = {"noise": 0.0, "turb": 0.0}
    for tab in P.random_tables():
        rec = tab[0]
        for q in pts:
            for name, want, got in (("noise", P.noise(rec, q), oracle.perlin_noise(tab, q)), ("turb", P.turb(rec, q, 7), oracle.perlin_turb(tab, q, 7))):
                assert abs(got - want[0]) <= want[1], (name, tuple(q), got, want)
                if want[1] > 1e-300:  # nothing but underflow terms at lattice points: every term is an exact zero
                    worst[name] = max(worst[name], abs(got - want[0]) / want[1])
        for q in bad:
            assert np.isnan(oracle.perlin_noise(tab, q)) and np.isnan(oracle.perlin_turb(tab, q, 7)), tuple(q)
            assert np.isnan(P.noise(rec, q)[0]) and np.isnan(P.turb(rec, q, 7)[0]) and np.isnan(P.noise_value(rec, 4.0, q)[0])
    print(f"points {len(pts)} x 2 tables; worst observed / bound: noise {worst['noise']:.3f} turb {worst['turb']:.3f}")
    assert len(pts) >= 200


def test_every_edge_of_the_cell_index_is_among_the_points():
    pts, _ = P.perlin_points()
    cells = {P.rust_as_i32(P.ffloor(c)) for q in pts for c in q}
    assert {P.I32_MAX, P.I32_MIN, -1, 0, 255, 256, -256, 2 ** 31 - 2, -2 ** 31 + 1} <= cells
    seventh = {P.rust_as_i32(P.ffloor(c * 64.0)) for q in pts for c in q}
    assert {2 ** 31 - 17, P.I32_MAX, P.I32_MIN, -2 ** 31 + 17} <= seventh  # 64 (2^25 -+ 0.265625) = 2^31 -+ 17
    assert any(c - P.ffloor(c) == 1.0 for q in pts for c in q)  # the one inexact u


# ----------------------------------------------------------------------------- c. the host mirror of Perlin::new
SEEDS = [0, 1, 2, 3, 42, 2 ** 32 - 1, 2 ** 63, 2 ** 64 - 1]


def _host_tables(rl, seed):
    world = rl.World.build(lambda b: b.list([b.sphere((0.0, 0.0, 0.0), 1.0, b.lambertian(b.noise(4.0, seed)))]))
    tabs = world.perlins()
    assert tabs.shape == (1,)
    return tabs


def test_host_perlin_tables_are_single_cycles_of_unit_vectors(rl):
    """permute (perlin.rs:82-89) swaps p[i] with p[gen_range(0..i)], the upper end excluded, so an element never stays: started from
    the identity that is Sattolo's algorithm and the result is one cycle through all 256 indices.  A uniformly random permutation (a
    Fisher-Yates shuffle, gen_range(0..=i)) is one with probability 1/256 per table.

    Unit vectors: with s = x1^2 + x2^2 and f = 2 sqrt(1 - s) the vector is (x1 f, x2 f, 1 - 2s) and its squared length 4s(1 - s) +
    (1 - 2s)^2 = 1 exactly.  In binary64 s' = s (1 + 2u) at most (two squares and a sum), which moves the exact length by 4 (s - s')(1 - s')
    <= 8u s(1 - s) <= 2u; f carries 1 - s' (u), the square root (u / 2 of it, u of its own) and each product one more: (x1 f)^2 + (x2 f)^2
    moves by 2 (3/2 + 1) u * 4s(1 - s) <= 5u; 1 - 2s' rounds once: 2u (1 - 2s)^2 <= 2u.  In all |v|^2 - 1 <= 9u, measured exactly."""
    seen = set()
    worst = Fraction(0)
    for seed in SEEDS:
        tab = _host_tables(rl, seed)[0]
        for name in ("perm_x", "perm_y", "perm_z"):
            perm = [int(v) for v in tab[name]]
            assert sorted(perm) == list(range(256)), (seed, name)
            at, steps = perm[0], 1
            while at != 0:
                at, steps = perm[at], steps + 1
            assert steps == 256, (seed, name, steps)
        for vec in tab["randvec"]:
            worst = max(worst, abs(sum(Fraction(float(c)) ** 2 for c in vec) - 1))
        assert _host_tables(rl, seed).tobytes() == tab.tobytes(), seed
        seen.add(tab.tobytes())
    print(f"seeds {len(SEEDS)}; worst | |randvec|^2 - 1 | = {float(worst) / P.U:.3f} u (bound 9 u)")
    assert worst <= 9 * Fraction(P.U)
    assert len(seen) == len(SEEDS)


# ----------------------------------------------------------------------------- d. the reference's pattern tables
WHITE, BLACK = (1.0, 1.0, 1.0), (0.0, 0.0, 0.0)
LIGHT = [((0.0, 10.0, 0.0), WHITE)]
IDENT = np.eye(4)


def ambient_only(b, pattern):
    """material.rs:276-287: ambient 1, diffuse and specular 0; with a white light lighting() is the surface colour exactly"""
    return b.material(pattern=pattern, ambient=1.0, diffuse=0.0, specular=0.0)


def axis_probe(axis, divide=8.0):
    """The reference's MockPattern (pattern/mod.rs:23-35) returns the pattern point as a colour; nothing here does.  A gradient from black
    to white returns frac(x) of its point in every channel, so a gradient whose inverse is T(1/2) S(1 / divide) P_axis, P_axis moving the
    wanted coordinate into x, reads coordinate / divide + 1/2, exactly for dyadic coordinates inside +-divide / 2.  -> the transform to
    compose after the pattern transform under test (its inverse is applied first, then this one's)."""
    perm = np.zeros((4, 4))
    perm[0, axis], perm[1, (axis + 1) % 3], perm[2, (axis + 2) % 3], perm[3, 3] = 1, 1, 1, 1
    inverse = T(0.5, 0.5, 0.5) @ S(1 / divide, 1 / divide, 1 / divide) @ perm
    return np.linalg.inv(inverse), inverse


def _set_inverse(b, index, inverse):
    b.pats[index - 1]["inverse"] = np.asarray(inverse, dtype=np.float64).reshape(16)


def plane_world(rl, kind, a, b_colour, pattern_inverse):
    """an xz plane with the pattern; a ray from (x, 1, z) straight down meets it at t = 1 at the object point (x, 0, z)"""
    b = WorldBuilder(rl.api)
    pat = b.pattern(kind, a, b_colour, IDENT)
    _set_inverse(b, pat, pattern_inverse)
    return b.world(rl, [b.shape(rl.api.O_PLANE, material=ambient_only(b, pat))], lights=LIGHT)


# at_local(point) of a default pattern (a white, b black) -> colour.  A point off the plane y = 0 is reached through a pattern
# transform translation(0, -y, 0), whose inverse moves the plane's (x, 0, z) to (x, y, z).
AT_LOCAL = {
    "PAT_STRIPE": [((0, 0, 0), WHITE), ((0, 1, 0), WHITE), ((0, 2, 0), WHITE),  # stripe.rs:46-62 constant in y
                   ((0, 0, 1), WHITE), ((0, 0, 2), WHITE),  # :64-80 constant in z
                   ((0.9, 0, 0), WHITE), ((1, 0, 0), BLACK), ((-0.1, 0, 0), BLACK), ((-1, 0, 0), BLACK), ((-1.1, 0, 0), WHITE)],  # :82-110
    "PAT_RING": [((0, 0, 0), WHITE), ((1, 0, 0), BLACK), ((0, 0, 1), BLACK), ((0.708, 0, 0.708), BLACK)],  # ring.rs:47-68
    "PAT_GRADIENT": [((0, 0, 0), WHITE), ((0.25, 0, 0), (0.75,) * 3), ((0.5, 0, 0), (0.5,) * 3), ((0.75, 0, 0), (0.25,) * 3)],  # gradient.rs:44-64
    "PAT_CHECKER3D": [((0, 0, 0), WHITE), ((0.99, 0, 0), WHITE), ((1.01, 0, 0), BLACK), ((0, 0.99, 0), WHITE), ((0, 1.01, 0), BLACK),
                      ((0, 0, 0.99), WHITE), ((0, 0, 1.01), BLACK)],  # checker3d.rs:44-96
}


def test_the_model_gives_the_references_pattern_tables(rl):
    for name, rows in AT_LOCAL.items():
        for point, want in rows:
            colour, _ = P.rtc_pattern_at(getattr(rl.api, name), WHITE, BLACK, IDENT, [], point)
            assert tuple(colour) == tuple(want), (name, point, colour)
    # pattern/mod.rs:47-56: a pattern scaled by 2 at (2, 3, 4) is at its own (1, 1.5, 2): the probes read 1/8 + 1/2, 1.5/8 + 1/2, 2/8 + 1/2
    for axis, want in enumerate((0.625, 0.6875, 0.75)):
        inverse = axis_probe(axis)[1] @ np.linalg.inv(S(2, 2, 2))
        assert P.rtc_pattern_at(P.GRADIENT, BLACK, WHITE, inverse, [], (2.0, 3.0, 4.0))[0][0] == want
    # transformed.rs:177-198: object scaled by 2, point (2, 3, 4) -> (1, 1.5, 2); :200-223: and the pattern translated by (0.5, 1, 1.5),
    # point (2.5, 3, 3.5) -> (1.25, 1.5, 1.75) - (0.5, 1, 1.5) = (0.75, 0.5, 0.25)
    chain = [np.linalg.inv(S(2, 2, 2))]
    for axis, (w1, w2) in enumerate(zip((0.625, 0.6875, 0.75), (0.59375, 0.5625, 0.53125))):
        probe = axis_probe(axis)[1]
        assert P.rtc_pattern_at(P.GRADIENT, BLACK, WHITE, probe, chain, (2.0, 3.0, 4.0))[0][0] == w1
        assert P.rtc_pattern_at(P.GRADIENT, BLACK, WHITE, probe @ np.linalg.inv(T(0.5, 1, 1.5)), chain, (2.5, 3.0, 3.5))[0][0] == w2
    # applied in the other order (pattern inverse first, then the chain) the last case reads (2.5 - 0.5) / 2 = 1, not 0.75
    assert P.rtc_pattern_at(P.GRADIENT, BLACK, WHITE, axis_probe(0)[1] @ chain[0], [np.linalg.inv(T(0.5, 1, 1.5))], (2.5, 3.0, 3.5))[0][0] == 0.625


@pytest.mark.parametrize("name", sorted(AT_LOCAL))
def test_the_oracle_gives_the_references_pattern_tables(rl, oracle, name):
    for point, want in AT_LOCAL[name]:
        world = plane_world(rl, getattr(rl.api, name), WHITE, BLACK, T(0.0, float(point[1]), 0.0))
        got = oracle.rtc_color_at(world.desc, (float(point[0]), 1.0, float(point[2])), (0.0, -1.0, 0.0))
        assert tuple(got) == tuple(want), (name, point, got)


def probe_world(rl, shape_kind, chain, pattern_transform, axis):
    """shape under the Transformed chain (outermost first), its pattern the axis probe composed after pattern_transform
    -> (world, pattern inverse, chain inverses outermost first)"""
    b = WorldBuilder(rl.api)
    pattern_inverse = axis_probe(axis)[1] @ np.linalg.inv(pattern_transform)
    pat = b.pattern(rl.api.PAT_GRADIENT, BLACK, WHITE, IDENT)
    _set_inverse(b, pat, pattern_inverse)
    node = b.shape(shape_kind, material=ambient_only(b, pat))
    for m in reversed(chain):
        node = b.xf(m, node)
    world = b.world(rl, [node], lights=LIGHT)
    return world, pattern_inverse, [b.tr[k]["inverse"].copy() for k in range(len(chain) - 1, -1, -1)]


def test_the_oracle_applies_the_object_chain_before_the_pattern_transform(rl, oracle):
    """pattern/mod.rs:47-56 and transformed.rs:177-223 on real surfaces (the reference's tests put a mock object at a free point; a hit
    here lies on a shape).  Plane, pattern scaled by 2: the hit (2, 0, 4) is the pattern's (1, 0, 2).  Cube scaled by 2, ray (1, 1.5, -5)
    + t (0, 0, 1): t = 3, world (1, 1.5, -2), object (0.5, 0.75, -1); with the pattern translated by (0.5, 1, 1.5) the pattern point is
    (0, -0.25, -2.5).  Read as coordinate / 8 + 1/2."""
    api = rl.api
    for axis, want in enumerate((0.625, 0.5, 0.75)):
        world = probe_world(rl, api.O_PLANE, [], S(2, 2, 2), axis)[0]
        assert tuple(oracle.rtc_color_at(world.desc, (2.0, 1.0, 4.0), (0.0, -1.0, 0.0))) == (want,) * 3, axis
    for axis, (w1, w2) in enumerate(zip((0.5625, 0.59375, 0.375), (0.5, 0.46875, 0.1875))):
        world = probe_world(rl, api.O_CUBE, [S(2, 2, 2)], IDENT, axis)[0]
        assert tuple(oracle.rtc_color_at(world.desc, (1.0, 1.5, -5.0), (0.0, 0.0, 1.0))) == (w1,) * 3, axis
        world, inverse, chain = probe_world(rl, api.O_CUBE, [S(2, 2, 2)], T(0.5, 1, 1.5), axis)
        assert tuple(oracle.rtc_color_at(world.desc, (1.0, 1.5, -5.0), (0.0, 0.0, 1.0))) == (w2,) * 3, axis
        assert P.rtc_pattern_at(P.GRADIENT, BLACK, WHITE, inverse, chain, (1.0, 1.5, -2.0))[0][0] == w2


def test_lighting_with_a_pattern_applied(rl, oracle):
    """material.rs:276-318: stripe, ambient 1: (0.9, 0, 0) is white and (1.1, 0, 0) black"""
    world = plane_world(rl, rl.api.PAT_STRIPE, WHITE, BLACK, IDENT)
    assert tuple(oracle.rtc_color_at(world.desc, (0.9, 1.0, 0.0), (0.0, -1.0, 0.0))) == WHITE
    assert tuple(oracle.rtc_color_at(world.desc, (1.1, 1.0, 0.0), (0.0, -1.0, 0.0))) == BLACK
