"""The procedural textures from their definitions, shared by the CPU tier (tests/test_procedural_model.py) and the GPU tier
(tests/test_gpu_procedural.py).  Written from the reference's text (ray-tracing-one-weekend perlin.rs / texture.rs, ray-tracer-challenge
pattern/*.rs and material.rs), not from the oracle or the kernels, in mpmath at 60 digits on the exact binary64 inputs.

Every numeric function returns (value, bound): the value the reference's expressions have in exact arithmetic, and a first-order forward
bound on what binary64 evaluation in the reference's order can differ from it by, u = 2^-53 per rounding.  The bound is accumulated by
`Err`, one rule per operation, next to the value; the comments state what it comes to.  FMA contraction rounds less often, never more, so
the bound covers a contracting compiler too.

Rust's float -> integer `as` casts saturate and send NaN to 0 (rust_as_i32 / rust_as_i64).  Integer `+` wraps in a release build and panics
on overflow in a debug build; the project mirrors the release build, and so does this model (perlin.rs:57-59 `i + di as i32`,
texture.rs:47 `x + y + z`)."""
import math

import mpmath as mp
import numpy as np

DPS = 60
U = 2.0 ** -53
ETA = 2.0 ** -1074  # the spacing of the subnormals: what a product that underflows can lose, whatever its size
I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1


# ----------------------------------------------------------------------------- Rust's casts and integer arithmetic
def _rust_as_int(x, lo, hi):
    x = float(x)
    if math.isnan(x):
        return 0
    if x >= float(hi):  # float(hi) is 2^31 - 1 exactly, or 2^63 (hi rounds up): either way every x at or above it saturates
        return hi
    if x <= float(lo):
        return lo
    return int(x)  # toward zero


def rust_as_i32(x):
    """`x as i32` for an f64: toward zero, saturating, NaN -> 0 -> Python int"""
    return _rust_as_int(x, I32_MIN, I32_MAX)


def rust_as_i64(x):
    """`x as i64` for an f64 -> Python int.  The largest double below 2^63 is 2^63 - 1024 and converts exactly; 2^63 and everything above,
    +inf included, gives i64::MAX (odd); -2^63 and below gives i64::MIN (even)."""
    return _rust_as_int(x, I64_MIN, I64_MAX)


def wrap_i32(n):
    return (n + 2 ** 31) % 2 ** 32 - 2 ** 31


def wrap_i64(n):
    return (n + 2 ** 63) % 2 ** 64 - 2 ** 63


def rust_rem2(n):
    """`n % 2` of Rust: the sign of the dividend (-3 % 2 == -1)"""
    return -((-n) % 2) if n < 0 else n % 2


def ffloor(x):
    """f64::floor: +-inf and NaN stay"""
    x = float(x)
    return float(math.floor(x)) if math.isfinite(x) else x


# ----------------------------------------------------------------------------- value with a running first-order bound
class Err:
    """v: the exact value of an expression of binary64 inputs (an mpf); e: a bound on |computed - v| to first order in u.
    A rounded operation adds u |result|; an operation marked exact adds nothing.  Products drop the second-order term e_x e_y, and add
    ETA for gradual underflow (sums of binary64 numbers are exact down there; products are not), which matters 1 ulp from a lattice
    point at 0."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=0):
        self.v, self.e = mp.mpf(v), mp.mpf(e)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    def add(self, o, exact=False):
        o = Err.of(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + (0 if exact else U * abs(v)))

    def sub(self, o, exact=False):
        o = Err.of(o)
        v = self.v - o.v
        return Err(v, self.e + o.e + (0 if exact else U * abs(v)))

    def mul(self, o, exact=False):
        o = Err.of(o)
        v = self.v * o.v
        return Err(v, abs(self.v) * o.e + abs(o.v) * self.e + (0 if exact else U * abs(v) + ETA))


# ----------------------------------------------------------------------------- Perlin (perlin.rs:38-115)
def _cell(x):
    """-> (i, u) of one coordinate: i = floor(x) as i32 (perlin.rs:43), u = x - floor(x) (perlin.rs:39) as the binary64 it is.
    x - floor(x) is exact for every x >= 0 and every x <= -1: the difference keeps x's last bit and is no longer than x.  The one
    exception is -1 < x < 0, where 1 - |x| needs bits below 2^-53 when |x| has them: -1e-20 - (-1) rounds to 1.0.  It is a single
    correctly rounded subtraction either way, so the reference's u is this double, and the model takes it as its input."""
    f = ffloor(x)
    return rust_as_i32(f), x - f


def _hermite(u):
    """u u (3 - 2u) (perlin.rs:92) -> (uu, 1 - uu).  2u is exact; 3 - 2u, u u and their product round: uu carries 3 roundings.
    1 - uu (perlin.rs:107) rounds once more on top of uu's error."""
    eu = Err(u)
    uu = eu.mul(eu).mul(Err(3).sub(eu.mul(2, exact=True)))
    return uu, Err(1).sub(uu)


def noise(tab, p):
    """Perlin::noise (perlin.rs:38-65) + perlin_interp (:91-115) -> (value, bound) as floats; (nan, nan) for a non-finite coordinate
    (inf - inf).  tab: one record of api.PERLIN (randvec [256, 3], perm_x / perm_y / perm_z [256]).

    Cell index: floor -> saturating `as i32` -> `+ di` wrapping in 32 bits -> `& 255`.  The wrapping add is the release build's; a debug
    build of the reference panics there for i = i32::MAX, that is for every coordinate >= 2^31 - 1.

    Per corner: the three blend factors are i_f uu + (1 - i_f)(1 - uu) with i_f in {0, 1}: a product with 0, a product with 1 and a sum
    with 0, all exact, so a factor is uu (3 roundings) or 1 - uu (4).  u - i_f is exact for i_f = 0 and one rounding for i_f = 1 (u - 1 is
    exact only for u >= 1/2).  The dot product is 3 products and 2 sums; the term is 3 more products; the accumulation is 8 sums, the
    first onto 0.0 exact.  In all a corner's term carries at most 3 * 4 + (1 + 3) + 3 = 19 roundings relative to the product of the
    magnitudes, and each of the 7 later sums one of the partial sum: the bound stays below 27 u * sum |term| <= 27 u * 8 * sqrt(3)."""
    if not all(math.isfinite(float(c)) for c in p):
        return float("nan"), float("nan")
    with mp.workdps(DPS):
        cells = [_cell(float(c)) for c in p]
        (i, u), (j, v), (k, w) = cells
        blends = [_hermite(c[1]) for c in cells]
        perms = (tab["perm_x"], tab["perm_y"], tab["perm_z"])
        accum = Err(0)
        for di in range(2):
            for dj in range(2):
                for dk in range(2):
                    idx = [int(perm[wrap_i32(c + d) & 255]) for perm, c, d in zip(perms, (i, j, k), (di, dj, dk))]
                    vec = tab["randvec"][idx[0] ^ idx[1] ^ idx[2]]
                    # weight_v = (u - i_f, v - j_f, w - k_f); dot = c.x * w.x + c.y * w.y + c.z * w.z, left to right (vec3.rs:44-46)
                    wv = [Err(c[1]).sub(d, exact=(d == 0)) for c, d in zip(cells, (di, dj, dk))]
                    dot = Err(float(vec[0])).mul(wv[0]).add(Err(float(vec[1])).mul(wv[1])).add(Err(float(vec[2])).mul(wv[2]))
                    fa, fb, fc = (blends[a][0] if d else blends[a][1] for a, d in enumerate((di, dj, dk)))
                    accum = accum.add(fa.mul(fb).mul(fc).mul(dot), exact=(di + dj + dk == 0))
        return float(accum.v), float(accum.e + U * abs(accum.v) + ETA)  # + the returned double's own rounding


def _noise_err(tab, p):
    v, e = noise(tab, p)
    return Err(v, e)


def turb(tab, p, depth):
    """Perlin::turb (perlin.rs:67-79): |sum_k 2^-k noise(2^k p)| -> (value, bound).  weight is a power of two, so weight * noise and
    weight *= 0.5 are exact; temp_p * 2.0 is exact (no overflow below 2^1023 / 2^depth); abs is exact.  Each accum += rounds once, the first
    onto 0.0 not at all: the bound is sum_k 2^-k noise_bound_k plus (depth - 1) roundings of partial sums."""
    if not all(math.isfinite(float(c)) for c in p):
        return float("nan"), float("nan")
    with mp.workdps(DPS):
        accum, weight = Err(0), 1.0
        q = [float(c) for c in p]
        for it in range(depth):
            n = _noise_err(tab, q)
            accum = accum.add(n.mul(weight, exact=True), exact=(it == 0))
            weight *= 0.5
            q = [c * 2.0 for c in q]
        return float(abs(accum.v)), float(accum.e + U * abs(accum.v) + ETA)


def noise_value(tab, scale, p, turb7=None):
    """Noise::value (texture.rs:89-93): 0.5 * (1 + sin(scale * p.z + 10 * turb(p, 7))) -> (value, arithmetic bound, sin's argument).
    scale * p.z, 10 * turb and their sum round once each; |sin'| <= 1 carries the argument's error over unchanged; 1 + sin rounds once and
    the product with 0.5 is exact.  What the library's sin adds to that is not part of this bound: the caller allows for it separately.
    turb7: turb(tab, p, 7) where the caller has it already (it does not depend on the scale)."""
    t, te = turb(tab, p, 7) if turb7 is None else turb7
    z = float(p[2])
    if math.isnan(t) or not math.isfinite(z) or not math.isfinite(float(scale) * z):
        return float("nan"), float("nan"), float("nan")
    with mp.workdps(DPS):
        arg = Err(float(scale)).mul(z).add(Err(t, te).mul(10))
        s = mp.sin(arg.v)
        one = Err(s, arg.e).add(1)
        return float(one.v / 2), float(one.e / 2), float(arg.v)


def perlin_table(perm_x, perm_y, perm_z, randvec):
    """one PERLIN-shaped record without the package: the fields noise() reads"""
    tab = np.zeros(1, dtype=np.dtype([("randvec", "<f8", (256, 3)), ("perm_x", "<u4", 256), ("perm_y", "<u4", 256), ("perm_z", "<u4", 256)]))
    tab["perm_x"], tab["perm_y"], tab["perm_z"], tab["randvec"] = perm_x, perm_y, perm_z, randvec
    return tab


def lattice_table(rows):
    """hand-made table: identity permutations (or the three given), every vector zero but the listed {index: vector}"""
    perms = rows.get("perms", [np.arange(256)] * 3)
    rv = np.zeros((256, 3))
    for k, vec in rows["vectors"].items():
        rv[k] = vec
    return perlin_table(perms[0], perms[1], perms[2], rv)


def random_tables():
    """Two tables of random unit vectors (normalised normals; their length is 1 to a rounding, which the model takes as it is).  The
    first has the asymmetric permutations identity, 3i mod 256 and 5i + 1 mod 256, the second three random ones: with either, a swap of two
    tables or of two axes moves the value by far more than any bound."""
    rng = np.random.default_rng(20260)
    out = []
    k = np.arange(256)
    for perms in ([k, (3 * k) % 256, (5 * k + 1) % 256], [rng.permutation(256) for _ in range(3)]):
        v = rng.normal(size=(256, 3))
        out.append(perlin_table(perms[0], perms[1], perms[2], v / np.linalg.norm(v, axis=1, keepdims=True)))
    return out


def perlin_points():
    """-> (finite points [n, 3], non-finite points [m, 3]).  Uniform in +-40; +-1 ulp around lattice points (with the table wrap 255 | 256
    among them); -1e-20, where x - floor(x) rounds to 1.0; +-2^24; |p| on both sides of 2^31 / 64 = 2^25, where turb's 7th octave
    saturates the cast; |p| on both sides of 2^31 with one coordinate and with all three saturated; 1e300."""
    rng = np.random.default_rng(77)
    pts = [tuple(q) for q in rng.uniform(-40.0, 40.0, (110, 3))]
    for _ in range(14):
        lat = rng.choice([-256.0, -3.0, -1.0, 0.0, 1.0, 2.0, 255.0, 256.0], 3)
        for _ in range(3):
            pts.append(tuple(float(np.nextafter(c, c + s)) if s else float(c) for c, s in zip(lat, rng.integers(-1, 2, 3))))
    mid = (0.3, -7.6, 12.7)

    def one(axis, x):
        q = list(mid)
        q[axis] = x
        return tuple(q)
    for axis in range(3):
        pts += [one(axis, -1e-20), one(axis, 1e-20)]
    b24, b25, b31 = 2.0 ** 24, 2.0 ** 25, 2.0 ** 31
    pts += [one(0, b24 + 0.375), one(1, -b24 - 0.375), one(2, b24 - 0.625), (b24 + 0.25, -b24 + 0.75, b24 + 0.5)]
    for axis in range(3):
        pts += [one(axis, s * (b25 + e)) for s in (1.0, -1.0) for e in (-0.265625, 0.0, 0.265625)]
    edge31 = [b31 - 1.5, b31 - 0.75, b31, b31 + 3.25, -b31 + 1.5, -b31, -b31 - 2.5]
    pts += [one(axis, x) for axis in range(3) for x in edge31]
    pts += [(x, x, x) for x in edge31] + [(b31 + 3.25, -b31 - 2.5, b31 - 0.75)]
    pts += [one(0, 1e300), one(2, -1e300), (1e300, 1e300, 1e300), (1e19, -1e19, 0.5)]
    inf, nan = float("inf"), float("nan")
    bad = [one(0, inf), one(1, -inf), one(2, nan), (inf, inf, inf), (nan, 0.5, inf)]
    return np.array(pts), np.array(bad)


# ----------------------------------------------------------------------------- Checker (texture.rs:41-55)
def checker_leaf(tree, p):
    """Checker::value: tree = colour | ((scale,), even, odd).  inv_scale = 1 / scale (texture.rs:36); per axis floor(p * inv_scale) `as
    i64`, saturating; the three summed as i64, wrapping in a release build (a debug build panics on the overflow); Rust's % keeps the sign, so
    an odd negative sum is -1 != 0: odd.  Beyond 2^63 a coordinate is i64::MAX, which is odd; below -2^63 it is i64::MIN, which is even."""
    while not isinstance(tree[0], float):
        scale, even, odd = tree
        inv = 1.0 / scale[0]
        s = 0
        for c in p:
            s = wrap_i64(s + rust_as_i64(ffloor(float(c) * inv)))
        tree = even if rust_rem2(s) == 0 else odd
    return np.array(tree)


# ----------------------------------------------------------------------------- RTC patterns (pattern/*.rs, material.rs:13-20)
STRIPE, RING, GRADIENT, CHECKER3D = 1, 2, 3, 4  # rl_render.h RL_PAT_*


def _apply(m, q):
    """rows 0..2 of a 4 x 4 row-major matrix on the point q (w = 1)"""
    return [m[4 * r] * q[0] + m[4 * r + 1] * q[1] + m[4 * r + 2] * q[2] + m[4 * r + 3] for r in range(3)]


def _mpm(m):
    return [mp.mpf(float(x)) for x in np.asarray(m, dtype=np.float64).reshape(16)]


def pattern_point(pattern_inverse, chain_inverses, world_point):
    """pattern.inverse * (object chain inverse * world point) (pattern/mod.rs:9-11 after transformed.rs:43 per level): the stored inverse
    matrices, outermost first, then the pattern's, multiplied with the point in mpmath -> 3 mpf"""
    q = [mp.mpf(c) for c in world_point]
    for m in list(chain_inverses) + [pattern_inverse]:
        q = _apply(_mpm(m), q)
    return q


def _to_integer(x):
    return abs(x - mp.nint(x))


def _f(x):
    return float(x)


def rtc_pattern_at(kind, a, b, pattern_inverse, chain_inverses, world_point):
    """Pattern::at for the four kinds -> (colour [3] float64, second).  world_point: 3 numbers (mpf or float), taken exactly.

    Stripe (stripe.rs:21-27), ring (ring.rs:20-28), checker3d (checker3d.rs:19-25): second = the distance of the decided quantity from the
    nearest integer, x, sqrt(x^2 + z^2), and the smallest over the three coordinates: a computed point nearer to the true one than that
    decides the same colour.  checker3d adds the three floors as f64 before its one cast.
    Gradient (gradient.rs:20-25): a + (b - a) * frac(x); second = (bound, distance of x from the nearest integer).  b - a, the product
    and the sum round once each, x - floor(x) once for x < 0: bound = u (3 |b - a| frac + |a| + |colour|) per channel, its largest taken;
    the caller adds |b - a| times its own bound on x."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    with mp.workdps(DPS):
        x, y, z = pattern_point(pattern_inverse, chain_inverses, world_point)
        if kind == STRIPE:
            n, margin = rust_as_i64(_f(mp.floor(x))), _to_integer(x)
        elif kind == RING:
            r = mp.sqrt(x * x + z * z)
            n, margin = rust_as_i64(_f(mp.floor(r))), _to_integer(r)
        elif kind == CHECKER3D:
            n = rust_as_i64(_f(mp.floor(x)) + _f(mp.floor(y)) + _f(mp.floor(z)))
            margin = min(_to_integer(c) for c in (x, y, z))
        else:
            frac = x - mp.floor(x)
            colour = np.array([_f(mp.mpf(ca) + (mp.mpf(cb) - mp.mpf(ca)) * frac) for ca, cb in zip(a, b)])
            bound = max(U * (3 * abs(cb - ca) * _f(frac) + abs(ca) + abs(c)) for ca, cb, c in zip(a, b, colour))
            return colour, (bound, _f(_to_integer(x)))
        return (a if rust_rem2(n) == 0 else b).copy(), _f(margin)


def local_point_bound(pattern_inverse, chain_inverses, o, d, t):
    """A bound on each coordinate of the pattern point as binary64 arithmetic gets it from the ray: the ray's origin and direction go through
    the chain's inverses (a row is 3 products and 3 sums for a point, 3 and 2 for a vector: at most 4 and 3 roundings of the row's
    magnitudes), the local point is o' + d' * t (2 roundings) and the pattern's inverse is applied to it (4).  Magnitudes are carried as
    upper bounds |M| |x|, so the result is an upper bound whatever cancels.  -> float, the largest of the three coordinates"""
    def absm(m):
        m = np.abs(np.asarray(m, dtype=np.float64).reshape(4, 4))
        return m[:3, :3], m[:3, 3]
    ao, ad = np.abs(np.asarray(o, dtype=np.float64)), np.abs(np.asarray(d, dtype=np.float64))
    eo, ed = np.zeros(3), np.zeros(3)
    for m in chain_inverses:
        m3, tr = absm(m)
        eo, ao = m3 @ eo + 4 * U * (m3 @ ao + tr), m3 @ ao + tr
        ed, ad = m3 @ ed + 3 * U * (m3 @ ad), m3 @ ad
    t = abs(float(t))
    ap = ao + t * ad
    ep = eo + t * ed + 2 * U * ap
    m3, tr = absm(pattern_inverse)
    return float((m3 @ ep + 4 * U * (m3 @ ap + tr)).max())
