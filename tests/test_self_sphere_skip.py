"""CPU tier: the self-test skip of the fast sphere traversal (csrc/rl_rtiow_wave.h fast_self_miss).  A scattered ray starts on the sphere
it has just left; SHADE decides from the new ray's a, half_b and c whether its test of that sphere can accept a root, and the TRAV step
skips the sphere when it cannot.  The skip is only sound if, whenever the predicate fires, BOTH rounded roots of Sphere::hit are below
the reference's tmin = 1e-10 — self-hits ("acne") are real at grazing angles, so this is checked here against a binary64 restatement of
Sphere::hit's root arithmetic (numpy neither contracts nor fuses: the same roundings as the kernels built with -ffp-contract=off).  The
GPU's sqrt is only assumed faithful, so the roots are also checked with sqrt rounded one ulp up."""
import os

import numpy as np

U = 2.0 ** -53
TMIN = 1e-10


def _len2(x, y, z):
    return (x * x + y * y) + z * z


def _dot(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def _roots(ocx, ocy, ocz, dx, dy, dz, r2):
    """sphere.rs:32-47 as fast_sphere_hit evaluates it: a, half_b, c, disc and both roots (NaN where disc < 0)."""
    a = _len2(dx, dy, dz)
    half_b = _dot(ocx, ocy, ocz, dx, dy, dz)
    c = _len2(ocx, ocy, ocz) - r2
    disc = half_b * half_b - a * c
    with np.errstate(invalid="ignore"):
        sq = np.sqrt(disc)
    return a, half_b, c, disc, sq


# The kernel's predicate, verbatim: _skip below restates it, and test_the_restatement_matches_the_kernel keeps the two in step.
KERNEL_PREDICATE = ("const double rhs = 1e-10 * (a * half_b);",
                    "return rhs >= 1e-270 && rhs <= 1.7976931348623157e308 && 4.4408920985006262e-16 * (half_b * half_b) + 0.6 * (a * fabs(c)) < rhs;")


def _skip(a, half_b, c):
    """fast_self_miss (csrc/rl_rtiow_wave.h), the same expressions in the same order."""
    with np.errstate(invalid="ignore", over="ignore"):
        rhs = 1e-10 * (a * half_b)
        return (rhs >= 1e-270) & (rhs <= 1.7976931348623157e308) & (4.4408920985006262e-16 * (half_b * half_b) + 0.6 * (a * np.abs(c)) < rhs)


def test_the_restatement_matches_the_kernel():
    """The soundness tests below check _skip; this one checks that _skip is still what the kernel evaluates."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rendering-learning_amd", "csrc", "rl_rtiow_wave.h")).read()
    body = src[src.index("__device__ __forceinline__ bool fast_self_miss("):]
    body = body[:body.index("\n}\n")]
    lines = [ln.split("//")[0].strip() for ln in body.splitlines()[1:]]
    assert lines == ["const double a = len2(d);", "const double half_b = dot(oc, d);", "const double c = len2(oc) - s.r2;", *KERNEL_PREDICATE]


def _accepts(a, half_b, sq):
    """Does Sphere::hit accept a root >= 1e-10 (for some window max)?"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        r_l = (-half_b - sq) / a
        r_u = (-half_b + sq) / a
        return (r_l >= TMIN) | (r_u >= TMIN)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _case(rng, n):
    """Rays that leave a sphere: the origin is the rounded hit point of a ray that came in from outside (or, for a quarter of them, from
    inside: glass), the direction has a log-uniform cosine against the normal from 1e-7 (grazing) to 1, either sign, and any length."""
    r = 10.0 ** rng.uniform(-3, 6, n)
    # centres near the origin and centres about a radius away (a ground sphere under the scene)
    cen = np.where(rng.random((n, 1)) < 0.5, rng.uniform(-5, 5, (n, 3)), rng.uniform(-2, 2, (n, 3)) * r[:, None])
    r2 = r * r
    nrm = _unit(rng, n)
    # the incoming ray: from a point at 1.5 … 40 radii (or from inside, for the glass-exit cases) towards the sphere
    inside = rng.random(n) < 0.25
    tgt = cen + nrm * r[:, None]
    dist = np.where(inside, 0.0, r * 10.0 ** rng.uniform(0.2, 1.6, n))
    wob = _unit(rng, n) * (0.5 * r)[:, None]
    o0 = np.where(inside[:, None], cen + wob * 0.5, tgt + (nrm + 0.3 * _unit(rng, n)) * dist[:, None])
    d0 = (tgt - o0) * (10.0 ** rng.uniform(-1, 1, n))[:, None]
    oc0 = o0 - cen
    a0, hb0, c0, disc0, sq0 = _roots(oc0[:, 0], oc0[:, 1], oc0[:, 2], d0[:, 0], d0[:, 1], d0[:, 2], r2)
    with np.errstate(invalid="ignore"):
        rl0 = (-hb0 - sq0) / a0
        ru0 = (-hb0 + sq0) / a0
    t = np.where(rl0 >= TMIN, rl0, ru0)
    ok = np.isfinite(t) & (t >= TMIN)
    p = o0 + d0 * t[:, None]  # camera.rs / ray.rs at(): o + d * t, rounded
    oc = p - cen  # SHADE's p - center: the new ray's oc
    # new direction: cosine against the outward normal log-uniform in [1e-7, 1], sign random (inward = refraction into the sphere)
    cos = 10.0 ** rng.uniform(-7, 0, n)
    cos = np.where(rng.random(n) < 0.2, rng.uniform(0, 1, n), cos)
    sgn = np.where(rng.random(n) < 0.8, 1.0, -1.0)
    tan = _unit(rng, n)
    tan = tan - nrm * np.sum(tan * nrm, axis=1, keepdims=True)
    tan /= np.linalg.norm(tan, axis=1, keepdims=True)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    dl = 10.0 ** rng.uniform(-2, 1, n)
    d = (nrm * (sgn * cos)[:, None] + tan * sin[:, None]) * dl[:, None]
    return oc[ok], d[ok], r2[ok], r[ok], (sgn * cos)[ok], dl[ok]


def test_skip_only_where_both_rounded_roots_are_below_tmin():
    rng = np.random.default_rng(20261016)
    fired = total = 0
    for _ in range(8):
        oc, d, r2, r, cos, dl = _case(rng, 400_000)
        a, half_b, c, disc, sq = _roots(oc[:, 0], oc[:, 1], oc[:, 2], d[:, 0], d[:, 1], d[:, 2], r2)
        skip = _skip(a, half_b, c)
        hit = (disc >= 0.0) & _accepts(a, half_b, sq)
        hit_up = (disc >= 0.0) & _accepts(a, half_b, np.nextafter(sq, np.inf))  # a faithful sqrt one ulp high
        bad = skip & (hit | hit_up)
        assert not bad.any(), (oc[bad][:3], d[bad][:3], r2[bad][:3])
        assert not (skip & (cos < 0)).any()  # an inward ray never skips
        fired += int(skip.sum())
        total += len(skip)
        # acne is real: some outward rays DO have a root >= 1e-10 (mostly grazing ones), so the skip cannot be assumed
        assert (hit & (cos > 0)).any()
    assert total > 2_500_000 and fired > total // 4


def test_skip_fires_on_outward_non_grazing_rays():
    """A predicate too weak to fire would make the skip worthless.  Outward rays with cos > 1e-2 and the direction lengths of a scattered
    ray (0.5 … 2): nearly all of them skip off spheres of scene size (r <= 10); off r <= 1000 most do — the rest are origins far from the
    world's origin whose rounded hit point sits a few 1e-13 r off the surface, and about half of those do have a root >= 1e-10."""
    rng = np.random.default_rng(7)
    oc, d, r2, r, cos, dl = _case(rng, 1_000_000)
    a, half_b, c, disc, sq = _roots(oc[:, 0], oc[:, 1], oc[:, 2], d[:, 0], d[:, 1], d[:, 2], r2)
    skip = _skip(a, half_b, c)
    sel = (cos > 1e-2) & (dl >= 0.5) & (dl <= 2.0)
    small, big = sel & (r <= 10.0), sel & (r <= 1000.0)
    assert small.sum() > 10_000 and big.sum() > 20_000
    assert skip[small].mean() >= 0.999, skip[small].mean()
    assert skip[big].mean() >= 0.9, skip[big].mean()
    # over the whole log-uniform mix (cosines down to 1e-7, radii up to 1e6) about half of the outward rays skip
    out = cos > 0
    assert skip[out].mean() > 0.4


def test_degenerate_values_never_skip():
    inf, nan = np.inf, np.nan
    # ... plus a * half_b overflowing to +inf while the left-hand side stays finite (a = 1e300, half_b = 1e100)
    a = np.array([0.0, 1.0, 1.0, inf, 1.0, 1.0, 1.0, 1e-300, nan, 1e300])
    half_b = np.array([1.0, 0.0, -1.0, 1.0, inf, nan, 1.0, 1e-300, 1.0, 1e100])
    c = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, nan, 0.0, 0.0, 0.0])
    assert not _skip(a, half_b, c).any()
    # the plain outward case skips
    assert _skip(np.array([1.0]), np.array([1.0]), np.array([1e-16]))[0]
