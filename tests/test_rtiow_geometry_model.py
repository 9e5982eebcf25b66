"""CPU tier: the oracle's RTIOW primitives, instances and textures pinned against a geometric model that shares nothing with it or with
the host mirror, plus the scene builders, ray generators and directed tables that tests/test_gpu_rtiow_geometry.py imports to hold the
kernels to the same model.

The model (`Recorder` / `Model`) takes the calls a test makes on `SceneBuilder`, records them as a tree, and never looks at the flattened
scene.  It states every primitive in WORLD space: an instance chain is composed into one affine map x -> A x + b, spheres map to a centre
and |s| * radius, planars to mapped q, u, v, vertex normals go through A^-T, a moving centre is c1 + time (c2 - c1) before the map.  The
world-space ray is intersected directly, in mpmath at 60 digits on the exact binary64 inputs: planars by solving o + t d = q + a u + b v as
a 3x3 system with Cramer's rule, spheres by the roots of |o + t d - c|^2 = r^2.

Rotation convention, stated once: right-handed, counter-clockwise seen from the positive end of the axis, angle deg * pi / 180;
rotate_y(+90) takes +z to +x (and +x to -z), rotate_x(+90) takes +y to +z, rotate_z(+90) takes +x to +y.

Reference rules that are not geometry, each with a directed case of its own in DIRECTED below:
  * the parallel cut |n^ . d_obj| < 1e-8 on the unnormalised object-space direction (plane.rs:55);
  * the closed interval of Interval::contains (interval.rs:35);
  * equal t: the later hittable of a list wins (hittable/mod.rs:91-104: the fold passes max = closest t to a closed interval);
  * the face is the sign of d . n, zero counting as front (hittable/mod.rs:33), with the interpolated normal where there is one
    (triangle.rs:73-80).

Every ray also gets a list of decisions (distance to the deciding threshold, forward bound of the decided quantity): a ray with a
decision closer than its bound is `decided = False` and is left out of comparisons.  Every field gets a first-order forward rounding
bound with u = 2^-53; the counts are derived next to `Leaf.bounds_*`.
"""
import math

import mpmath as mp
import numpy as np
import pytest

DPS = 60
U = 2.0 ** -53
PARALLEL = 1e-8  # plane.rs:55
INF = float("inf")
SQ2 = math.sqrt(2.0)


# ----------------------------------------------------------------------------- mp vectors as tuples
def V(x):
    return tuple(mp.mpf(float(c)) for c in x)


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scl(s, a):
    return (s * a[0], s * a[1], s * a[2])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def norm(a):
    return mp.sqrt(dot(a, a))


def unit(a):
    return scl(1 / norm(a), a)


def mv(m, x):
    return (dot(m[0], x), dot(m[1], x), dot(m[2], x))


def mm(a, b):
    bt = tr(b)
    return tuple(tuple(dot(r, c) for c in bt) for r in a)


def tr(m):
    return tuple(tuple(m[j][i] for j in range(3)) for i in range(3))


def fl(a):
    return tuple(float(c) for c in a)


def fnorm(a):
    return math.sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2])


def rotation(axis, deg):
    """the textbook rotation by deg * pi / 180 about axis 0 / 1 / 2 (convention in the module docstring) and its inverse"""
    th = mp.mpf(float(deg)) * mp.pi / 180
    c, s = mp.cos(th), mp.sin(th)
    i, j = (axis + 1) % 3, (axis + 2) % 3
    m = [[mp.mpf(int(r == k)) for k in range(3)] for r in range(3)]
    m[i][i], m[i][j], m[j][i], m[j][j] = c, -s, s, c
    m = tuple(tuple(r) for r in m)
    return m, tr(m)


# ----------------------------------------------------------------------------- recorder
class Recorder:
    """Same calls as SceneBuilder's geometry; each goes to the builder unchanged and into `nodes` under the id the builder returned.
    mat() makes a fuzz-0 Metal whose albedo[0] is its tag, so a hit record's material index is told apart through World.materials()
    whatever order the flattening gave the materials."""

    def __init__(self, b):
        self.b, self.nodes, self.tags = b, {}, {}

    @staticmethod
    def _f(x):
        return None if x is None else np.array(x, dtype=np.float64)

    def mat(self):
        tag = len(self.tags) + 1
        m = self.b.metal((float(tag), 0.0, 0.0), 0.0)
        self.tags[m] = tag
        return m

    def _put(self, i, node):
        self.nodes[i] = node
        return i

    def sphere(self, center, radius, mat, center2=None):
        c1, c2 = self._f(center), self._f(center2)
        return self._put(self.b.sphere(c1, float(radius), mat, center2=c2), ("sphere", c1, c2, float(radius), self.tags[mat]))

    def _planar(self, kind, q, u, v, mat):
        q, u, v = self._f(q), self._f(u), self._f(v)
        i = getattr(self.b, kind)(q, u, v, mat)
        return self._put(i, ("planar", kind, q, u, v, None, None, None, self.tags[mat]))

    def plane(self, q, u, v, mat):
        return self._planar("plane", q, u, v, mat)

    def quad(self, q, u, v, mat):
        return self._planar("quad", q, u, v, mat)

    def triangle(self, q, u, v, mat):
        return self._planar("triangle", q, u, v, mat)

    def triangle_from_model(self, points, mat, uvs=None, normals=None):
        p, t, n = self._f(points), self._f(uvs), self._f(normals)
        i = self.b.triangle_from_model(p, mat, uvs=t, normals=n)
        return self._put(i, ("planar", "triangle", None, None, None, p, t, n, self.tags[mat]))

    def translate(self, obj, offset):
        o = self._f(offset)
        return self._put(self.b.translate(obj, o), ("inst", 4, o, obj))

    def rotate_x(self, obj, deg):
        return self._put(self.b.rotate_x(obj, float(deg)), ("inst", 0, float(deg), obj))

    def rotate_y(self, obj, deg):
        return self._put(self.b.rotate_y(obj, float(deg)), ("inst", 1, float(deg), obj))

    def rotate_z(self, obj, deg):
        return self._put(self.b.rotate_z(obj, float(deg)), ("inst", 2, float(deg), obj))

    def scale(self, obj, s):
        return self._put(self.b.scale(obj, float(s)), ("inst", 3, float(s), obj))

    def list(self, objs):
        return self._put(self.b.list(objs), ("group", False, list(objs)))

    def bvh(self, objs):
        return self._put(self.b.bvh(objs), ("group", True, list(objs)))


IDENT = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def _conditions(dec, conds):
    """conds = [(value that must be >= 0, its bound)] of a conjunction.  All hold: each is a decision.  Some fail: the conjunction is as
    firmly false as its most firmly violated member, and only that one is a decision."""
    failed = [(-val, bnd) for val, bnd in conds if val < 0]
    if not failed:
        dec += [(val, bnd) for val, bnd in conds]
        return True
    dec.append(max(failed, key=lambda c: c[0] / c[1] if c[1] > 0 else INF))
    return False


class Leaf:
    """One primitive in world space.  `levels` is its instance chain, outermost first, in floats, for the rounding bounds only:
    ("T", offset) or ("M", matrix, inverse, gain of the inverse, entry roundings of the inverse, entry roundings of the matrix)."""

    def __init__(self, node, A, b, Ainv, det_sign, levels, in_bvh, order):
        self.A, self.b, self.Ainv, self.levels, self.in_bvh, self.order = A, b, Ainv, levels, in_bvh, order
        self.AinvT = tr(Ainv)
        self.kind = node[0]
        if self.kind == "sphere":
            _, c1, c2, r, self.tag = node
            self.label = "sphere" if c2 is None else "moving sphere"
            self.c1 = add(mv(A, V(c1)), b)
            self.dc = None if c2 is None else sub(add(mv(A, V(c2)), b), self.c1)
            self.c1_obj, self.dc_obj_len = fl(V(c1)), (0.0 if c2 is None else fnorm(c2 - c1))
            self.r_obj = mp.mpf(r)
            self.r = self.r_obj * mp.cbrt(abs(mp.det(mp.matrix([list(row) for row in A]))))
        else:
            _, self.shape, q, u, v, pts, uvs, normals, self.tag = node
            self.label = self.shape + (" with uvs" if uvs is not None else "") + (" with normals" if normals is not None else "")
            self.edge_err = 0.0
            if pts is not None:  # triangle.rs:43-46: u and v are ROUNDED differences; the model's triangle is the three points themselves
                P = [V(p) for p in pts]
                q, u, v = P[0], sub(P[1], P[0]), sub(P[2], P[0])
                self.edge_err = 2 * U  # one rounding per edge, relative to the edge
            else:
                q, u, v = V(q), V(u), V(v)
                if self.shape == "triangle":  # triangle.rs:25-27 + 43-44: p2 = fl(q + u), u' = fl(p2 - q): two roundings at |q| + |u|, per edge
                    fq, fu, fv = fnorm(fl(q)), fnorm(fl(u)), fnorm(fl(v))
                    self.edge_err = 2 * U * ((fq + fu) / fu + (fq + fv) / fv)
            self.q_obj, self.u_obj, self.v_obj = fl(q), fl(u), fl(v)
            n_obj = cross(u, v)
            self.kappa = float(norm(u) * norm(v) / norm(n_obj))
            self.m_par = mv(self.AinvT, unit(n_obj))  # n^_obj . (A^-1 d) = (A^-T n^_obj) . d
            self.q, self.u, self.v = add(mv(A, q), b), mv(A, u), mv(A, v)
            self.n = cross(self.u, self.v)
            self.n_unit = scl(det_sign, unit(self.n))  # = unit(A^-T (u x v)): (A u) x (A v) = det(A) A^-T (u x v)
            self.uvs = None if uvs is None else [tuple(mp.mpf(float(c)) for c in t) for t in uvs]
            self.vn = None if normals is None else [mv(self.AinvT, V(n)) for n in normals]
            self.vn_obj_len = None if normals is None else [fnorm(n) for n in normals]
            self.vn_obj = None if normals is None else [V(n) for n in normals]

    # ------------------------------------------------------------------------- rounding bounds (floats, first order, u = 2^-53)
    def into_object(self, o, d):
        """-> (o', d', |err o'|, |err d'|) of the reference's object-space ray (transform.rs:147-148, translate.rs:15).
        Translate: one subtraction per component: u |o_k|.  Transform: each component is a 3-term dot product accumulated from 0.0:
        3 roundings (the second product, two additions; 0.0 + x is exact) on sum |m_ij x_j| <= sqrt(2) |row| |x| over the three rows of an
        axis rotation or a scale, plus r roundings in the entries themselves (r = 2 |theta| + 2 for a rotation: deg * (pi / 180) is two
        roundings of theta, sin and cos one ulp = 2u each; r = 1 for 1 / s): (3 + r) sqrt(2) u |x_k|, and the incoming error times the gain."""
        eo = ed = 0.0
        for lv in self.levels:
            if lv[0] == "T":
                o = (o[0] - lv[1][0], o[1] - lv[1][1], o[2] - lv[1][2])
                eo += U * fnorm(o)
            else:
                _, _, minv, g, r, _ = lv
                o = tuple(minv[i][0] * o[0] + minv[i][1] * o[1] + minv[i][2] * o[2] for i in range(3))
                d = tuple(minv[i][0] * d[0] + minv[i][1] * d[1] + minv[i][2] * d[2] for i in range(3))
                eo = g * eo + (3 + r) * SQ2 * U * fnorm(o)
                ed = g * ed + (3 + r) * SQ2 * U * fnorm(d)
        return o, d, eo, ed

    def out_of_object(self, p, ep, en):
        """-> (|err p|, |err n^|) in world space (transform.rs:156-160, translate.rs:18): the same counts outward; the forward scale is
        exact (r = 0), a rotation's entries carry the same r.  The normal is a unit vector: (3 + r) sqrt(2) u for inv_t . n, 3u for the
        normalisation (|n|^2: 3 roundings deep, halved by the root; the root; the division)."""
        for lv in reversed(self.levels):
            if lv[0] == "T":
                p = (p[0] + lv[1][0], p[1] + lv[1][1], p[2] + lv[1][2])
                ep += U * fnorm(p)
            else:
                _, m, _, g, r, rf = lv
                p = tuple(m[i][0] * p[0] + m[i][1] * p[1] + m[i][2] * p[2] for i in range(3))
                ep = ep / g + (3 + rf) * SQ2 * U * fnorm(p)
                en = en + (3 + r) * SQ2 * U + 3 * U
        return ep, en

    def hit(self, o, d, time, tmin, tmax, fo, fd):
        """-> (record or None, decisions).  o, d: the world ray in mp; fo, fd: the same in floats for the bounds."""
        oo, od, eo, ed = self.into_object(fo, fd)
        lo, ld = fnorm(oo), fnorm(od)
        if self.kind == "sphere":
            return self._hit_sphere(o, d, time, tmin, tmax, oo, od, eo, ed, lo, ld)
        return self._hit_planar(o, d, tmin, tmax, oo, od, eo, ed, lo, ld)

    def _hit_planar(self, o, d, tmin, tmax, oo, od, eo, ed, lo, ld):
        dec = []
        kap = self.kappa
        # n^ = unit(u x v): cross product 3 roundings per component relative to |u||v| = kappa |u x v|; normalisation 4 (|n|^2 3 deep halved
        # by the root -> 1.5, root 1, division 1, rounded up); plus the edges' own roundings through the cross product (kappa each)
        dn = (3 * kap + 4) * U + kap * self.edge_err
        lq = fnorm(self.q_obj)
        den_par = dot(self.m_par, d)  # the object-space n^ . d_obj, exactly
        fden = abs(float(den_par))
        dden = dn * ld + 3 * U * ld + ed  # 3-term dot product: 3 roundings; the direction's own error
        dec.append((abs(fden - PARALLEL), dden))
        if fden < PARALLEL:  # plane.rs:55
            return None, dec
        w = sub(o, self.q)
        dn_w = dot(d, self.n)
        t = -dot(w, self.n) / dn_w
        ft = float(t)
        # t = (D - n^ . o') / den, D = n^ . q: D carries dn |q| + 3u |q|; the numerator adds dn |o'| + 3u |o'| + err(o') and its own
        # subtraction u |t den|; the quotient u |t|
        dnum = (dn + 3 * U) * (lq + lo) + eo + U * abs(ft) * fden
        dt = (dnum + abs(ft) * dden) / fden + U * abs(ft)
        dec.append((abs(ft - tmin), dt))
        if tmax != INF:
            dec.append((abs(ft - tmax), dt))
        if not (tmin <= t <= tmax):  # interval.rs:35
            return None, dec
        alpha = dot(d, cross(w, self.v)) / dn_w
        beta = dot(d, cross(self.u, w)) / dn_w
        fa, fb = float(alpha), float(beta)
        p = add(o, scl(t, d))
        p_obj = tuple(oo[i] + ft * od[i] for i in range(3))
        # p' = o' + t d': err(o') + |t| err(d') + err(t) |d'| + the product's and the sum's rounding
        ep = eo + abs(ft) * ed + dt * ld + U * abs(ft) * ld + U * fnorm(p_obj)
        hp = tuple(p_obj[i] - self.q_obj[i] for i in range(3))
        lhp = fnorm(hp)
        ehp = ep + U * lhp
        # alpha = w . (hp x v), w = n / (n . n): |w| |v| = kappa / |u|.  err(hp) passes through at that rate; the cross product 3, the dot
        # product 3, w itself 3 kappa (its cross product) + 4 (n . n 3 deep, the division): (3 kappa + 10) u |hp| kappa / |u|; the edges' own
        # roundings move alpha and beta by kappa edge_err (1 + |alpha| + |beta|)
        lu, lv = fnorm(self.u_obj), fnorm(self.v_obj)
        edge = kap * self.edge_err * (1 + abs(fa) + abs(fb))
        da = kap / lu * (ehp + (3 * kap + 10) * U * lhp) + edge
        db = kap / lv * (ehp + (3 * kap + 10) * U * lhp) + edge
        edge_dist = INF
        if self.shape == "quad":  # quad.rs:40
            inside = _conditions(dec, [(fa, da), (1 - fa, da), (fb, db), (1 - fb, db)])
            edge_dist = min(abs(fa), abs(1 - fa), abs(fb), abs(1 - fb))
            assert inside == (0 <= alpha <= 1 and 0 <= beta <= 1)
            if not inside:
                return None, dec
        elif self.shape == "triangle":  # triangle.rs:65
            inside = _conditions(dec, [(fa, da), (fb, db), (1 - fa - fb, da + db + U)])
            edge_dist = min(abs(fa), abs(fb), abs(1 - fa - fb))
            assert inside == (alpha >= 0 and beta >= 0 and alpha + beta <= 1)
            if not inside:
                return None, dec
        n, en = self.n_unit, dn
        uu, vv, bu, bv = alpha, beta, da, db
        if self.shape == "triangle" and (self.vn is not None or self.uvs is not None):
            f1 = 1 - alpha - beta
            d1 = da + db + 2 * U
            if self.vn is not None:
                blend = add(add(scl(alpha, self.vn[1]), scl(beta, self.vn[2])), scl(f1, self.vn[0]))
                n = unit(blend)
                l1, l2, l3 = self.vn_obj_len
                blend_obj = add(add(scl(alpha, self.vn_obj[1]), scl(beta, self.vn_obj[2])), scl(f1, self.vn_obj[0]))
                lb = float(norm(blend_obj))
                # v2 a + v3 b + v1 f1 (triangle.rs:76): the weights' errors on the vertex normals' lengths, and 3 roundings on the terms
                eN = da * l2 + db * l3 + d1 * l1 + 3 * U * (l2 * abs(fa) + l3 * abs(fb) + l1 * abs(float(f1)))
                en = eN / lb + 3 * U
                dec.append((lb * lb, 1e-16 + 2 * lb * eN))  # NormalizedVec3::try_from gives up at |n|^2 <= 1e-16 (vec3.rs:236-247)
            if self.uvs is not None:
                (a1, b1), (a2, b2), (a3, b3) = self.uvs
                uu = a1 * f1 + a2 * alpha + a3 * beta
                vv = b1 * f1 + b2 * alpha + b3 * beta
                # t1 f1 + t2 a + t3 b (triangle.rs:86-87): the same shape
                bu = abs(float(a1)) * d1 + abs(float(a2)) * da + abs(float(a3)) * db + 3 * U * (abs(float(a1 * f1)) + abs(float(a2 * alpha)) + abs(float(a3 * beta)))
                bv = abs(float(b1)) * d1 + abs(float(b2)) * da + abs(float(b3)) * db + 3 * U * (abs(float(b1 * f1)) + abs(float(b2 * alpha)) + abs(float(b3 * beta)))
        facing = dot(d, n)  # world space; equals d_obj . n_obj up to the positive factor the normalisation removes
        dec.append((abs(float(facing)) / float(norm(d)), en + (3 * U * ld + ed) / ld))  # as a cosine: both sides divided by |d|
        front = facing <= 0
        if not front:
            n = scl(-1, n)
        bp, bn = self.out_of_object(p_obj, ep, en)
        rec = dict(t=t, p=p, normal=n, front=bool(front), u=uu, v=vv, tag=self.tag, leaf=self, edge=edge_dist,
                   flat_front=bool(dot(d, self.n_unit) <= 0), bound=dict(t=dt, p=bp, normal=bn, u=bu, v=bv))
        return rec, dec

    def _hit_sphere(self, o, d, time, tmin, tmax, oo, od, eo, ed, lo, ld):
        dec = []
        c = self.c1 if self.dc is None else add(self.c1, scl(time, self.dc))
        oc = sub(o, c)
        a, hb, cc = dot(d, d), dot(oc, d), dot(oc, oc) - self.r * self.r
        disc = hb * hb - a * cc
        # object-space magnitudes for the bounds: the scale between the spaces is s = r / r_obj; t and the ratios are invariant
        s = float(self.r / self.r_obj)
        fr = float(self.r_obj)
        loc = float(norm(oc)) / s
        fhb, fa, fcc, fdisc = float(hb) / (s * s), ld * ld, float(cc) / (s * s), float(disc) / (s ** 4)
        # centre: c1 + time (c2 - c1) (sphere.rs:27): the difference, the product, the sum: 2u |time| |c2 - c1| + u |c|
        c_obj_len = fnorm(self.c1_obj) + abs(float(time)) * self.dc_obj_len
        ec = 0.0 if self.dc is None else 2 * U * abs(float(time)) * self.dc_obj_len + U * c_obj_len
        eoc = eo + ec + U * loc
        ea = 2 * ld * ed + 3 * U * fa  # |d|^2: 3 roundings deep
        ehb = eoc * ld + loc * ed + 3 * U * loc * ld
        ecc = 2 * loc * eoc + 4 * U * (loc * loc + fr * fr)  # |oc|^2 3 deep, r r, the subtraction
        edisc = 2 * abs(fhb) * ehb + abs(fcc) * ea + fa * ecc + 2 * U * (fhb * fhb + abs(fa * fcc))  # two products and the subtraction
        dec.append((abs(fdisc), edisc))
        if disc < 0:  # sphere.rs:43
            return None, dec
        sq = mp.sqrt(disc)
        fsq = math.sqrt(max(fdisc, 0.0))
        esq = (edisc / (2 * fsq) if fsq > 0 else INF) + U * fsq
        t = None
        for root in ((-hb - sq) / a, (-hb + sq) / a):  # sphere.rs:49-57
            ft = float(root)
            et = (ehb + esq + U * (abs(fhb) + fsq)) / fa + abs(ft) * (ea / fa + U)
            dec.append((abs(ft - tmin), et))
            if tmax != INF:
                dec.append((abs(ft - tmax), et))
            if tmin <= root <= tmax:
                t = root
                break
        if t is None:
            return None, dec
        p = add(o, scl(t, d))
        outward = scl(1 / self.r, sub(p, c))
        p_obj = tuple(oo[i] + ft * od[i] for i in range(3))
        ep = eo + abs(ft) * ed + et * ld + U * abs(ft) * ld + U * fnorm(p_obj)
        en = (ep + ec + U * fr) / fr + U  # (p - c) / r (sphere.rs:61): the subtraction at |p - c| = r, the division
        n_obj = mv(self.Ainv, scl(1 / self.r_obj, sub(p, c)))  # the object's own outward normal: what get_sphere_uv is given (sphere.rs:70)
        nx, ny, nz = (float(v) for v in n_obj)
        # sphere.rs:91-98: u = (atan2(-z, x) + pi) / (2 pi), v = acos(-y) / pi.  atan2 moves by err / hypot(x, z), acos by err / sqrt(1 - y^2);
        # the functions (one ulp each), the sum and the quotients: 4u and 3u of values within [0, 1]
        rho, sy = math.hypot(nx, nz), math.sqrt(max(1 - ny * ny, 0.0))
        bu = (en / rho if rho > 0 else INF) / (2 * math.pi) + 4 * U
        bv = (en / sy if sy > 0 else INF) / math.pi + 3 * U
        if nx < 0:
            dec.append((abs(nz), en))  # atan2 jumps by 2 pi across z = 0 at x < 0
        uu = (mp.atan2(-n_obj[2], n_obj[0]) + mp.pi) / (2 * mp.pi)
        vv = mp.acos(-n_obj[1]) / mp.pi
        facing = dot(d, outward)
        dec.append((abs(float(facing)) / float(norm(d)), en + (3 * U * ld + ed) / ld))
        front = facing <= 0
        n = outward if front else scl(-1, outward)
        bp, bn = self.out_of_object(p_obj, ep, en)
        rec = dict(t=t, p=p, normal=n, front=bool(front), u=uu, v=vv, tag=self.tag, leaf=self, edge=INF,
                   bound=dict(t=et, p=bp, normal=bn, u=bu, v=bv))
        return rec, dec


class Model:
    """The world-space primitives of a recorded scene, in the order the reference's lists visit them."""

    def __init__(self, rec, root):
        self.leaves = []
        with mp.workdps(DPS):
            ident = tuple(tuple(mp.mpf(c) for c in r) for r in IDENT)
            self._walk(rec.nodes, root, ident, V((0, 0, 0)), ident, 1, [], False)

    def _walk(self, nodes, i, A, b, Ainv, det_sign, levels, in_bvh):
        node = nodes[i]
        if node[0] == "group":
            for c in node[2]:
                self._walk(nodes, c, A, b, Ainv, det_sign, levels, in_bvh or node[1])
        elif node[0] == "inst":
            _, op, param, child = node
            if op == 4:
                off = V(param)
                self._walk(nodes, child, A, add(mv(A, off), b), Ainv, det_sign, levels + [("T", fl(off))], in_bvh)
            else:
                if op == 3:
                    s = mp.mpf(param)
                    m = tuple(tuple(s * c for c in r) for r in IDENT)
                    minv = tuple(tuple(c / s for c in r) for r in IDENT)
                    g, r, rf, sign = 1 / abs(param), 1, 0, (1 if param > 0 else -1)
                else:
                    m, minv = rotation(op, param)
                    g, r, sign = 1.0, 2 * abs(math.radians(param)) + 2, 1
                    rf = r
                lv = ("M", tuple(fl(row) for row in m), tuple(fl(row) for row in minv), g, r, rf)
                self._walk(nodes, child, mm(A, m), b, mm(minv, Ainv), det_sign * sign, levels + [lv], in_bvh)
        else:
            self.leaves.append(Leaf(node, A, b, Ainv, det_sign, levels, in_bvh, len(self.leaves)))

    def trace(self, origins, dirs, times=None, tmin=1e-10, tmax=INF):
        """-> one dict per ray: hit, and for a hit t, p, normal, u, v (mp), front, tag, edge (distance of (alpha, beta) to the hit
        planar's edge), bound (per field, floats); decided: every decision on the ray's way lies further from its threshold than its
        bound; ratio_min: the smallest distance / bound among the decisions."""
        out = []
        with mp.workdps(DPS):
            for k in range(len(origins)):
                o, d = V(origins[k]), V(dirs[k])
                fo, fd = fl(o), fl(d)
                time = mp.mpf(0.0 if times is None else float(times[k]))
                best, decisions, hits = None, [], []
                for leaf in self.leaves:
                    rec, dec = leaf.hit(o, d, time, tmin, tmax, fo, fd)
                    decisions += dec
                    if rec is not None:
                        hits.append(rec)
                        if best is None or rec["t"] <= best["t"]:  # equal t: the later one (hittable/mod.rs:91-104)
                            best = rec
                for rec in hits:
                    if rec is not best:  # the gap to every other candidate against both t's bounds
                        decisions.append((abs(float(rec["t"] - best["t"])), rec["bound"]["t"] + best["bound"]["t"]))
                ratio = min((dist / bnd if bnd > 0 else INF) for dist, bnd in decisions) if decisions else INF
                res = dict(hit=best is not None, decided=ratio > 1.0, ratio_min=ratio)
                if best is not None:
                    res.update(best)
                out.append(res)
        return out


def build_scene(rl, fn):
    """fn(Recorder) -> root id; -> (World, Model)"""
    keep = {}

    def go(b):
        rec = Recorder(b)
        root = fn(rec)
        keep["rec"], keep["root"] = rec, root
        return root

    world = rl.World.build(go)
    return world, Model(keep["rec"], keep["root"])


def material_tags(world):
    """material index of a hit record -> the tag Recorder.mat() gave it"""
    return np.rint(world.materials()["albedo"][:, 0]).astype(np.int64)


# ----------------------------------------------------------------------------- comparison
FIELDS = ("t", "p", "normal", "u", "v")


def compare(res, got, worst, where):
    """One decided ray: `got` = dict(t, p, normal, front, u, v, tag) or None.  hit, front and the material exact, every other field within
    the model's bound; `worst` collects the largest observed / bound per field."""
    if not res["hit"]:
        assert got is None, (where, got)
        return
    assert got is not None, (where, float(res["t"]), res["tag"])
    assert got["tag"] == res["tag"] and got["front"] == res["front"], (where, got, res["tag"], res["front"])
    with mp.workdps(DPS):
        err = dict(t=abs(mp.mpf(float(got["t"])) - res["t"]), u=abs(mp.mpf(float(got["u"])) - res["u"]), v=abs(mp.mpf(float(got["v"])) - res["v"]),
                   p=norm(sub(V(got["p"]), res["p"])), normal=norm(sub(V(got["normal"]), res["normal"])))
        for f in FIELDS:
            bnd = res["bound"][f]
            ratio = float(err[f]) / bnd if bnd > 0 else (0.0 if err[f] == 0 else INF)
            worst[f] = max(worst.get(f, 0.0), ratio)
            assert ratio <= 1.0, (where, f, float(err[f]), bnd, got, res["leaf"].kind, len(res["leaf"].levels))


def oracle_record(oracle, world, tags, o, d, time, tmin, tmax):
    h = oracle.rtiow_hit(world.desc, o, d, time, tmin, tmax)
    if h is None:
        return None
    h["tag"] = int(tags[h["mat"]])
    return h


def gpu_record(h, tags):
    """one RTIOW_HIT record -> the dict compare() takes"""
    if not h["hit"]:
        return None
    return dict(t=float(h["t"]), p=h["p"], normal=h["normal"], front=bool(h["front_face"]), u=float(h["u"]), v=float(h["v"]), tag=int(tags[h["material"]]))


# ----------------------------------------------------------------------------- random scenes
N_SCENES, N_RAYS = 40, 160  # (300 rays a scene put the two random tests at 50 s: the model's mpmath arithmetic is the cost)
BVH_EDGE = 1e-3  # (b): hits this close to the hit planar's edge are left out: the box test is a strict tmin < tmax (aabb.rs:131)
MAX_LEFT_OUT, MIN_HITS = 0.02, 100


def _basis(rng, lo, hi):
    while True:
        u, v = rng.uniform(-hi, hi, 3), rng.uniform(-hi, hi, 3)
        lu, lv = np.linalg.norm(u), np.linalg.norm(v)
        if min(lu, lv) >= lo and np.linalg.norm(np.cross(u, v)) >= 0.5 * lu * lv:
            return u, v


def random_object(rec, rng):
    kind = int(rng.integers(0, 8))
    m = rec.mat()
    c = rng.uniform(-2.0, 2.0, 3)
    if kind == 0:
        return rec.sphere(c, rng.uniform(0.4, 1.3), m)
    if kind == 1:
        return rec.sphere(c, rng.uniform(0.4, 1.3), m, center2=c + rng.uniform(-1.0, 1.0, 3))
    u, v = _basis(rng, 0.8, 2.5)
    if kind == 2:
        return rec.plane(c * 2.5, u, v, m)
    if kind == 3:
        return rec.quad(c, u, v, m)
    if kind == 4:
        return rec.triangle(c, u, v, m)
    pts = np.stack([c, c + u, c + v])
    uvs = rng.uniform(0.0, 1.0, (3, 2)) if kind in (5, 7) else None
    normals = None
    if kind in (6, 7):  # not unit length; with sigma = -1 every vertex normal is tilted more than 90 degrees from u x v
        n = np.cross(u, v)
        n /= np.linalg.norm(n)
        sigma = -1.0 if rng.random() < 0.5 else 1.0
        normals = (sigma * n + rng.uniform(-0.45, 0.45, (3, 3))) * rng.uniform(0.5, 3.0, (3, 1))
    return rec.triangle_from_model(pts, m, uvs=uvs, normals=normals)


def random_instances(rec, rng, obj, n):
    for _ in range(n):
        op = int(rng.integers(0, 5))
        if op == 4:
            obj = rec.translate(obj, rng.uniform(-1.5, 1.5, 3))
        elif op == 3:
            obj = rec.scale(obj, float(np.exp(rng.uniform(math.log(0.3), math.log(3.0)))))
        else:
            obj = (rec.rotate_x, rec.rotate_y, rec.rotate_z)[op](obj, float(rng.uniform(-360.0, 540.0)))
    return obj


def random_scene(seed, with_bvh):
    """-> fn(Recorder).  1 to 12 objects of the whole vocabulary, each bare or under 1 to 4 instances; from three objects on, the tail of
    the list may become a group of its own under further instances.  with_bvh: the root and the inner group are `bvh`s (a `list` root of
    instanced `bvh`s for every third seed)."""
    def fn(rec):
        rng = np.random.default_rng(seed)
        n = int(rng.integers(1, 13))
        objs = [random_instances(rec, rng, random_object(rec, rng), int(rng.integers(0, 5)) if rng.random() < 0.7 else 0) for _ in range(n)]
        group = rec.bvh if with_bvh else rec.list
        if n >= 3 and rng.random() < 0.6:
            k = int(rng.integers(1, n - 1))
            inner = random_instances(rec, rng, group(objs[k:]), int(rng.integers(1, 3)))
            objs = objs[:k] + [inner]
        if with_bvh and seed % 3 == 0:
            return rec.list([random_instances(rec, rng, rec.bvh(objs), 1)])
        return group(objs)
    return fn


def _targets(model, rng, n, times):
    """n world-space points on or just around the model's primitives (floats): what the rays are aimed at"""
    pts = np.zeros((n, 3))
    for k in range(n):
        leaf = model.leaves[int(rng.integers(0, len(model.leaves)))]
        if leaf.kind == "sphere":
            w = rng.normal(size=3)
            c = np.array(fl(leaf.c1)) + (0.0 if leaf.dc is None else times[k] * np.array(fl(leaf.dc)))
            pts[k] = c + float(leaf.r) * rng.uniform(0.0, 1.02) * w / np.linalg.norm(w)
        else:
            a, b = rng.uniform(-0.05, 1.05, 2)
            if leaf.shape == "triangle" and rng.random() < 0.8 and a + b > 1:
                a, b = 1 - a, 1 - b
            pts[k] = np.array(fl(leaf.q)) + a * np.array(fl(leaf.u)) + b * np.array(fl(leaf.v))
    return pts


def random_rays(model, seed, n=N_RAYS):
    """-> (origins, dirs, times): camera-like rays from one eye (unnormalised: they reach their target at t = 1), rays that start inside
    the scene, axis-parallel rays (exact zeros), and rays with direction lengths from 1e-3 to 1e3"""
    rng = np.random.default_rng(seed + 7919)
    times = rng.uniform(0.0, 1.0, n)
    tg = _targets(model, rng, n, times)
    centre, spread = tg.mean(axis=0), max(1.0, float(np.abs(tg - tg.mean(axis=0)).max()))
    n_cam, n_in, n_ax = int(0.45 * n), int(0.25 * n), int(0.15 * n)
    eye_dir = rng.normal(size=3)
    eye = centre + 3.0 * spread * eye_dir / np.linalg.norm(eye_dir)
    o = np.zeros((n, 3))
    o[:n_cam] = eye
    o[n_cam:n_cam + n_in] = centre + rng.uniform(-0.5, 0.5, (n_in, 3)) * spread
    o[n_cam + n_in + n_ax:] = centre + rng.uniform(-2.0, 2.0, (n - n_cam - n_in - n_ax, 3)) * spread
    d = tg - o
    for k in range(n_cam + n_in, n_cam + n_in + n_ax):  # through the target along one axis, from 0.5 to 4 target distances away
        axis, sign, length = int(rng.integers(0, 3)), (1.0 if rng.random() < 0.5 else -1.0), float(np.exp(rng.uniform(-1.0, 1.5)))
        d[k] = 0.0
        d[k, axis] = sign * length
        o[k] = tg[k] - d[k] * rng.uniform(0.5, 4.0)
    for k in range(n_cam + n_in + n_ax, n):
        d[k] *= 10.0 ** rng.uniform(-3.0, 3.0) / np.linalg.norm(d[k])
    return o, d, times


def interval_of(seed):
    """even seeds: the queries' default interval; odd seeds: a finite one around the camera-like rays' t = 1"""
    return (1e-10, INF) if seed % 2 == 0 else (0.125, 8.0)


SEEDS_A = [3000 + k for k in range(N_SCENES)]
SEEDS_B = [5000 + k for k in range(N_SCENES)]


def use_ray(res, with_bvh):
    return res["decided"] and not (with_bvh and res["hit"] and res["edge"] < BVH_EDGE)


_scene_cache = {}


def random_case(rl, seed, with_bvh):
    """(world, model, tags, (o, d, times), (tmin, tmax), the model's results): built and traced once per process"""
    key = (seed, with_bvh)
    if key not in _scene_cache:
        world, model = build_scene(rl, random_scene(seed, with_bvh))
        rays = random_rays(model, seed)
        tmin, tmax = interval_of(seed)
        _scene_cache[key] = (world, model, material_tags(world), rays, (tmin, tmax), model.trace(*rays, tmin=tmin, tmax=tmax))
    return _scene_cache[key]


def check_counts(per_scene, total_rays):
    """the caps of the issue: per_scene = [(seed, rays left out, hits compared)]"""
    left_out = sum(s[1] for s in per_scene)
    assert left_out <= MAX_LEFT_OUT * total_rays, (left_out, total_rays)
    for seed, _, hits in per_scene:
        assert hits >= MIN_HITS, (seed, hits)
    return left_out


LABELS = ("sphere", "moving sphere", "plane", "quad", "triangle", "triangle with uvs", "triangle with normals", "triangle with uvs with normals")


def reach(results, with_bvh, tally):
    """counts, over the compared hits: per primitive kind, per instance kind in the hit's chain, per chain depth, back faces, and smooth
    triangles whose face is not the one u x v would give"""
    for res in results:
        if not (res["hit"] and use_ray(res, with_bvh)):
            continue
        leaf = res["leaf"]
        tally[leaf.label] = tally.get(leaf.label, 0) + 1
        tally["depth %d" % min(len(leaf.levels), 4)] = tally.get("depth %d" % min(len(leaf.levels), 4), 0) + 1
        for lv in leaf.levels:
            op = "translate" if lv[0] == "T" else ("scale" if lv[5] == 0 else "rotate")
            tally[op] = tally.get(op, 0) + 1
        tally["back"] = tally.get("back", 0) + (not res["front"])
        if leaf.kind != "sphere" and leaf.vn is not None:
            tally["face from the blend"] = tally.get("face from the blend", 0) + (res["flat_front"] != res["front"])


def check_reach(tally):
    for key in LABELS + ("depth 0", "depth 1", "depth 2", "depth 3", "depth 4", "translate", "scale", "rotate", "back", "face from the blend"):
        assert tally.get(key, 0) >= 100, (key, tally)


def _run_random(rl, oracle, seeds, with_bvh):
    worst, per_scene, tally = {}, [], {}
    for seed in seeds:
        world, model, tags, (o, d, times), (tmin, tmax), results = random_case(rl, seed, with_bvh)
        left, hits = 0, 0
        for i, res in enumerate(results):
            if not use_ray(res, with_bvh):
                left += 1
                continue
            compare(res, oracle_record(oracle, world, tags, o[i], d[i], times[i], tmin, tmax), worst, (seed, i))
            hits += res["hit"]
        reach(results, with_bvh, tally)
        per_scene.append((seed, left, hits))
    left_out = check_counts(per_scene, len(seeds) * N_RAYS)
    check_reach(tally)
    print(sorted(tally.items()))
    print(f"bvh={with_bvh}: {len(seeds) * N_RAYS} rays, {left_out} left out, fewest compared hits {min(s[2] for s in per_scene)}, "
          "worst observed / bound " + " ".join(f"{f} {worst.get(f, 0.0):.3f}" for f in FIELDS))


def test_random_list_scenes_meet_the_model(rl, oracle):
    """(a): bare `list` roots: no box lies on the reference's path"""
    _run_random(rl, oracle, SEEDS_A, False)


def test_random_bvh_scenes_meet_the_model(rl, oracle):
    """(b): the same vocabulary inside `bvh` roots and `bvh`s inside instances: a box too small for a rotated, scaled or moving child
    would lose hits the model sees"""
    _run_random(rl, oracle, SEEDS_B, True)


# ----------------------------------------------------------------------------- (b) directed box scenes
def box_scene_thin_and_turned(rec):
    """two axis-aligned quads (zero-thickness boxes, padded by DELTA: aabb.rs:15-20), a quad turned 45 degrees about y and one about z under
    a scale, and a moving sphere, in one bvh"""
    q1 = rec.quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), rec.mat())
    q2 = rec.quad((3.0, 0.0, -1.0), (0.0, 0.0, 2.0), (0.0, 2.0, 0.0), rec.mat())
    q3 = rec.translate(rec.rotate_y(rec.quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), rec.mat()), 45.0), (0.0, 0.0, -4.0))
    q4 = rec.translate(rec.scale(rec.rotate_z(rec.quad((-1.0, -1.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0), rec.mat()), 45.0), 1.5), (-5.0, 0.0, 0.0))
    ms = rec.sphere((0.0, 4.0, 0.0), 0.5, rec.mat(), center2=(3.0, 5.0, 1.0))
    return rec.bvh([q1, q2, q3, q4, ms])


def box_scene_rays(model):
    """aimed, from inside the margin (alpha, beta in {0.002, 0.5, 0.998}), at each quad through its box's corners and faces from several
    sides; at the moving sphere at time 0, 0.5 and 1 near the ends of its swept box"""
    rng = np.random.default_rng(77)
    o, d, times = [], [], []
    for leaf in model.leaves:
        for _ in range(4):
            w = rng.normal(size=3)
            w /= np.linalg.norm(w)
            if leaf.kind == "sphere":
                for time in (0.0, 0.5, 1.0):
                    c = np.array(fl(leaf.c1)) + time * np.array(fl(leaf.dc))
                    for sgn in (-1.0, 1.0):  # towards the surface point furthest along / against the motion
                        target = c + sgn * 0.45 * np.array(fl(leaf.dc)) / np.linalg.norm(fl(leaf.dc)) + 0.05 * w
                        o.append(target + 6.0 * w), d.append(-6.0 * w), times.append(time)
            else:
                for a in (0.002, 0.5, 0.998):
                    for b in (0.002, 0.5, 0.998):
                        target = np.array(fl(leaf.q)) + a * np.array(fl(leaf.u)) + b * np.array(fl(leaf.v))
                        o.append(target + 6.0 * w), d.append(-6.0 * w), times.append(0.0)
    return np.array(o), np.array(d), np.array(times)


def box_case(rl):
    if "box" not in _scene_cache:
        world, model = build_scene(rl, box_scene_thin_and_turned)
        rays = box_scene_rays(model)
        _scene_cache["box"] = (world, model, material_tags(world), rays, (1e-10, INF), model.trace(*rays))
    return _scene_cache["box"]


def test_thin_turned_and_moving_children_of_a_bvh(rl, oracle):
    world, model, tags, (o, d, times), (tmin, tmax), results = box_case(rl)
    worst, hits, left = {}, 0, 0
    for i, res in enumerate(results):
        if not use_ray(res, True):
            left += 1
            continue
        compare(res, oracle_record(oracle, world, tags, o[i], d[i], times[i], tmin, tmax), worst, ("box", i))
        hits += res["hit"]
    print(f"box scene: {len(results)} rays, {left} left out, {hits} hits; worst " + " ".join(f"{f} {worst.get(f, 0.0):.3f}" for f in FIELDS))
    assert left <= MAX_LEFT_OUT * len(results) and hits >= 0.6 * len(results), (left, hits, len(results))
    assert {r["tag"] for r in results if r["hit"]} == {1, 2, 3, 4, 5}  # every child is reached


# ----------------------------------------------------------------------------- (c) directed cases, exact
Q0, QU, QV = (0.0, 0.0, 0.0), (2.0, 0.0, 0.0), (0.0, 2.0, 0.0)
UP = np.nextafter


def _quad(rec):
    return rec.list([rec.quad(Q0, QU, QV, rec.mat())])


def _tri(rec):
    return rec.list([rec.triangle(Q0, QU, QV, rec.mat())])


def _sphere(rec):
    return rec.list([rec.sphere((0.0, 0.0, 0.0), 1.0, rec.mat())])


def _down(x, y):
    """from (x, y, 4) straight down: t = 4 on the plane z = 0"""
    return ((x, y, 4.0), (0.0, 0.0, -1.0))


def _hitz(x, y, a, b, t=4.0, front=True, n=(0.0, 0.0, 1.0), tag=1):
    return dict(t=t, p=(x, y, 0.0), normal=n, front=front, u=a, v=b, tag=tag)


def directed_cases():
    """-> [dict(name, fn, tmin, tmax, rays [(o, d)], want [None | dict], tol)]: tol 0 compares every field with ==.  The inputs are
    dyadic, so every intermediate of the reference's arithmetic is representable and the expected record is exact; the expected values are
    worked out by hand in the comments."""
    cases = []

    def case(name, fn, rays, want, tmin=1e-10, tmax=INF, tol=0.0):
        assert len(rays) == len(want)
        cases.append(dict(name=name, fn=fn, tmin=tmin, tmax=tmax, rays=rays, want=want, tol=tol))

    # quad q = 0, u = (2, 0, 0), v = (0, 2, 0): n = (0, 0, 4), n^ = (0, 0, 1), D = 0, w = (0, 0, 1/4); from (x, y, 4) along -z: denom = -1,
    # t = (0 - 4) / -1 = 4, p = (x, y, 0), alpha = 1/4 (2 x) = x / 2, beta = y / 2.  The edges and corners are hits (quad.rs:40); the next
    # double above 2 gives alpha = 1 + 2^-52; the smallest normal number below 0 gives alpha = -2^-1023, a subnormal but not zero.
    above2, below0 = float(UP(2.0, 3.0)), -2.0 ** -1022
    pts = [(0.0, 1.0), (2.0, 1.0), (1.0, 0.0), (1.0, 2.0), (0.0, 0.0), (2.0, 0.0), (0.0, 2.0), (2.0, 2.0), (0.5, 1.5)]
    out = [(above2, 1.0), (1.0, above2), (below0, 1.0), (1.0, below0), (above2, above2)]
    case("quad edges and corners", _quad, [_down(x, y) for x, y in pts + out], [_hitz(x, y, x / 2, y / 2) for x, y in pts] + [None] * len(out))
    # triangle on the same q, u, v (Triangle::new: p2 = q + u and u = p2 - q are exact here): alpha + beta = 1 on the hypotenuse, both
    # legs, the three vertices (triangle.rs:65); (1.25, 1) has alpha + beta = 1.125
    pts = [(1.0, 1.0), (0.5, 1.5), (1.5, 0.5), (1.0, 0.0), (0.0, 1.0), (0.0, 0.0), (2.0, 0.0), (0.0, 2.0), (0.5, 0.5)]
    case("triangle edges and vertices", _tri, [_down(x, y) for x, y in pts + [(1.25, 1.0), (below0, 1.0)]],
         [_hitz(x, y, x / 2, y / 2) for x, y in pts] + [None, None])
    # Interval::contains is closed (interval.rs:35): t = 4 at tmin = 4 and at tmax = 4 is a hit, one ulp inside either end is a miss
    after4, before4 = float(UP(4.0, 5.0)), float(UP(4.0, 3.0))
    for tmin, tmax, hit in ((4.0, 10.0, True), (1.0, 4.0, True), (after4, 10.0, False), (1.0, before4, False)):
        case(f"planar t at the interval's end {tmin} {tmax}", _quad, [_down(1.0, 1.0)], [_hitz(1.0, 1.0, 0.5, 0.5) if hit else None], tmin, tmax)
    # unit sphere at 0 from (0, 0, 5) along -z: a = 1, half_b = -5, c = 24, disc = 1, r_l = 4, r_u = 6 (sphere.rs:49-57).  r_l at (0, 0, 1):
    # outward (0, 0, 1), front, u = (atan2(-1, 0) + pi) / 2 pi = (pi / 2) / (2 pi) = 1/4, v = acos(-0) / pi = 1/2, all exact in binary64
    # (fl(pi) / 2 and 3 fl(pi) / 2 are representable).  r_u at (0, 0, -1): outward (0, 0, -1) along d: back face, normal (0, 0, 1),
    # u = (atan2(1, 0) + pi) / 2 pi = 3/4.
    ray = [((0.0, 0.0, 5.0), (0.0, 0.0, -1.0))]
    near = dict(t=4.0, p=(0.0, 0.0, 1.0), normal=(0.0, 0.0, 1.0), front=True, u=0.25, v=0.5, tag=1)
    far = dict(t=6.0, p=(0.0, 0.0, -1.0), normal=(0.0, 0.0, 1.0), front=False, u=0.75, v=0.5, tag=1)
    after6, before6 = float(UP(6.0, 7.0)), float(UP(6.0, 5.0))
    for tmin, tmax, want in ((4.0, 5.0, near), (0.0, 4.0, near), (after4, 6.0, far), (6.0, 7.0, far), (after4, before6, None), (after6, 9.0, None),
                             (0.0, before4, None)):
        case(f"sphere roots at the interval's ends {tmin} {tmax}", _sphere, ray, [want], tmin, tmax)
    # the parallel cut (plane.rs:55): |n^ . d| = 1e-9 < 1e-8 misses, 1e-7 hits: t = fl(-4 / -1e-7), p.z = fl(4 + fl(t * -1e-7)) in IEEE
    # arithmetic without contraction; x and y keep their values (t * 0 = 0).  hp x v = (-2 p.z, 0, 2), so alpha = beta = 1/4 * 2 = 1/2.
    t7 = -4.0 / -1e-7
    z7 = 4.0 + t7 * -1e-7
    case("parallel cut", _quad, [((1.0, 1.0, 4.0), (0.0, 0.0, -1e-9)), ((1.0, 1.0, 4.0), (0.0, 0.0, -1e-7))],
         [None, dict(t=t7, p=(1.0, 1.0, z7), normal=(0.0, 0.0, 1.0), front=True, u=0.5, v=0.5, tag=1)])
    # under scale(100) the object-space direction is fl(1 / 100) * -1e-7, about 1e-9: cut, although the world direction is 1e-7
    # (transform.rs:148: the direction is not renormalised)
    case("parallel cut in object space", lambda rec: rec.list([rec.scale(rec.quad(Q0, QU, QV, rec.mat()), 100.0)]),
         [((100.0, 100.0, 4.0), (0.0, 0.0, -1e-7)), ((100.0, 100.0, 4.0), (0.0, 0.0, -1e-5))],
         [None, "model"])
    # back face: from below along +z: denom = 1, t = (0 + 4) / 1 = 4, d . n^ > 0: back, normal flipped (hittable/mod.rs:36)
    case("back face", _quad, [((1.0, 1.0, -4.0), (0.0, 0.0, 1.0))], [_hitz(1.0, 1.0, 0.5, 0.5, front=False, n=(0.0, 0.0, -1.0))])
    # equal t: two coincident quads in one list, the later one wins (hittable/mod.rs:91-104); and the earlier one when it is nearer
    case("equal t, the later wins", lambda rec: rec.list([rec.quad(Q0, QU, QV, rec.mat()), rec.quad(Q0, QU, QV, rec.mat())]),
         [_down(1.0, 1.0)], [_hitz(1.0, 1.0, 0.5, 0.5, tag=2)])
    case("nearer first", lambda rec: rec.list([rec.quad((0.0, 0.0, 1.0), QU, QV, rec.mat()), rec.quad(Q0, QU, QV, rec.mat())]),
         [_down(1.0, 1.0)], [dict(t=3.0, p=(1.0, 1.0, 1.0), normal=(0.0, 0.0, 1.0), front=True, u=0.5, v=0.5, tag=1)])
    # t is unchanged by scale (transform.rs:148).  scale(2): object ray o = (1/2, 1/2, 2), d = (0, 0, -1/2): denom = -1/2,
    # t = (0 - 2) / (-1/2) = 4, p' = (1/2, 1/2, 0), p = (1, 1, 0), alpha = beta = 1/4; inv_t n^ = (0, 0, 1/2), normalised by sqrt(1/4).
    # scale(1/2) from (1/2, 1/2, 4): o' = (1, 1, 8), d' = (0, 0, -2), t = 4, alpha = beta = 1/2.  rotate_z(0) is the identity exactly;
    # the translation is integer.
    case("scale keeps t", lambda rec: rec.list([rec.scale(rec.quad(Q0, QU, QV, rec.mat()), 2.0)]), [_down(1.0, 1.0)], [_hitz(1.0, 1.0, 0.25, 0.25)])
    case("scale half keeps t", lambda rec: rec.list([rec.scale(rec.quad(Q0, QU, QV, rec.mat()), 0.5)]), [_down(0.5, 0.5)], [_hitz(0.5, 0.5, 0.5, 0.5)])
    # translate(scale(rotate_z(q, 0), 2), (1, -2, 3)) from (2, -1, 7): translate: o = (1, 1, 4); then the scale(2) case: t = 4,
    # p = (1, 1, 0) + (1, -2, 3)
    case("translate of scale of rotate by 0",
         lambda rec: rec.list([rec.translate(rec.scale(rec.rotate_z(rec.quad(Q0, QU, QV, rec.mat()), 0.0), 2.0), (1.0, -2.0, 3.0))]),
         [((2.0, -1.0, 7.0), (0.0, 0.0, -1.0))], [dict(t=4.0, p=(2.0, -1.0, 3.0), normal=(0.0, 0.0, 1.0), front=True, u=0.25, v=0.25, tag=1)])
    # sphere radius 1 at (1, 0, 0) under scale(2) from (2, 0, 10): o' = (1, 0, 5), d' = (0, 0, -1/2), oc = (0, 0, 5), a = 1/4,
    # half_b = -5/2, c = 24, disc = 25/4 - 6 = 1/4, r_l = (5/2 - 1/2) / (1/4) = 8, p' = (1, 0, 1), outward (0, 0, 1), p = (2, 0, 2)
    case("sphere under scale", lambda rec: rec.list([rec.scale(rec.sphere((1.0, 0.0, 0.0), 1.0, rec.mat()), 2.0)]),
         [((2.0, 0.0, 10.0), (0.0, 0.0, -1.0))], [dict(t=8.0, p=(2.0, 0.0, 2.0), normal=(0.0, 0.0, 1.0), front=True, u=0.25, v=0.5, tag=1)])
    # a smooth triangle whose vertex normals all point along -z while u x v points along +z: from above, alpha = beta = 1/4, the blend is
    # (0, 0, -2) (1/4 + 1/4 + 1/2), its unit (0, 0, -1) lies along d: back face, normal (0, 0, 1) (triangle.rs:73-80)
    case("the blend decides the face",
         lambda rec: rec.list([rec.triangle_from_model([Q0, QU, QV], rec.mat(), normals=[(0.0, 0.0, -2.0)] * 3)]),
         [_down(0.5, 0.5), ((0.5, 0.5, -4.0), (0.0, 0.0, 1.0))],
         [_hitz(0.5, 0.5, 0.25, 0.25, front=False), _hitz(0.5, 0.5, 0.25, 0.25, front=True, n=(0.0, 0.0, -1.0))])
    # vertex UVs (triangle.rs:86-87): t1 = (0, 0), t2 = (1, 0), t3 = (0.5, 1) at alpha = 1/2, beta = 1/4: u = 0 + 1/2 + 1/8, v = 1/4
    case("vertex uvs", lambda rec: rec.list([rec.triangle_from_model([Q0, QU, QV], rec.mat(), uvs=[(0.0, 0.0), (1.0, 0.0), (0.5, 1.0)])]),
         [_down(1.0, 0.5)], [_hitz(1.0, 0.5, 0.625, 0.25)])
    # scale(-1) is accepted (transform.rs:76-86 has no check): the quad lies over [-2, 0]^2; from (-1, -1, 4): o' = (1, 1, -4),
    # d' = (0, 0, 1), denom = 1: back face in object space, t = 4, normal -n^ = (0, 0, -1), inv_t = -1: world normal (0, 0, 1), front stays 0
    case("scale by -1", lambda rec: rec.list([rec.scale(rec.quad(Q0, QU, QV, rec.mat()), -1.0)]),
         [_down(-1.0, -1.0), _down(1.0, 1.0)], [_hitz(-1.0, -1.0, 0.5, 0.5, front=False), None])
    # translate(rotate_y(q, 90), (1, 0, 0)) and rotate_y(translate(q, (1, 0, 0)), 90) are two worlds.  rotate_y(90) takes (x, y, z) to
    # (z, y, -x): the first quad lies in the plane x = 1 over z in [-2, 0], the second in x = 0 over z in [-3, -1]; both normals are +x.
    # One ray from (2, 1/2, -3/2) along -x: first world t = 1, p = (1, 1/2, -3/2), alpha = 3/4; second t = 2, p = (0, 1/2, -3/2),
    # alpha = (3/2 - 1) / 2 = 1/4.  cos 90 degrees is 6.1e-17, not 0: compared at 1e-15.
    ray = [((2.0, 0.5, -1.5), (-1.0, 0.0, 0.0))]
    case("translate of rotate", lambda rec: rec.list([rec.translate(rec.rotate_y(rec.quad(Q0, QU, QV, rec.mat()), 90.0), (1.0, 0.0, 0.0))]), ray,
         [dict(t=1.0, p=(1.0, 0.5, -1.5), normal=(1.0, 0.0, 0.0), front=True, u=0.75, v=0.25, tag=1)], tol=1e-15)
    case("rotate of translate", lambda rec: rec.list([rec.rotate_y(rec.translate(rec.quad(Q0, QU, QV, rec.mat()), (1.0, 0.0, 0.0)), 90.0)]), ray,
         [dict(t=2.0, p=(0.0, 0.5, -1.5), normal=(1.0, 0.0, 0.0), front=True, u=0.25, v=0.25, tag=1)], tol=1e-15)
    # a unit quad centred on the origin in each coordinate plane, turned by 90 degrees about each axis (and by -90 about the axis of its
    # normal's successor): the quarter turns as integer maps, R_x: (x, y, z) -> (x, -z, y), R_y: -> (z, y, -x), R_z: -> (-y, x, z).  The ray
    # starts one normal above the point (alpha, beta) = (3/4, 1/4) of the turned quad and runs against the turned normal: t = 1.
    quarter = {0: lambda p: (p[0], -p[2], p[1]), 1: lambda p: (p[2], p[1], -p[0]), 2: lambda p: (-p[1], p[0], p[2])}
    back = {0: lambda p: (p[0], p[2], -p[1]), 1: lambda p: (-p[2], p[1], p[0]), 2: lambda p: (p[1], -p[0], p[2])}
    for plane in range(3):
        e = np.eye(3)
        u, v = e[(plane + 1) % 3], e[(plane + 2) % 3]  # u x v = the plane's axis
        nrm, q = e[plane], -(u + v) / 2
        point = q + 0.75 * u + 0.25 * v
        for axis, deg in [(0, 90.0), (1, 90.0), (2, 90.0), ((plane + 1) % 3, -90.0)]:
            turn = quarter[axis] if deg > 0 else back[axis]
            p_w, n_w = np.array(turn(point)) + 0.0, np.array(turn(nrm)) + 0.0

            def fn(rec, q=q, u=u, v=v, axis=axis, deg=deg):
                return rec.list([(rec.rotate_x, rec.rotate_y, rec.rotate_z)[axis](rec.quad(q, u, v, rec.mat()), deg)])

            case(f"quad of plane {plane} turned {deg} about {axis}", fn, [(tuple(p_w + n_w), tuple(-n_w))],
                 [dict(t=1.0, p=tuple(p_w), normal=tuple(n_w), front=True, u=0.75, v=0.25, tag=1)], tol=1e-15)
    return cases


DIRECTED = directed_cases()
_directed_cache = {}


def directed_world(rl, k):
    if k not in _directed_cache:
        world, model = build_scene(rl, DIRECTED[k]["fn"])
        _directed_cache[k] = (world, model, material_tags(world))
    return _directed_cache[k]


def check_directed(case, model, records):
    """records: one dict (as compare() takes) or None per ray of the case"""
    for (o, d), want, got in zip(case["rays"], case["want"], records):
        if isinstance(want, str):  # "model": a hit whose record is the model's business; here only that it is one
            res = model.trace([o], [d], tmin=case["tmin"], tmax=case["tmax"])[0]
            assert res["hit"] and res["decided"]
            compare(res, got, {}, case["name"])
            continue
        if want is None:
            assert got is None, (case["name"], o, got)
            continue
        assert got is not None, (case["name"], o)
        assert got["tag"] == want["tag"] and got["front"] == want["front"], (case["name"], o, got)
        for f in FIELDS:
            g, w = np.asarray(got[f], dtype=np.float64), np.asarray(want[f], dtype=np.float64)
            if case["tol"] == 0.0:
                assert np.array_equal(g, w), (case["name"], o, f, got[f], want[f])
            else:
                assert np.abs(g - w).max() <= case["tol"], (case["name"], o, f, got[f], want[f])


@pytest.mark.parametrize("k", range(len(DIRECTED)), ids=[c["name"] for c in DIRECTED])
def test_directed_cases(rl, oracle, k):
    case = DIRECTED[k]
    world, model, tags = directed_world(rl, k)
    check_directed(case, model, [oracle_record(oracle, world, tags, o, d, 0.0, case["tmin"], case["tmax"]) for o, d in case["rays"]])


def test_the_model_agrees_with_the_directed_answers(rl):
    """the by-hand answers also pin the model: a model that shared a slip with the oracle would have to share it with the hand as well"""
    for k, case in enumerate(DIRECTED):
        _, model, _ = directed_world(rl, k)
        o, d = [r[0] for r in case["rays"]], [r[1] for r in case["rays"]]
        for want, res in zip(case["want"], model.trace(o, d, tmin=case["tmin"], tmax=case["tmax"])):
            if isinstance(want, str):
                continue
            assert res["hit"] == (want is not None), (case["name"], want)
            if want is None:
                continue
            assert res["tag"] == want["tag"] and res["front"] == want["front"], case["name"]
            for f in FIELDS:
                got = np.array([float(c) for c in res[f]]) if f in ("p", "normal") else float(res[f])
                assert np.abs(got - np.asarray(want[f])).max() <= 1e-15, (case["name"], f, got, want[f])


def test_scale_by_minus_one_is_accepted(rl):
    world, model = build_scene(rl, lambda rec: rec.list([rec.scale(rec.sphere((1.0, 0.0, 0.0), 1.0, rec.mat()), -1.0)]))
    assert world.counts()["transforms"] == 1 and float(model.leaves[0].r) == 1.0 and fl(model.leaves[0].c1) == (-1.0, 0.0, 0.0)


# ----------------------------------------------------------------------------- (d) textures
def rust_as_u32(x):
    """Rust's `f64 as u32`: toward zero, saturating, NaN -> 0"""
    if math.isnan(x):
        return 0
    return int(min(max(x, 0.0), 4294967295.0))


def image_index(w, h, u, v):
    """Image::value (texture.rs:63-81) from its definition: u and v clamped to [0, 1] (NaN stays NaN), v flipped, column = u (W - 1) and
    row = (1 - v) (H - 1) cut to integers -> (row, column)"""
    uc = u if math.isnan(u) else min(max(u, 0.0), 1.0)
    vc = v if math.isnan(v) else min(max(v, 0.0), 1.0)
    return rust_as_u32((1.0 - vc) * float(h - 1)), rust_as_u32(uc * float(w - 1))


def image_value(img, u, v):
    """img [H, W, 3] float32, rows top to bottom; the texel widened exactly"""
    return img[image_index(img.shape[1], img.shape[0], u, v)].astype(np.float64)


from procedural_model import checker_leaf  # noqa: E402  Checker::value with Rust's saturating casts, shared with the procedural tiers


IMAGE_SIZES = [(1, 1), (2, 3), (3, 2), (5, 4)]  # (W, H)


def image_texels(w, h):
    """distinct float32 texels: a transposed or flipped lookup cannot give the same colour"""
    k = np.arange(h * w * 3, dtype=np.float32).reshape(h, w, 3)
    return (k + np.float32(1.0)) / np.float32(64.0) + np.float32(1e-3) * k * k


def image_coordinates(w):
    edge = 1.0 / (w - 1) if w > 1 else 0.5
    return [-0.5, 0.0, float(UP(edge, 0.0)), float(UP(edge, 2.0)), 0.5, 1.0 - 2.0 ** -53, 1.0, 1.5, float("nan")]


CHECKER_COLOURS = [(0.1, 0.2, 0.3), (0.9, 0.8, 0.7), (0.5, 0.25, 0.125), (0.0, 1.0, 0.0)]


def checker_trees():
    a, b, c, d = CHECKER_COLOURS
    return [((0.5,), a, b), ((3.0,), a, ((0.5,), b, ((0.25,), c, d)))]  # one level; nested two deep


def checker_points(scale):
    pts = [(x, y, z) for x in (-0.3 * scale, 0.3 * scale) for y in (-0.3 * scale, 0.3 * scale) for z in (-0.3 * scale, 0.3 * scale)]
    pts += [(k * scale, 0.1 * scale, 0.1 * scale) for k in (-2.0, -1.0, 0.0, 1.0, 2.0, 3.0)]
    pts += [(0.1 * scale, k * scale, -0.1 * scale) for k in (-2.0, -1.0, 0.0, 1.0)] + [(-0.1 * scale, 0.1 * scale, k * scale) for k in (-2.0, -1.0, 0.0, 1.0)]
    pts += [(-scale, -scale, -scale), (-2 * scale, -scale, 0.0), (1e15, 0.1, 0.1), (-1e15, 0.1, 0.1), (1e15, -1e15, 0.1)]
    rng = np.random.default_rng(5)
    return np.array(pts + [tuple(p) for p in rng.uniform(-4.0, 4.0, (37, 3))])


def texture_world(rl):
    """-> (world, [(flattened texture id, image [H, W, 3])], [(flattened texture id, tree)]): one Lambertian sphere per texture, in a list,
    so the k-th material is the k-th texture's"""
    images = [image_texels(w, h) for w, h in IMAGE_SIZES]
    trees = checker_trees()

    def fn(b):
        def tex(tree):
            return b.solid(tree) if isinstance(tree[0], float) else b.checker(tree[0][0], tex(tree[1]), tex(tree[2]))
        ts = [b.image(img) for img in images] + [tex(t) for t in trees]
        return b.list([b.sphere((3.0 * k, 0.0, 0.0), 1.0, b.lambertian(t)) for k, t in enumerate(ts)])

    world = rl.World.build(fn)
    ids = [int(t) for t in world.materials()["texture"]]
    return world, list(zip(ids[:len(images)], images)), list(zip(ids[len(images):], trees))


def test_image_restatement_by_hand():
    """2 x 3 (W x H) image, rows top to bottom.  u = 0.5: column (0.5 * 1) cut = 0; u = 1: column 1; v = 1: row 0 (flipped); v = 0: row 2;
    v = 0.5: row (0.5 * 2) = 1; u just below 1: column 0; out of range clamps; NaN: column / row 0."""
    img = image_texels(2, 3)
    nan = float("nan")
    for u, v, row, col in [(0.5, 1.0, 0, 0), (1.0, 1.0, 0, 1), (1.0, 0.0, 2, 1), (0.0, 0.5, 1, 0), (1.0 - 2.0 ** -53, 0.0, 2, 0), (1.5, -0.5, 2, 1),
                           (-0.5, 1.5, 0, 0), (nan, 0.0, 2, 0), (1.0, nan, 0, 1), (0.0, 1.0 - 2.0 ** -53, 0, 0), (0.0, 0.49, 1, 0), (0.0, 0.51, 0, 0)]:
        assert np.array_equal(image_value(img, u, v), img[row, col].astype(np.float64)), (u, v)
    assert len({tuple(t) for t in image_texels(5, 4).reshape(-1, 3).tolist()}) == 20


def test_checker_restatement_by_hand():
    """scale 0.5: (0.1, 0.1, 0.1): 0 + 0 + 0 even; (-0.1, 0.1, 0.1): -1: odd although -1 % 2 is -1; (-0.5, 0.1, 0.1): floor(-1) = -1 odd;
    (-1, 0.1, 0.1): -2 even; (0.5, 0.1, 0.1): 1 odd; (-0.5, -0.5, -0.5): -3 odd; (1e15, 0.1, 0.1): 2e15 even."""
    a, b = CHECKER_COLOURS[:2]
    tree = checker_trees()[0]
    for p, want in [((0.1, 0.1, 0.1), a), ((-0.1, 0.1, 0.1), b), ((-0.5, 0.1, 0.1), b), ((-1.0, 0.1, 0.1), a), ((0.5, 0.1, 0.1), b),
                    ((-0.5, -0.5, -0.5), b), ((1e15, 0.1, 0.1), a), ((-0.1, -0.1, 0.1), a)]:
        assert tuple(checker_leaf(tree, p)) == want, p
    # nested: scale 3 even -> a; odd -> scale 0.5; its odd -> scale 0.25
    nested = checker_trees()[1]
    assert tuple(checker_leaf(nested, (0.1, 0.1, 0.1))) == CHECKER_COLOURS[0]
    assert tuple(checker_leaf(nested, (-0.1, 0.1, 0.1))) == CHECKER_COLOURS[3]  # 3: -1 odd; 0.5: -1 odd; 0.25: -1 odd -> d
    assert tuple(checker_leaf(nested, (3.1, 0.1, 0.1))) == CHECKER_COLOURS[1]  # 3: 1 odd; 0.5: floor(6.2) = 6 even -> b
    assert tuple(checker_leaf(nested, (3.6, 0.1, 0.1))) == CHECKER_COLOURS[2]  # 3: 1 odd; 0.5: 7 odd; 0.25: floor(14.4) = 14 even -> c


def test_texture_tables_reach_every_texel_and_every_leaf():
    for w, h in IMAGE_SIZES:
        reached = {image_index(w, h, u, v) for u in image_coordinates(w) for v in image_coordinates(h)}
        assert reached == {(j, i) for j in range(h) for i in range(w)}, (w, h)
    one, nested = checker_trees()
    assert {tuple(checker_leaf(one, q)) for q in checker_points(one[0][0])} == set(CHECKER_COLOURS[:2])
    assert {tuple(checker_leaf(nested, q)) for q in checker_points(nested[0][0])} == set(CHECKER_COLOURS)
