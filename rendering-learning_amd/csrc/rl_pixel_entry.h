// Per-pixel entry of the FAST traversal (rl_rtiow_wave.h, LDS_SCENE = 4): where the camera rays of a pixel start their walk.
//
// All camera rays of one pixel leave the same lens disc through the same pixel square, and each of them walks the tree from the root with
// closest = +inf, re-discovering the same missed boxes.  Camera and scene are fixed for a render call, so this kernel does that part of
// the walk once per pixel: it walks the tree with the pixel's BEAM — every ray get_ray (camera.rs:203-216, the GEN block) can produce for
// the pixel — and writes one word per pixel, the entries a camera ray of that pixel starts from instead of the root:
//     word = e0 | e1 << 10 | e2 << 20 | 3 << 30        (entry ids as on the walk's stack, FAST_NONE = unused, e0 is visited first)
// The entries are disjoint subtrees (or leaves) that together hold every leaf the beam may touch — its box is touched by some ray of the
// beam AND (RL_PIXEL_ENTRY_SPHERE, default on) the beam is not proven to miss the sphere itself, see "The sphere test" below:
//     no such leaf -> all FAST_NONE (the sample is a miss without a single step);  one -> that leaf;  otherwise the deepest inner node
//     whose subtree holds them all, and with max_entries = 2 / 3 that node split once / twice into the reduced entries of its children
//     (the child subtree's own deepest holder), nearest first by the beam's entry distance.
//
// Why the frames cannot change.  A sphere outside the entries' subtrees has a padded leaf box that no ray of the beam touches in exact
// arithmetic.  By the guard_pad argument (rl_fast_bvh.cpp) its rounded discriminant is negative, so Sphere::hit returns None for every
// window: it can neither be the answer, nor be within a tie band of the answer, nor trip an order check, and the root walk — whether
// it rejects that sphere's boxes or visits them — gets nothing from it.  Inside an entry's subtree the walk is the root walk's own
// reject-only walk.  So answer, amb flag, re-traces and panic-site counts are those of the root walk for every ray it trusts.
// A leaf that only the sphere test removed has its box touched, so the box-only cut visits it.  No point (t >= 0) of any camera ray of
// the pixel lies within r + pad of its centre, pad = guard_pad (the sphere grown by it lies inside the leaf box; the ball tested below is larger still).  Either the ray's LINE stays that far away too: then r^2 - b^2 <= -2 r pad
// and by the guard_pad argument the rounded discriminant is negative, fast_sphere_hit returns at `disc < 0`.  Or the line meets the
// sphere behind the origin only: then c = |oc|^2 - r^2 >= 2 r pad, eight times what rounding moves a c by, so the rounded a c is positive and
// disc <= RN(half_b^2), sq <= |half_b| (sqrt of a rounded square returns the magnitude), and half_b > 0: both rounded roots are <= 0 < 1e-10
// and the visit returns at the window test.  Both returns come before closest, hit_prim or amb are touched: the visit the box-only cut
// pays changes nothing, and answer, re-traces (slow_traces) and panic-site counts are those of the box-only table.
// (No occlusion culling here: a leaf behind a sphere the whole beam hits stays, since dropping it would change which rays are re-traced.)
//
// The beam test is CONSERVATIVE: "missed" only when no ray of the beam touches the stored box.  A ray is o + t d, t >= 0, with
// o = lookfrom + a U + b V (|(a, b)| <= 1; U = V = 0 without defocus) and o + d = T = pixel_center + sx du + sy dv, |sx|, |sy| <= 1/2; so
// its points are (1 - t) o + t T.  Per axis k, with O_k = [lookfrom_k -+ (|U_k| + |V_k|)] and T_k = [pc_k -+ (|du_k| + |dv_k|) / 2]:
//     0 <= t <= 1:  x_k(t) in [Olo + t (Tlo - Olo), Ohi + t (Thi - Ohi)]
//     t >= 1:       x_k(t) in [Ohi + t (Tlo - Ohi), Olo + t (Thi - Olo)]
// both ends linear in t: "inside the box's slab" is two linear inequalities per axis and piece, the six of a piece cut an interval of t,
// and the box is missed when that interval is empty in both pieces (a superset test: the three axes may use different rays).
// Rounding.  The kernel's ray is the ROUNDED (o, d) of GEN: pixel_center, pixel_sample and o carry at most 8u M of error each, u = 2^-53,
// M = the sum of the magnitudes that enter them (|p00| + W |du| + H |dv| + |lookfrom| + |U| + |V|, largest axis), and d = RN(ps - o)
// moves the point at t by t u |d| <= 2 t u M: the ray's points lie within 18u M (1 + t) of the exact beam's.  The lines above are
// evaluated in binary64 too (their offsets and slopes carry <= 4u M).  So every line is pushed OUTWARDS by delta (1 + t) with
// delta = 2^-40 M = 8192u M — offset -+ delta, slope -+ delta — several hundred times the sum of all of that.  The inequalities are then
// solved by one subtraction and one division each (relative error <= 2.01u in the bound of t, sign exact); an interval [lo, hi] of t
// counts as empty only when lo > hi + 1e-12 (|lo| + |hi|), five thousand times those roundings.  NaN fails every comparison and fmax / fmin
// drop it: a NaN or infinity anywhere removes constraints, never adds one, and a non-finite delta makes every box "touched".
//
// The sphere test (leaves only; inner nodes keep the box test).  Camera rays skim the sphere field and cross many box corners without
// meeting the sphere; each such leaf in a word costs every camera ray of the pixel a binary64 Sphere::hit that ends at the discriminant.
// With the axis A(t) = (1 - t) lookfrom + t pixel_center, a point of the beam is P(t) - A(t) = (1 - t)(a U + b V) + t (sx du + sy dv), so
//     |P(t) - A(t)| <= w(t) = |1 - t| rho_o + t rho_t,    rho_o = the largest singular value of [U V] (0 without defocus) >= |a U + b V|,
//                                                         rho_t = max(|du + dv|, |du - dv|) / 2 >= |sx du + sy dv|  (convex: a corner)
// and |P(t) - c| >= dist - w(t) for a centre c at distance dist from the axis LINE.  A ray can be within the sphere only while it is inside
// the sphere's padded box, i.e. for t in the hull [t_lo, t_hi] of the non-empty pieces beam_touches finds, and w is convex, so
//     dist - max(w(t_lo), w(t_hi)) > R      =>      no point of any ray of the beam lies within R of c.
// R = r + pad + |dc| / 2 around the centre at time 1/2 (rl_fast_bvh.cpp fast_leaf_balls; a moving centre stays within |dc| / 2 of it, pad is
// the largest pad of the sphere's leaf box, >= guard_pad).  Rounding.  The axis is the line through the ROUNDED lookfrom and pixel_center,
// exact by definition; the rounded ray's points lie within 18u M (1 + t) of the exact beam's and pixel_center within 8u M (above), so w
// gets the same delta (1 + t) as the box lines.  t_lo and t_hi carry <= 2.01u relative error and w has slope <= rho_o + rho_t + delta <= 2 M:
// 5u M t, inside that delta as well.  rho_o and rho_t are grown by 2^-40 relative (a dozen roundings each).  dist = |(c - lookfrom) x D| / |D|:
// the difference carries u (|c| + |lookfrom|) per axis, each component of the product 4u |c - lookfrom| |D|, root and quotient 3u:
// under 16u (|c| + |lookfrom|) in all, and the test allows eps = 2^-40 (|c|_1 + |lookfrom|_1 + R), five hundred times that.  An infinite t_hi
// and a NaN w are tested for; a non-finite R, dist or delta, or D = 0 (NaN by 0 * inf) fail the final comparison: "touched".  The test only ever removes a leaf.
//
// Time slices (RL_PIXEL_ENTRY_TIME = T = 1 | 2 | 4 | 8, default 4; leaves of moving spheres only).  The ball above holds a moving sphere for
// the whole shutter interval: R = r + pad + |dc| / 2 where the sphere's own radius is r, and in bouncing_spheres |dc| is of the order of r, so
// the ball's silhouette is several times the sphere's and every pixel in the difference sends all its camera rays through a Sphere::hit that
// the sample's time alone rules out (measured: 0.50 of the 0.68 wasted visits per camera ray, profiles/pixel_entry_time.txt).  GEN draws
// `time` before it starts the ray, so the table holds T words per pixel, [pixel][T], and a camera ray takes word k = floor(time T) —
// exact: T is a power of two and time = gen_f64() < 1, so time * T is exact and the conversion truncates (rl_pixel_entry_slices.h time_slice).
// The walk is ONE walk per pixel: inner boxes hold the whole sweep and are tested once, as above; a leaf the all-times test keeps is then
// tested, if its sphere moves, against the ball of each slice,
//     c_k = c(1/2) + dc ((k + 1/2) / T - 1/2),        R_k = R - h (1 - 1 / T),   h = RN(|dc| / 2) (fast_leaf_balls' own term of R)
// and the walk carries T + 1 cuts, the all-times one (written to the one-word table, bit for bit what the one-slice kernel writes: the root
// walks of the other kernels, T = 1 and the tests read it) and one per slice.  The split loop is the all-times table's: a slice takes ITS
// reductions of the child subtrees that loop visits, so a slice's entries lie inside the all-times entries — fewer leaves below them, never
// others — and a stationary world's slice words are the all-times word.
// Why the frames cannot change.  For time in [k / T, (k + 1) / T] the exact centre c0 + dc time lies within |dc| / (2 T) of the exact slice
// centre.  R carries r + pad + h plus a relative 1e-12 of itself plus 1e-12 |c|_max (fast_leaf_balls), about 9000u (R + |c|_max), which
// was there for the rounding of c(1/2) and of the kernel's own c0 + dc time: 2u |c|_max.  The slices add: h against |dc| / 2 (three
// roundings, 3u h), the product and the difference in R_k (2u R), and two roundings per coordinate of c_k, under 2u (|c| + |dc|) per axis,
// 4u (|c|_max + 2 h) as a length: 13u (R + |c|_max) in all, still a seven-hundredth of what R carries, so no term is added to eps:
//     R_k >= r + pad + |dc| / (2 T) + |RN(c_k) - c_k| + what the ball test's own rounding (eps, above) needs.
// (eps is taken of the ball that is tested, RN(c_k) and R_k: the distance's 16u (|c| + |lookfrom|) is in terms of that very centre.)  A leaf dropped from slice k is therefore one that no camera
// ray of the pixel, at a time of that slice, approaches within r + pad of its centre: by the argument of "The sphere test" fast_sphere_hit
// returns at `disc < 0` or at the window test, before it touches closest, hit_prim or amb.  Answer, re-traces (slow_traces) and panic-site
// counts are the all-times table's.  A motion value that is not finite (rl_fast_bvh.cpp) leaves the call with one slice; so does a box-only
// table (RL_PIXEL_ENTRY_SPHERE=0), and a sliced table above 256 MB.
#pragma once
#include "rl_rtiow_kernel.h"
#include "rl_pixel_entry_slices.h"  // time_slice, slice_ball, PIXEL_ENTRY_TIME_DEFAULT

namespace rl {

// How many entries a pixel's word may hold by default (RL_PIXEL_ENTRY / rl_debug_set_pixel_entry change it; 0 = no table, root walk)
static constexpr int PIXEL_ENTRY_DEFAULT = 3;

struct PixelBeam {
  double olo[3], ohi[3], tlo[3], thi[3];  // origin and target intervals per axis (not yet pushed outwards)
  double delta;
  // the sphere test: axis origin and direction (rounded lookfrom, pixel_center - lookfrom), 1 / |dir|, the radii of w(t) (grown)
  double f[3], dir[3], inv_len, rho_o, rho_t;
};

// true when some ray of the beam MAY touch the box b = {x.min, x.max, y.min, y.max, z.min, z.max}; [t_near, t_far]: the hull of t over the touching rays
__device__ __forceinline__ bool beam_touches(const PixelBeam &B, const float *b, double &t_near, double &t_far) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  if (!(B.delta < INF)) {  // also NaN
    t_near = 0.0, t_far = INF;
    return true;
  }
  bool touched = false;
  t_near = INF, t_far = 0.0;
#pragma unroll
  for (int piece = 0; piece < 2; piece++) {
    double lo = piece ? 1.0 : 0.0, hi = piece ? INF : 1.0;
    bool empty = false;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double bl = (double)b[2 * k], bh = (double)b[2 * k + 1];
      // lower line A + t S (pushed down), upper line C + t E (pushed up)
      const double A = (piece ? B.ohi[k] : B.olo[k]) - B.delta, S = (B.tlo[k] - (piece ? B.ohi[k] : B.olo[k])) - B.delta;
      const double C = (piece ? B.olo[k] : B.ohi[k]) + B.delta, E = (B.thi[k] - (piece ? B.olo[k] : B.ohi[k])) + B.delta;
      // A + t S <= bh
      const double a = bh - A;
      if (S > 0.0) hi = fmin(hi, a / S);
      else if (S < 0.0) lo = fmax(lo, a / S);
      else if (a < 0.0) empty = true;
      // C + t E >= bl
      const double c = bl - C;
      if (E > 0.0) lo = fmax(lo, c / E);
      else if (E < 0.0) hi = fmin(hi, c / E);
      else if (c > 0.0) empty = true;
    }
    if (lo > hi + 1e-12 * (fabs(lo) + fabs(hi))) empty = true;
    if (!empty) touched = true, t_near = fmin(t_near, lo), t_far = fmax(t_far, hi);
  }
  return touched;
}
__device__ __forceinline__ bool beam_touches(const PixelBeam &B, const float *b, double &t_near) {
  double t_far;
  return beam_touches(B, b, t_near, t_far);
}

// false only when NO ray of the beam comes within R of c while t is in [t_lo, t_hi], ball = {c.x, c.y, c.z, R} (header: the sphere test)
__device__ __forceinline__ bool beam_may_touch_ball(const PixelBeam &B, const double *ball, double t_lo, double t_hi) {
  if (!(t_hi < __longlong_as_double(0x7FF0000000000000ll))) return true;  // (also NaN; with rho_o = 0 an infinite t would make w NaN, which fmax drops)
  const double ax = ball[0] - B.f[0], ay = ball[1] - B.f[1], az = ball[2] - B.f[2], R = ball[3];
  const double cx = ay * B.dir[2] - az * B.dir[1], cy = az * B.dir[0] - ax * B.dir[2], cz = ax * B.dir[1] - ay * B.dir[0];
  const double dist = sqrt(cx * cx + cy * cy + cz * cz) * B.inv_len;
  const double w_lo = fabs(1.0 - t_lo) * B.rho_o + t_lo * B.rho_t + B.delta * (1.0 + t_lo);
  const double w_hi = fabs(1.0 - t_hi) * B.rho_o + t_hi * B.rho_t + B.delta * (1.0 + t_hi);
  const double eps = 0x1.0p-40 * (fabs(ball[0]) + fabs(ball[1]) + fabs(ball[2]) + fabs(B.f[0]) + fabs(B.f[1]) + fabs(B.f[2]) + R);
  if (!(w_lo >= 0.0 && w_hi >= 0.0)) return true;  // NaN
  return !(dist - fmax(w_lo, w_hi) - eps > R);
}

// A leaf: its box and, with `balls`, its sphere.  Returns the tables of `want` the leaf belongs to: bit 0 the all-times table, bit 1 + k slice k
// of NS - 1 (NS = 1: the all-times table alone).  A leaf the all-times ball excludes is in no slice (no ray comes within r + pad at any time),
// a stationary sphere (h == 0) is in every slice its all-times test leaves it in, a moving one in the slices whose own ball the beam may touch.
template <int NS>
__device__ __forceinline__ uint32_t beam_leaf_tables(const PixelBeam &B, const float *box, const double *balls, const double *motion, uint32_t sphere, uint32_t want,
                                                     double &t_near) {
  double t_far;
  if (!beam_touches(B, box, t_near, t_far)) return 0u;
  if (!balls) return want;
  const double *ball = balls + (size_t)sphere * 4;
  if (!beam_may_touch_ball(B, ball, t_near, t_far)) return 0u;
  if (NS == 1) return want;
  const double *mo = motion + (size_t)sphere * 4;
  if (mo[3] == 0.0) return want;
  uint32_t in = want & 1u;
#pragma unroll
  for (int k = 0; k + 1 < NS; k++)
    if ((want >> (k + 1)) & 1u) {
      double sb[4];
      slice_ball(ball, mo, (uint32_t)k, (uint32_t)(NS - 1), sb);
      if (beam_may_touch_ball(B, sb, t_near, t_far)) in |= 2u << k;
    }
  return in;
}

// What a subtree reduces to: the number of its leaves the beam may touch, the deepest entry that holds them all, the nearest t among them
struct EntryCut {
  uint32_t count, entry;
  double t_near;
};


// Reduces the subtree of entry e (its own box already found touched, at t_e): post-order walk with an explicit stack, depth <= FAST_MAX_DEPTH
// (a leaf e has passed beam_leaf_tables at its parent for every table of `want`; balls: null = box-only cut).  ONE walk for all NS tables: a box is
// tested once, a leaf counts in the tables beam_leaf_tables names, and out[s] is what the walk of table s alone would return.
template <int NS>
__device__ __forceinline__ void reduce_subtree(const RtiowParams &P, const PixelBeam &B, const double *balls, const double *motion, uint32_t e, double t_e, uint32_t want,
                                               EntryCut *out) {
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const EntryCut none{0u, FAST_NONE, INF};
  if (e >= P.n_fast_inner) {
#pragma unroll
    for (int s = 0; s < NS; s++) out[s] = ((want >> s) & 1u) ? EntryCut{1u, e, t_e} : none;
    return;
  }
  constexpr int MAXD = (int)FAST_MAX_DEPTH + 2;
  uint32_t node[MAXD], phase[MAXD];  // phase: children of node[] already handled (0 .. 2)
  EntryCut acc[MAXD][NS];            // what the handled children reduced to, per table
  int sp = 0;
  node[0] = e, phase[0] = 0;
#pragma unroll
  for (int s = 0; s < NS; s++) acc[0][s] = none, out[s] = none;
  for (;;) {
    if (phase[sp] == 2u) {  // both children handled: this node's result goes to its parent
#pragma unroll
      for (int s = 0; s < NS; s++) out[s] = acc[sp][s];
      if (sp == 0) break;
      sp--;
    } else {
      const FastNode &nd = P.fast_nodes[node[sp]];
      const uint32_t side = phase[sp]++;
      const uint32_t ce = side ? (nd.child >> 16) : (nd.child & 0xFFFFu);
      double tc;
      uint32_t in = 0u, cnt = 1u;  // the tables the child counts in, with cnt leaves
      if (ce >= P.n_fast_inner) in = beam_leaf_tables<NS>(B, nd.box[side], balls, motion, ce - P.n_fast_inner, want, tc);
      else if (beam_touches(B, nd.box[side], tc)) {
        if (sp + 1 < MAXD) {  // (always: the tree is at most FAST_MAX_DEPTH deep)
          sp++;
          node[sp] = ce, phase[sp] = 0;
#pragma unroll
          for (int s = 0; s < NS; s++) acc[sp][s] = none;
          continue;
        } else in = want, cnt = 2u;  // not walked: the child itself holds whatever lies below it
      }
#pragma unroll
      for (int s = 0; s < NS; s++) out[s] = ((in >> s) & 1u) ? EntryCut{cnt, ce, tc} : none;
    }
    // fold out[] (a child's result) into the node on top of the stack
#pragma unroll
    for (int s = 0; s < NS; s++) {
      EntryCut &a = acc[sp][s];
      if (out[s].count != 0u) {
        if (a.count != 0u) a = EntryCut{a.count + out[s].count, node[sp], fmin(a.t_near, out[s].t_near)};
        else a = out[s];
      }
    }
  }
}

// The beam of pixel (px, y) of the camera's frame.  False when a radius of the sphere test came out NaN: the box-only cut then.
__device__ __forceinline__ bool pixel_beam(const rl_rtiow_camera &cam, uint32_t px, uint32_t y, PixelBeam &B) {
  const uint32_t W = cam.image_width;
  double M = 0.0, len2 = 0.0, uu = 0.0, vv = 0.0, uv = 0.0, dp2 = 0.0, dm2 = 0.0;
  const bool lens = !(cam.defocus_angle <= 0.0);  // (NaN: GEN takes the disc branch too)
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double pc = (cam.pixel_00[k] + cam.pixel_du[k] * (double)px) + cam.pixel_dv[k] * (double)y;
    const double ht = 0.5 * (fabs(cam.pixel_du[k]) + fabs(cam.pixel_dv[k]));
    const double ho = lens ? fabs(cam.defocus_disk_u[k]) + fabs(cam.defocus_disk_v[k]) : 0.0;
    B.tlo[k] = pc - ht, B.thi[k] = pc + ht;
    B.olo[k] = cam.lookfrom[k] - ho, B.ohi[k] = cam.lookfrom[k] + ho;
    M = fmax(M, fabs(cam.pixel_00[k]) + fabs(cam.pixel_du[k]) * (double)W + fabs(cam.pixel_dv[k]) * (double)cam.image_height + fabs(cam.lookfrom[k]) +
                    fabs(cam.defocus_disk_u[k]) + fabs(cam.defocus_disk_v[k]));
    B.f[k] = cam.lookfrom[k], B.dir[k] = pc - cam.lookfrom[k];
    len2 += B.dir[k] * B.dir[k];
    const double U = cam.defocus_disk_u[k], V = cam.defocus_disk_v[k], dp = cam.pixel_du[k] + cam.pixel_dv[k], dm = cam.pixel_du[k] - cam.pixel_dv[k];
    uu += U * U, vv += V * V, uv += U * V, dp2 += dp * dp, dm2 += dm * dm;
  }
  B.inv_len = 1.0 / sqrt(len2);
  B.rho_o = lens ? sqrt(0.5 * ((uu + vv) + sqrt((uu - vv) * (uu - vv) + 4.0 * uv * uv))) * (1.0 + 0x1.0p-40) : 0.0;
  B.rho_t = 0.5 * sqrt(fmax(dp2, dm2)) * (1.0 + 0x1.0p-40);
  B.delta = M * 0x1.0p-40;
  if (!(M >= 0.0)) B.delta = __longlong_as_double(0x7FF0000000000000ll);  // NaN
  return B.rho_o >= 0.0 && B.rho_t >= 0.0;
}

// One thread per pixel of the rows this call renders: out[pr * W + px] (the kernels' shard-local pixel index), the all-times word, and with
// NS = T + 1 > 1 the words of the T time slices beside it, out_t[(pr * W + px) * T + k].  NS = 1 is the kernel of the one-word table.
template <int NS>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(256) rtiow_pixel_entry_kernel(RtiowParams P, const float *leaf_boxes, const double *leaf_balls, const double *leaf_motion,
                                                                                uint32_t max_entries, uint32_t *out, uint32_t *out_t) {
  const uint32_t W = P.cam.image_width;
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint64_t)P.nrows * W) return;
  const uint32_t pr = (uint32_t)(i / W), px = (uint32_t)(i - (uint64_t)pr * W);
  const uint32_t y = P.row_first + pr * P.row_step;
  PixelBeam B;
  if (!pixel_beam(P.cam, px, y, B)) leaf_balls = nullptr;  // NaN: the box-only cut
  constexpr uint32_t ALL = (1u << NS) - 1u;
  // the root: a leaf of its own (one sphere, no node) is tested against its leaf box, an inner node is walked
  const uint32_t root = P.fast_root;
  EntryCut c[3][NS];
  uint32_t nc = 1;
  if (root >= P.n_fast_inner) {
    double t0;
    const uint32_t in = beam_leaf_tables<NS>(B, leaf_boxes + (size_t)(root - P.n_fast_inner) * 8, leaf_balls, leaf_motion, root - P.n_fast_inner, ALL, t0);
#pragma unroll
    for (int s = 0; s < NS; s++) c[0][s] = ((in >> s) & 1u) ? EntryCut{1u, root, t0} : EntryCut{0u, FAST_NONE, 0.0};
  } else reduce_subtree<NS>(P, B, leaf_balls, leaf_motion, root, 0.0, ALL, c[0]);
  // split the holder of several leaves into its children's reduced entries, the one with the most leaves first, up to max_entries.  The
  // all-times table (c[.][0]) decides which holder is split; a slice takes its own reduction of the same child subtrees, out of the same walk,
  // so its entries lie inside the all-times entries: fewer leaves below them, never other ones.
  while (nc < max_entries && nc < 3u) {
    uint32_t pick = 3u, best = 1u;
    for (uint32_t k = 0; k < nc; k++)
      if (c[k][0].entry < P.n_fast_inner && c[k][0].count > best) pick = k, best = c[k][0].count;
    if (pick == 3u) break;
    const FastNode &nd = P.fast_nodes[c[pick][0].entry];
    double ta, tb;
    // (a holder of several leaves has them on both sides: both boxes are touched, both reductions count at least one, and a child that is
    // a leaf itself is one the reduction accepted)
    const bool ha = beam_touches(B, nd.box[0], ta), hb = beam_touches(B, nd.box[1], tb);
    if (!(ha && hb)) break;
    // a slice whose own cut of this holder's subtree is a node below it has its leaves on one side; a child that is a leaf counts for the slices
    // that hold it: both are what the walk's leaf tests say again
    EntryCut ra[NS], rb[NS];
    const uint32_t ea = nd.child & 0xFFFFu, eb = nd.child >> 16;
    uint32_t wa = ALL, wb = ALL;
    if (NS > 1) {  // a leaf child: which slices hold it (the walk above tested it; the same test, the same answer)
      double tt;
      if (ea >= P.n_fast_inner) wa = beam_leaf_tables<NS>(B, nd.box[0], leaf_balls, leaf_motion, ea - P.n_fast_inner, ALL, tt) | 1u;
      if (eb >= P.n_fast_inner) wb = beam_leaf_tables<NS>(B, nd.box[1], leaf_balls, leaf_motion, eb - P.n_fast_inner, ALL, tt) | 1u;
    }
    reduce_subtree<NS>(P, B, leaf_balls, leaf_motion, ea, ta, wa, ra);
    reduce_subtree<NS>(P, B, leaf_balls, leaf_motion, eb, tb, wb, rb);
    if (ra[0].count == 0u || rb[0].count == 0u) break;
#pragma unroll
    for (int s = 0; s < NS; s++) c[pick][s] = ra[s], c[nc][s] = rb[s];
    nc++;
  }
#pragma unroll
  for (int s = 0; s < NS; s++) {
    // the table's own cuts (a slice may hold none of an all-times entry's leaves), nearest first (at most three: a sorting network)
    EntryCut v[3];
    uint32_t m = 0;
    for (uint32_t k = 0; k < nc; k++)
      if (c[k][s].count != 0u) v[m++] = c[k][s];
    auto order = [&](uint32_t a, uint32_t b) {
      if (b < m && v[b].t_near < v[a].t_near) {
        const EntryCut t = v[a];
        v[a] = v[b], v[b] = t;
      }
    };
    order(0, 1), order(1, 2), order(0, 1);
    uint32_t w = 3u << 30;
    for (uint32_t k = 0; k < 3u; k++) w |= (k < m ? v[k].entry : FAST_NONE) << (10u * k);
    if (s == 0) out[i] = w;
    else out_t[i * (uint64_t)(NS - 1) + (uint32_t)(s - 1)] = w;
  }
}

}  // namespace rl
