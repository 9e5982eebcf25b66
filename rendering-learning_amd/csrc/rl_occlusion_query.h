// Occlusion queries (include/rl_render.h rl_rtiow_occluded_rays*): Hittable::hit(&Ray, &Interval).is_some() on the scene
// root for a buffer of rays, one byte per ray.
//
//   rtiow_occluded_rays_kernel       the reference-order fold (general_trace), rtiow_hit_rays_kernel's body with a byte store of rec.any in
//                                    place of the record: counting calls, tmin != 1e-10, scenes without a query tree, RL_FAST=0.
//   rtiow_occluded_rays_fast_kernel  counter-free calls with tmin == 1e-10 on scenes that have a fast tree: an ANY-hit walk of that tree.
//
// The any-hit walk is the four-wide reject-only TRAV step of rtiow_hit_rays_fast_kernel (rl_ray_query.h).  The pieces it has in common
// with that kernel and the other bodies that walk this tree are called from rl_rtiow_fast_walk.h: the LDS carve with
// the tree-top staging, the ray start, the per-lane stack, the leaf's oimax, the box test with the filter's threshold.  The loop
// skeleton with its head, the node fetch with the four child tests and the stored-order visit remain a copy (ao_any_hit_walk,
// rl_rtiow_ao.h, holds the other of this form): as functions they changed this kernel's code.  Against the closest-hit form, three differences:
//   * the pruning bound is the caller's tmax from the first step to the last: nothing narrows it, no closest hit is kept, and the
//     children are visited in stored order (no sorting network);
//   * a leaf yields its root by the reference's expressions (those of fastg_sphere_hit / fastg_planar_hit) and the root is CLASSIFIED:
//       certain    1e-10 <= t <= tmax exactly, farther than the tie band below a finite tmax, and none of the cases in which the
//                  reference's own boxes may keep its fold from the primitive (grazing / pole hit, edge hit, far sphere): the ray is
//                  occluded, the lane stores 1 and leaves its walk at once;
//       uncertain  inside the interval but one of those: remembered, the walk goes on (a later certain root still decides 1);
//   * at the end without a certain root: an uncertain one, or a walk given up (filter range, grow, stack, step budget) -> the
//     reference's fold decides (general_trace at tmin = 1e-10, counted in stats[7]); otherwise 0.
// Why existence needs no order: a primitive with a certain root is reached by the reference's fold under the un-narrowed interval, and
// if the fold had narrowed the interval before it got there it had already found a hit.  So no tie test, no winner, no second
// evaluation, no normal: flagged (stats[6]) comes from re-traced rays only.
// No barrier and no wave-wide operation inside the ray loop: lanes leave their walks at different times.
#pragma once
#include "rl_ray_query.h"

namespace rl {

struct OcclusionQuery {
  const rl_ray *rays;
  unsigned long long n;
  double tmin, tmax;  // the Interval, closed at both ends
  uint8_t *occluded;  // [n]: 1 where hit() is Some
};

template <int NT, bool STATS>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_occluded_rays_kernel(RtiowParams P, OcclusionQuery Q) {
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  unsigned long long c_rays = 0, c_nodes = 0, c_sph = 0, c_pl = 0, c_inst = 0, c_flag = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const rl_ray &ray = Q.rays[idx];
    const D3 o = ld3(ray.origin), d = ld3(ray.dir);
    const double time = ray.time;
    c_rays++;
    Rec rec = rec_none(Q.tmax);
    GenCounters gc{0, 0, 0, 0, 0};
    auto draw = []() { return 0.0; };  // media are rejected on the host, as for rl_rtiow_hit_rays
    general_trace<STATS, false, false>(P, ops, 0u, NONE, o, d, o, d, time, Q.tmin, rec, gc, draw);
    c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
    Q.occluded[idx] = rec.any ? (uint8_t)1 : (uint8_t)0;
  }
  unsigned long long v;
  v = wave_sum(c_rays);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[0], v);
  v = wave_sum(c_flag);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[6], v);
  if (STATS) {
    v = wave_sum(c_nodes);
    if ((tid & 63) == 0) atomicAdd(&P.stats[1], v);
    v = wave_sum(c_sph);
    if ((tid & 63) == 0) atomicAdd(&P.stats[2], v);
    v = wave_sum(c_pl);
    if ((tid & 63) == 0) atomicAdd(&P.stats[3], v);
    v = wave_sum(c_inst);
    if ((tid & 63) == 0) atomicAdd(&P.stats[4], v);
  }
}

// what a leaf visit of the any-hit walk found
enum OccRoot : int { OCC_NONE = 0, OCC_UNCERTAIN = 1, OCC_CERTAIN = 2 };

// a root in [1e-10, tmax] is certain only when the reference's boxes, cut at tmax, cannot keep its fold from it: the condition under
// which rtiow_hit_rays_fast_kernel re-traces a winner next to a finite tmax.  `band`: the root's own error scale where that is wider.
__device__ __forceinline__ bool occ_clear_of_tmax(double t, double tmax, double band, float oimax) {
  if (!(tmax < __longlong_as_double(0x7FF0000000000000ll))) return true;
  return tmax - t > fmax(band, fast_tie_band(fabs(t) + fabs(tmax), oimax));
}

// Sphere::hit (sphere.rs:32-75) for the root only: fastg_sphere_hit's arithmetic, window [1e-10, tmax] exactly
__device__ __forceinline__ int occ_sphere_root(const DevSphere &s, uint32_t payload, D3 o, D3 d, double time, float oimax, double tmax) {
  D3 c0 = ld3(s.c0);
  D3 center = (payload & SPH_MOVING) ? c0 + ld3(s.dc) * time : c0;
  D3 oc = o - center;
  double a = len2(d);
  double half_b = dot(oc, d);
  double c = len2(oc) - s.r2;
  double disc = half_b * half_b - a * c;
  if (disc < 0.0) return OCC_NONE;
  double sq = sqrt(disc);
  double r_l = (-half_b - sq) / a;
  double r_u = (-half_b + sq) / a;
  // the far-sphere rule of fastg_sphere_hit, which holds with or without an accepted root (from_normalized, vec3.rs:219)
  const bool far = (r_l >= 1e-10 || r_u >= 1e-10) && c + s.r2 > 2.5e9 * s.r2;
  double t;
  if (1e-10 <= r_l && r_l <= tmax) t = r_l;
  else if (1e-10 <= r_u && r_u <= tmax) t = r_u;
  else return far ? OCC_UNCERTAIN : OCC_NONE;
  if (far || !occ_clear_of_tmax(t, tmax, 0.0, oimax)) return OCC_UNCERTAIN;
  return fast_hit_is_order_sensitive(oc, d, t, s.r2 * s.inv_r, half_b, sq, r_l, r_u, oimax) ? OCC_UNCERTAIN : OCC_CERTAIN;
}

// Plane::hit_ab + the interior tests (plane.rs:51-100, quad.rs:37-42, triangle.rs:60-95) for the root only: fastg_planar_hit's arithmetic
__device__ __forceinline__ int occ_planar_root(const DevPlanar &pl, D3 o, D3 d, float oimax, double tmax) {
  D3 normal = ld3(pl.normal);
  double denom = dot(normal, d);
  if (fabs(denom) < 1e-8) return OCC_NONE;
  double t = (pl.d - dot(normal, o)) / denom;
  if (!(1e-10 <= t && t <= tmax)) return OCC_NONE;
  const double band = fast_tie_band((fabs(pl.d) + fabs(normal.x * o.x) + fabs(normal.y * o.y) + fabs(normal.z * o.z)) / fabs(denom), oimax);
  D3 p = o + d * t;
  D3 hp = p - ld3(pl.q);
  D3 w = ld3(pl.w);
  double alpha = dot(w, cross(hp, ld3(pl.v)));
  double beta = dot(w, cross(ld3(pl.u), hp));
  const double w1 = fabs(w.x) + fabs(w.y) + fabs(w.z), d1 = fabs(d.x) + fabs(d.y) + fabs(d.z);
  const double uv1 = fmax(fabs(pl.u[0]) + fabs(pl.u[1]) + fabs(pl.u[2]), fabs(pl.v[0]) + fabs(pl.v[1]) + fabs(pl.v[2]));
  const double e = 1e-9 + band * d1 * w1 * uv1;
  bool inside, edge;
  if (pl.kind == RL_PLANAR_QUAD) {
    inside = 0.0 <= alpha && alpha <= 1.0 && 0.0 <= beta && beta <= 1.0;
    edge = fabs(alpha) <= e || fabs(alpha - 1.0) <= e || fabs(beta) <= e || fabs(beta - 1.0) <= e;
  } else if (pl.kind == RL_PLANAR_TRIANGLE) {
    inside = 0.0 <= alpha && 0.0 <= beta && alpha + beta <= 1.0;
    edge = fabs(alpha) <= e || fabs(beta) <= e || fabs(alpha + beta - 1.0) <= e;
  } else {
    inside = true, edge = false;
  }
  if (!inside) return OCC_NONE;
  return (edge || !occ_clear_of_tmax(t, tmax, band, oimax)) ? OCC_UNCERTAIN : OCC_CERTAIN;
}

// LDS: the per-lane stack [SD][NT] and the tree's top (P.fg_top nodes), as rtiow_hit_rays_fast_kernel.  stats[7] counts the re-traced rays.
template <int NT, int SD>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_occluded_rays_fast_kernel(RtiowParams P, OcclusionQuery Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  uint32_t *s_stack;
  uint4 *s_top;
  fastq_query_lds<NT, SD>(smem, P, tid, s_stack, s_top);
  const DevOp *ops = P.ops;
  const FastNodeQ *nodes = P.fg_nodes;
  const FastItem *items = P.fg_items;
  const uint32_t top = P.fg_top;
  const float FINF = __int_as_float(0x7F800000);
  const double tmax = Q.tmax;
  unsigned long long c_rays = 0, c_flag = 0, c_slow = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const rl_ray &ray = Q.rays[idx];
    const D3 wo = ld3(ray.origin), wd = ld3(ray.dir);
    const double time = ray.time;
    c_rays++;
    uint32_t sp = 0, steps = 0;
    const RayAux32 ra32 = ray_aux32_direct(wo, wd);
    bool amb, unsafe;
    bool unc = false, sure = false;  // an uncertain root was seen; a certain one ends the walk
    float grow;
    fastq_ray_start(P, wo, ra32, amb, unsafe, grow);
    const float c32 = unsafe ? FINF : (float)tmax;  // the pruning bound: the caller's tmax, first step to last
    // (loop head written out: as fastq_next_step() / fastq_first_entry(), 1,492 - 13,819 lines of every kernel that walks this tree flat changed)
    uint32_t seg = 0;
    uint32_t e = amb ? NONE : (P.fg_n_seg > 1u ? P.fg_seg_roots[0] : P.fg_root);
#pragma unroll 1
    for (;;) {
      while (e == NONE && !amb && seg + 1u < P.fg_n_seg) e = P.fg_seg_roots[++seg];
      if (e == NONE || amb) break;
      if (++steps > FASTG_STEP_BUDGET) {
        amb = true;
        break;
      }
      if (e & FASTG_LEAF) {
        const uint32_t item = e & ~FASTG_LEAF;
        const FastItem it = items[item];
        D3 o, d;
        replay_chain(P, ops, it.chain, wo, wd, o, d);
        const float oimax = fastq_leaf_oimax(ra32, it.chain, o, d);
        const int found = it.kind == 0 ? occ_sphere_root(P.fg_spheres[item], it.payload, o, d, time, oimax, tmax)
                                       : occ_planar_root(P.planars[it.payload], o, d, oimax, tmax);
        if (found == OCC_CERTAIN) {
          sure = true;
          break;
        }
        unc = unc || found == OCC_UNCERTAIN;
        e = fastq_pop<NT>(s_stack, tid, sp);
        continue;
      }
      // (a one-line lambda, not direct calls: called directly, fastq_missed changed 200 lines of this kernel)
      auto missed = [&](float b0, float b1, float b2, float b3, float b4, float b5, float &tmin) { return fastq_missed(ra32, grow, c32, b0, b1, b2, b3, b4, b5, tmin); };
      // (node fetch, child tests and child order written out: as functions over a node struct, 214 - 1,608 lines of the same kernels changed)
      const Float4 *nd = e < top ? (const Float4 *)(s_top + e * 8u) : (const Float4 *)(nodes + e);
      const Float4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5];
      const uint4 ch = *(const uint4 *)(nd + 6);
      float k0, k1, k2, k3;  // (the entry distances: not used, the children are visited in stored order)
      const bool h0 = !missed(lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, k0) && ch.x != NONE;
      const bool h1 = !missed(lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, k1) && ch.y != NONE;
      const bool h2 = !missed(lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, k2) && ch.z != NONE;
      const bool h3 = !missed(lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, k3) && ch.w != NONE;
      // children in STORED order, no sorting network: any certain hit ends the walk, so the order only decides how soon.  Measured against
      // nearest first on frame rays and shadow segments: 1.03 ... 5.6 times faster.  (Supposed reason: the node builder
      // opens the largest inner child and appends its halves, so a node's first slots keep its leaves — a ground sphere, a wall.)
      uint32_t first = NONE;
      auto visit = [&](bool h, uint32_t c) {
        if (!h) return;
        if (first != NONE) fastq_push<NT, SD>(s_stack, tid, sp, amb, first);
        first = c;
      };
      visit(h3, ch.w), visit(h2, ch.z), visit(h1, ch.y), visit(h0, ch.x);
      e = first != NONE ? first : fastq_pop<NT>(s_stack, tid, sp);
    }
    uint8_t occluded = sure ? (uint8_t)1 : (uint8_t)0;
    if (!sure && (amb || unc)) {  // the reference's own fold decides
      Rec rec = rec_none(tmax);
      GenCounters gc{0, 0, 0, 0, 0};
      auto draw = []() { return 0.0; };
      general_trace<false, false, false>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
      c_flag += gc.flagged;
      c_slow++;
      occluded = rec.any ? (uint8_t)1 : (uint8_t)0;
    }
    Q.occluded[idx] = occluded;
  }
  unsigned long long v;
  v = wave_sum(c_rays);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[0], v);
  v = wave_sum(c_flag);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[6], v);
  v = wave_sum(c_slow);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[7], v);
}

}  // namespace rl
