// RTIOW all-primitives kernel with the FAST traversal (counter-free renders only): the wave-scheduled state machine of
// rl_rtiow_wave_general.h walking the world-space surface-area-heuristic tree of rl_fast_bvh.cpp (build_fast_general) instead of the
// reference's threaded program.
//
//   TRAV  one 64-byte node from HBM / L2 / Infinity Cache = both children's binary32 boxes: reject-only tests (rl_rtiow_wave.h
//         ray_aux32_direct), nearer child first, the farther one pushed on a per-lane stack in LDS ([entry][lane]: conflict-free)
//   LEAF  one primitive OCCURRENCE: the world ray is taken through the occurrence's PUSH chain (transform.rs:145-149, translate.rs:15)
//         and the reference's Sphere::hit / Plane::hit_ab arithmetic yields the root only — no HitRecord is kept while traversing
//   SHADE the winning occurrence is evaluated once more with ray_t.max = its root (same arithmetic, same root) for the full
//         HitRecord, which then takes the POP chain (transform.rs:152-161) — or, for an order-sensitive ray, the whole ray is re-traced by
//         general_slow_trace, the reference's own fold — and is shaded as in rl_rtiow_wave_general.h
// No XF state, no HitRecord and no second ray live across states: 2 instead of 6 wave states touch the scene.
// Order-sensitive rays (rl_fast_bvh.cpp): two roots within fast_tie_band of each other, grazing sphere hits, planar hits within 1e-9 of an edge,
// rays outside the binary32 filter's range or whose origin is farther than r_safe from the scene's centre, stack overflow.
#pragma once
#include "rl_rtiow_fast_walk.h"  // FASTG_STEP_BUDGET and the pieces of the walk that its five bodies call
#include "rl_rtiow_general.h"
#include "rl_rtiow_wave.h"

namespace rl {

// The reference's fold over its own program (bvh.rs:79-95, hittable/mod.rs:88-111, transform.rs:143-164), exact divisions; returns the
// HitRecord in world space and the number of panic sites reached.
template <bool TRANS>
__device__ __forceinline__ uint32_t general_slow_trace(const RtiowParams &P, const DevOp *ops, D3 wo, D3 wd, double time, Rec &rec) {
  uint32_t flags = 0;
  D3 o = wo, d = wd;
  uint32_t pc = 0;
#pragma unroll 1
  for (;;) {
    const DevOp &op = ops[pc];
    uint32_t code = op.code & 0xFFu;
    if (code == OP_END) break;
    if (code == OP_BOX || code == OP_BOX_SPH || code == OP_BOX_PLANAR) {
      double bx[6] = {op.box[0], op.box[1], op.box[2], op.box[3], op.box[4], op.box[5]};
      if (!aabb_hit(bx, o, d, 1e-10, rec.t)) {
        pc = op.skip;
        continue;
      }
      if (code == OP_BOX) {
        pc++;
        continue;
      }
    }
    if (code == OP_BOX_SPH || code == OP_SPHERE) {
#pragma unroll 1
      for (int k = 0; k < 2; k++) {
        uint32_t pl = k == 0 ? op.a : op.b;
        if (pl == NONE || (k == 1 && code == OP_SPHERE)) continue;
        uint32_t si = pl & SPH_INDEX;
        if (sphere_hit_rec(P.spheres[si], pl, P.sphere_material[si], pc, o, d, time, rec)) flags++;
      }
      pc = code == OP_SPHERE ? pc + 1 : op.skip;
      continue;
    }
    if (code == OP_BOX_PLANAR || code == OP_PLANAR) {
#pragma unroll 1
      for (int k = 0; k < 2; k++) {
        uint32_t pl = k == 0 ? op.a : op.b;
        if (pl == NONE || (k == 1 && code == OP_PLANAR)) continue;
        if (planar_hit_rec(P.planars[pl], pc, o, d, rec)) flags++;
      }
      pc = code == OP_PLANAR ? pc + 1 : op.skip;
      continue;
    }
    if (code == OP_PUSH_TRANSLATE) o = o - ld3(P.translates[op.a].offset);
    else if (code == OP_PUSH_TRANSFORM) {
      const rl_transform &t = P.transforms[op.a];
      D3 no = mat3_mul(t.inv, o), nd = mat3_mul(t.inv, d);
      o = no, d = nd;
    } else {  // POP: op.b = the matching PUSH, whose .b is the parent PUSH
      uint32_t push_pc = op.b;
      if (rec.any && rec.pc > push_pc) {
        if (code == OP_POP_TRANSLATE) rec.p = rec.p + ld3(P.translates[op.a].offset);
        else {
          const rl_transform &t = P.transforms[op.a];
          rec.p = mat3_mul(t.m, rec.p);
          D3 wn = mat3_mul(t.inv_t, rec.normal);
          double m = len2(wn);
          if (approx_eq_eps(m, 0.0, 1e-16)) flags++;
          else rec.normal = normalize(wn);
        }
      }
      replay_chain(P, ops, ops[push_pc].b, wo, wd, o, d);
    }
    pc++;
  }
  return flags;
}

#ifdef RL_FASTG_VERIFY  // debug build (tools/verify_fastg.py): every ray is ALSO traced in the reference's order; mismatches are logged
// (g_vcount / g_vlog / g_vstats: rl_rtiow_wave.h — the sphere kernels log into them too)
#endif
// Sphere::hit / Plane::hit_ab for the ROOT only, acceptance window widened by the tie band (see fast_sphere_hit in rl_rtiow_wave.h)
__device__ __forceinline__ void fastg_planar_hit(const DevPlanar &pl, D3 o, D3 d, float oimax, uint32_t item, double &closest, uint32_t &best, bool &amb) {
  D3 normal = ld3(pl.normal);
  double denom = dot(normal, d);
  if (fabs(denom) < 1e-8) return;
  double t = (pl.d - dot(normal, o)) / denom;
  // t's rounding error scales with the cancelling terms of its numerator, not with t
  const double band = fast_tie_band((fabs(pl.d) + fabs(normal.x * o.x) + fabs(normal.y * o.y) + fabs(normal.z * o.z)) / fabs(denom), oimax);
  if (!(1e-10 <= t && t <= closest + band)) return;
  D3 p = o + d * t;
  D3 hp = p - ld3(pl.q);
  D3 w = ld3(pl.w);
  double alpha = dot(w, cross(hp, ld3(pl.v)));
  double beta = dot(w, cross(ld3(pl.u), hp));
  // within the hit point's own uncertainty (root error x |d|, seen through alpha = w . (hp x v), beta = w . (u x hp)) of an edge: the
  // reference's leaf box is the exact bound of the vertices, so such a hit may or may not pass it
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
  } else {  // an unbounded Plane (a stage of its own: FastGeneral::stage_roots): plane.rs:51-100 has no interior test, and no box anywhere
    inside = true, edge = false;
  }
  if (!inside) return;
  if (edge) amb = true;  // an edge-grazing hit may or may not pass the reference's own leaf box (the exact bound of the vertices)
  if (best != NONE && fabs(t - closest) <= band) amb = true;
  if (t <= closest) closest = t, best = item;
}

__device__ __forceinline__ void fastg_sphere_hit(const DevSphere &s, uint32_t payload, D3 o, D3 d, double time, float oimax, uint32_t item, double &closest,
                                                 uint32_t &best, bool &amb) {
  D3 c0 = ld3(s.c0);
  D3 center = (payload & SPH_MOVING) ? c0 + ld3(s.dc) * time : c0;
  D3 oc = o - center;
  double a = len2(d);
  double half_b = dot(oc, d);
  double c = len2(oc) - s.r2;
  double disc = half_b * half_b - a * c;
  if (disc < 0.0) return;
  double sq = sqrt(disc);
  double r_l = (-half_b - sq) / a;
  double r_u = (-half_b + sq) / a;
  // a sphere seen from more than ~5e4 radii away: the reference's from_normalized assert (vec3.rs:219) can fire for it, and whether
  // it is accepted along the way depends on the reference's order (rays from inside r_safe never get here: build_fast_general)
  if ((r_l >= 1e-10 || r_u >= 1e-10) && c + s.r2 > 2.5e9 * s.r2) amb = true;
  const double band = fast_tie_band(fabs(r_l) + fabs(r_u), oimax);
  const double hi = closest + band;
  double t;
  if (1e-10 <= r_l && r_l <= hi) t = r_l;
  else if (1e-10 <= r_u && r_u <= hi) t = r_u;
  else return;
  if (best != NONE && fabs(t - closest) <= band) amb = true;  // grazing / pole hits: only the winner matters, checked in SHADE
  if (t <= closest) closest = t, best = item;
}

// SD = entries of the per-lane LDS stack (a deeper pending list re-traces the ray in the reference's order: the tree may be 40 deep,
// the list of pending far children hardly ever is)
// Nodes are four wide (FastNodeQ, 128 B = one L2 line: one dependent fetch per two levels of the surface-area-heuristic binary tree,
// children visited nearest first).  Measured against the two-wide pair nodes they replaced: cfg 4 +1.3 %, cfg 5 (150 MB of nodes, items
// and spheres behind 4 MB of L2 per XCD) +6 ... 8 %.  Also measured, and dropped: a 10-bit lower bound of the entry distance in every stack
// entry, so that pop() can skip entries that have fallen behind the closest hit (cfg 4 -10 %, cfg 5 -6 %: the skipped visits are worth less
// than the dependent LDS round trips of the skipping loop).
// MEDIA (round 3): scenes with ConstantMedium objects (constant_medium.rs:27-80, deterministic variant: include/rl_render.h rl_medium).  The
// reference evaluates a medium where its fold reaches it, with ray_t.max = the closest hit found by everything BEFORE it in the program,
// and draws the free path from the RNG only if the ray's stretch inside the boundary, clamped to that closest hit, is non-empty.  So the
// items are cut into segments at the media (FastGeneral::seg_roots): a ray walks segment 0's tree, evaluates medium 0 with the closest hit
// so far (the boundary by the reference's own fold over its ops, twice; the draw from the pixel's ChaCha8 ring), walks segment 1's tree
// with the same running closest hit, ... — exactly the reference's order at the granularity that matters.  (BVH boxes around a medium
// never decide whether it draws: a ray that misses a box inside [t_min, closest] has an empty stretch inside the boundary, too.)  An
// order-sensitive ray rewinds the ring to the word position the ray started at and is re-traced by the reference's fold WITH its media.
// INDEP: the sample-parallel mode, as in rtiow_wave_indep_kernel (rl_rtiow_wave.h; the body is included into both kernels for the same reason)
template <int NT, int SD, bool TRANS, bool MEDIA = false>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_fast_general_kernel(const RtiowParams *__restrict__ Pp) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_fastgen_body.inc"
}
template <int NT, int SD, bool TRANS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_fast_general_indep_kernel(const RtiowParams *__restrict__ Pp) {
  constexpr bool INDEP = true, RAYS = false, PIXELS = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_fastgen_body.inc"
}
// RAYS (rl_rtiow_ray_color_rays*): Camera::ray_color for a buffer of rays, each with its own RNG cursor.  GEN claims rays
// instead of pixels and starts them as given (no get_ray); everything behind GEN — regeneration, FILL, TRAV, LEAF, SHADE, the far-origin
// treatment of start_ray, the exact re-trace — is the body's own.  P.cam carries the call's background and max_depth, P.key its seed.
template <int NT, int SD, bool TRANS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_fast_general_rays_kernel(const RtiowParams *__restrict__ Pp) {
  constexpr bool INDEP = false, RAYS = true, PIXELS = false, MOMENTS = never_v<NT>;
#include "rl_rtiow_fastgen_body.inc"
}
// PIXELS (rl_rtiow_render_pixels*): GEN claims elements of the caller's (x, y) list instead of tile slots and stores a pixel's
// sums at its element index; everything behind the claim is the body's own, so a listed pixel is the frame's pixel bit for bit.
template <int NT, int SD, bool TRANS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_fast_general_pixels_kernel(const RtiowParams *__restrict__ Pp) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = true, MOMENTS = never_v<NT>;
#include "rl_rtiow_fastgen_body.inc"
}
// MOMENTS (rl_rtiow_render_moments* / rl_rtiow_render_pixels_moments*): the frame and the list kernel once more, keeping the
// sum of the squared sample colours (P.out_sq) beside the sum — stored, resumed and zeroed wherever the sum is.  With P.out_count set
// (rl_rtiow_render_adaptive*) a pixel of the frame kernel also ends at the first checkpoint rtiow_adaptive_stop accepts.
template <int NT, int SD, bool TRANS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_fast_general_moments_kernel(const RtiowParams *__restrict__ Pp) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = false, MOMENTS = true;
#include "rl_rtiow_fastgen_body.inc"
}
template <int NT, int SD, bool TRANS, bool MEDIA>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_fast_general_pixels_moments_kernel(const RtiowParams *__restrict__ Pp) {
  constexpr bool INDEP = false, RAYS = false, PIXELS = true, MOMENTS = true;
#include "rl_rtiow_fastgen_body.inc"
}

}  // namespace rl
