// The pieces of one ray's walk over the four-wide fast tree (FastNodeQ) that its bodies CALL.  The bodies:
//   rtiow_hit_rays_fast_kernel       rl_ray_query.h               closest hit, the caller's tmax
//   features_fast_trace              rl_rtiow_features.h          closest hit, tmax = +inf (feature, AO, direct and NEE kernels)
//   rtiow_occluded_rays_fast_kernel  rl_occlusion_query.h         any hit
//   ao_any_hit_walk                  rl_rtiow_ao.h                any hit (AO, direct and NEE kernels)
//   TRAV / LEAF / start_ray          rl_rtiow_fastgen_body.inc    closest hit, wave-scheduled (the cfg 4 / 5 renders)
// A piece is here only where every kernel that includes the calling body came out with the instructions it had with the text written
// out (§3.24's first tier; profiles/fast_walk_pieces.txt has the comparison): nothing here rests on a timing.  What failed that test
// stays written out in each body — the loop's head (stage advance, step budget), the node fetch with its four child tests, the two
// child orders, the winner's record — and so do the loop skeleton and the two result shapes: the WHOLE walk as one function failed it
// twice (§3.16, §3.20).  In the two query kernels and in the wave-scheduled body the calls stand inside one-line lambdas: called
// directly, the same functions gave those kernels other code (the note at each place has the lines).  rl_rtiow_fastgen.h includes this file.
#pragma once
#include "rl_rtiow_general.h"
#include "rl_rtiow_wave.h"

namespace rl {

// A fast walk that has taken this many steps (nodes + primitive tests) is given up: the ray is re-traced by the reference's own fold, which
// prunes by ITS boxes (cfg 5: ~140 tests).  The rays that get here are far-origin rays (`unsafe`: every box widened by `grow`, no pruning by
// the closest hit) whose widened boxes overlap half the scene — a handful per frame walk 1e5 ... 1e6 steps, 30 ... 460 ms EACH in a
// traversal-only launch, and the megakernel's last lanes were those too: cfg 5 at 64 spp 2.54 -> 1.87 s.  Any budget is correct (the fold
// is the reference); measured at 64 spp: 64 steps 3.56 s (16.7 M rays re-traced), 128: 2.20 s (5.1 M), 256: 1.89 s, 512: 1.87 s, 2048: 1.88 s
// (4.15 M: the rays that are re-traced for other reasons).
static const uint32_t FASTG_STEP_BUDGET = 512;

// Ray start: what ray_aux32_direct leaves to decide.  amb: the ray is outside the binary32 filter's range, the reference's order decides.
// unsafe: the origin is farther than r_safe from the scene's centre (e.g. inside a huge ground sphere).  The boxes' padding was sized
// for origins inside r_safe, so such a ray widens every box interval by `grow` and does NOT prune by the closest hit or the interval's
// end: pad(L) = fg_pad_k * L^2 in world units (rl_fast_bvh.cpp), L = distance to the centre + the scene's radius; in units of t: / min |d_k|.
// (start_ray of rl_rtiow_fastgen_body.inc keeps its own text of this: see there.)
__device__ __forceinline__ void fastq_ray_start(const RtiowParams &P, D3 wo, const RayAux32 &ra32, bool &amb, bool &unsafe, float &grow) {
  const float FINF = __int_as_float(0x7F800000);
  amb = !(ra32.slack < FINF);
  grow = 0.0f;
  const float fx = (float)wo.x - P.fg_center[0], fy = (float)wo.y - P.fg_center[1], fz = (float)wo.z - P.fg_center[2];
  const float far2 = fmaf(fx, fx, fmaf(fy, fy, fz * fz));
  unsafe = !(far2 <= P.fg_rsafe2);
  if (unsafe) {
    const float L = sqrtf(far2) + P.fg_radius;
    grow = P.fg_pad_k * L * L * fmaxf(fmaxf(fabsf(ra32.invx), fabsf(ra32.invy)), fabsf(ra32.invz));
    if (!(grow < FINF)) amb = true;
  }
}

// The per-lane stack in LDS, [entry][lane]: conflict-free.
template <int NT>
__device__ __forceinline__ uint32_t fastq_pop(const uint32_t *s_stack, int tid, uint32_t &sp) {
  if (sp == 0) return NONE;
  sp--;
  return s_stack[(size_t)sp * NT + tid];
}
template <int NT, int SD>
__device__ __forceinline__ void fastq_push(uint32_t *s_stack, int tid, uint32_t &sp, bool &amb, uint32_t e) {
  if (sp < (uint32_t)SD) s_stack[(size_t)sp * NT + tid] = e, sp++;
  else amb = true;  // more pending children than the stack holds: the reference's order decides
}

// The tie band's coordinate scale max |o_k / d_k| of the ray a leaf's test actually sees: the world ray's, or that of the ray taken
// through the item's PUSH chain (binary32 is plenty for a tolerance).  NaN (0 * inf) -> +inf: every hit of this item counts as a tie.
__device__ __forceinline__ float fastq_leaf_oimax(const RayAux32 &ra32, uint32_t chain, D3 o, D3 d) {
  const float FINF = __int_as_float(0x7F800000);
  float oimax = ra32.oimax();
  if (chain != NONE)
    oimax = fmaxf(fmaxf(fabsf((float)o.x * __builtin_amdgcn_rcpf((float)d.x)), fabsf((float)o.y * __builtin_amdgcn_rcpf((float)d.y))),
                  fabsf((float)o.z * __builtin_amdgcn_rcpf((float)d.z)));
  if (!(oimax < FINF)) oimax = FINF;
  return oimax;
}

// The reject-only box test of one child, {x.min, x.max, y.min, y.max, z.min, z.max}: true when the ray certainly misses the box inside
// [1e-10, c32] (fast_miss_thresh, rl_rtiow_wave.h: the one statement of the threshold); false also for NaN arithmetic: visit.
// tmin: the entry distance.
__device__ __forceinline__ bool fastq_missed(const RayAux32 &ra32, float grow, float c32, float b0, float b1, float b2, float b3, float b4, float b5, float &tmin) {
  float t0x = fmaf(b0, ra32.invx, -ra32.oix), t1x = fmaf(b1, ra32.invx, -ra32.oix);
  float t0y = fmaf(b2, ra32.invy, -ra32.oiy), t1y = fmaf(b3, ra32.invy, -ra32.oiy);
  float t0z = fmaf(b4, ra32.invz, -ra32.oiz), t1z = fmaf(b5, ra32.invz, -ra32.oiz);
  tmin = fmaxf(fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z)) - grow, 1e-10f);
  float tmax = fminf(fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z)) + grow, c32);
  float diff = tmax - tmin;
  return diff < -fast_miss_thresh(ra32, tmin, tmax);
}

// The dynamic LDS of a query kernel: the per-lane stack and, behind it, the tree's top staged by the whole workgroup.  Every thread of
// the block calls this once, before anything else (pixel_lds, rl_rtiow_pixel_skeleton.h, does the same behind the pixel renders' RNG ring).
template <int NT, int SD>
__device__ __forceinline__ void fastq_query_lds(unsigned char *smem, const RtiowParams &P, int tid, uint32_t *&s_stack, uint4 *&s_top) {
  s_stack = (uint32_t *)smem;                                    // [SD][NT]
  s_top = (uint4 *)(smem + (size_t)NT * SD * sizeof(uint32_t));  // [fg_top] FastNodeQ
  if (P.fg_top) {
    for (uint32_t i = (uint32_t)tid; i < P.fg_top * 8u; i += (uint32_t)NT) s_top[i] = ((const uint4 *)P.fg_nodes)[i];
    __syncthreads();
  }
}

}  // namespace rl
