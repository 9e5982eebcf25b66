// Batched ray queries (include/rl_render.h rl_*_rays*): the kernels whose input is a buffer of rays instead of a camera.
//
//   rtiow_hit_rays_kernel      Hittable::hit(&Ray, &Interval) on the scene root (hittable/mod.rs:42, the fold of :88-111, bvh.rs:79-95):
//                              general_trace, the reference-order fold the counting renders use, with the caller's interval.
//   rtiow_hit_rays_seeded_kernel  the same fold with ConstantMedium objects evaluated: every ray carries an rl_rng_cursor to draw from
//   rtiow_hit_rays_fast_kernel counter-free queries with tmin == 1e-10 on scenes that have a fast tree: the four-wide SAH walk of
//                              rl_rtiow_fastgen.h as a flat per-lane loop; order-sensitive rays are re-traced by general_trace.
//   rtc_intersect_rays_kernel  World::intersect (world.rs:46-55) + hit (intersect.rs:159-168): rtc_intersect_all.
//   rtc_color_at_rays_kernel   World::color_at (world.rs:100): the per-ray body of rtc_full_kernel (rl_rtc_color_at_body.inc).
//
// One ray per lane, grid-stride over the batch; the grid is what is resident at once (occupancy API).  Rays are used as given (no
// normalisation: the reference does none).  Records are written with plain per-lane stores (88 / 40 / 24 B).
#pragma once
#include "rl_rtc_full_kernel.h"
#include "rl_rtiow_fastgen.h"
#include "rl_rtiow_general.h"

namespace rl {

struct RayQuery {
  const rl_ray *rays;
  unsigned long long n;
  double tmin, tmax;         // RTIOW: the Interval
  rl_rtiow_hit *hits;        // RTIOW
  rl_rtc_isect *isects;      // RTC intersect: [n][k] (null: counts only)
  uint32_t *counts;          // RTC intersect: [n]
  uint32_t *hit_index;       // RTC intersect: [n] (null: not wanted)
  uint32_t k;
  double *rgb;               // RTC color_at: [n][3]
};

__device__ __forceinline__ void hit_record_store(rl_rtiow_hit *dst, const Rec &rec) {
  double *out = (double *)dst;
  uint32_t *outw = (uint32_t *)(out + 9);
  if (rec.any) {
    double u, v;
    rec_uv(rec, u, v);
    out[0] = rec.t, out[1] = rec.p.x, out[2] = rec.p.y, out[3] = rec.p.z;
    out[4] = rec.normal.x, out[5] = rec.normal.y, out[6] = rec.normal.z, out[7] = u, out[8] = v;
    outw[0] = 1u, outw[1] = rec.front ? 1u : 0u, outw[2] = rec.mat, outw[3] = 0u;
  } else {
    out[0] = __longlong_as_double(0x7FF0000000000000ll);
#pragma unroll
    for (int i = 1; i < 9; i++) out[i] = 0.0;
    outw[0] = 0u, outw[1] = 0u, outw[2] = 0u, outw[3] = 0u;
  }
}

template <int NT, bool STATS>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_hit_rays_kernel(RtiowParams P, RayQuery Q) {
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
    auto draw = []() { return 0.0; };  // media are rejected on the host (a bare ray has no RNG stream to draw from)
    general_trace<STATS, false, true>(P, ops, 0u, NONE, o, d, o, d, time, Q.tmin, rec, gc, draw);
    c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
    hit_record_store(&Q.hits[idx], rec);
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

// Hittable::hit for rays that carry an RNG cursor (rl_rtiow_hit_rays_seeded*, scenes with ConstantMedium objects): the fold of
// rtiow_hit_rays_kernel with MEDIA = true, the free path of every medium the fold evaluates drawn from the ray's own cursor.  The lane's
// ChaCha8 blocks live in a Ring column (ODD: a cursor may stand at any word) and are generated at the ray's FIRST draw: a ray whose fold
// reaches no medium with rec1.t < rec2.t costs no block and returns its cursor as it came.  draw() runs in divergent control flow (only
// some lanes are inside a boundary); the ring's refill is per lane — its own LDS column, no cross-lane step — so that is safe.
// stats[5] += the words consumed (position difference), counting or not.
struct SeededHitQuery {
  const rl_ray *rays;
  const rl_rng_cursor *cursors;
  unsigned long long n;
  double tmin, tmax;
  rl_rtiow_hit *hits;
  rl_rng_cursor *out_cursors;  // null: not wanted (may be `cursors`: a lane reads its element's cursor before it writes it)
};
template <int NT, bool STATS>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_hit_rays_seeded_kernel(RtiowParams P, SeededHitQuery Q) {
  __shared__ unsigned long long s_rng[16 * NT];
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  Ring<NT, true, true> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  unsigned long long c_rays = 0, c_nodes = 0, c_sph = 0, c_pl = 0, c_inst = 0, c_flag = 0, c_words = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const uint64_t *cur = (const uint64_t *)(Q.cursors + idx);
    const uint64_t stream = cur[0], word_pos = cur[1];
    const rl_ray &ray = Q.rays[idx];
    const D3 o = ld3(ray.origin), d = ld3(ray.dir);
    const double time = ray.time;
    c_rays++;
    rng.stream = stream, rng.pos = (uint32_t)word_pos, rng.nres = 0;
    Rec rec = rec_none(Q.tmax);
    GenCounters gc{0, 0, 0, 0, 0};
    auto draw = [&]() {
      if (rng.nres == 0u) rng.reset_stream(stream);  // the ray's first draw: blocks pos / 16 and the next one
      return rng.gen_f64();
    };
    general_trace<STATS, true, true>(P, ops, 0u, NONE, o, d, o, d, time, Q.tmin, rec, gc, draw);
    c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
    c_words += rng.pos - (uint32_t)word_pos;
    hit_record_store(&Q.hits[idx], rec);
    if (Q.out_cursors) {
      uint64_t *oc = (uint64_t *)(Q.out_cursors + idx);
      oc[0] = stream, oc[1] = (uint64_t)rng.pos;
    }
  }
  unsigned long long v;
  v = wave_sum(c_rays);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[0], v);
  v = wave_sum(c_words);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[5], v);
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

// The fast walk (rl_rtiow_fastgen.h TRAV / LEAF / SHADE) for a caller's ray, one ray per lane from start to end: no RNG rings, so LDS
// holds the per-lane stack [SD][NT] and the tree's top (P.fg_top nodes).  `closest` starts at Q.tmax.  Re-traced in the reference's
// order (general_trace with ALL_UV, the very function of rtiow_hit_rays_kernel, so the record is the same bits): rays outside the binary32
// filter's range, ties (fast_tie_band), grazing / edge hits, far origins, stack overflow, the step budget — and a winner within the tie
// band of a finite tmax.  The render's "skip the scattered ray's own sphere" shortcut is NOT applied: a caller's ray does not say
// where it came from.  stats[7] counts the re-traced rays.
// The LDS carve with the tree-top staging, the ray start, the per-lane stack, the leaf's oimax and the box test are rl_rtiow_fast_walk.h's,
// shared with the other four bodies that walk this tree; the rest of the walk is this kernel's own text, and
// features_fast_trace (rl_rtiow_features.h) holds the other copy of the closest-hit form.
template <int NT, int SD>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtiow_hit_rays_fast_kernel(RtiowParams P, RayQuery Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  uint32_t *s_stack;
  uint4 *s_top;
  fastq_query_lds<NT, SD>(smem, P, tid, s_stack, s_top);
  const DevOp *ops = P.ops;
  const FastNodeQ *nodes = P.fg_nodes;
  const FastItem *items = P.fg_items;
  const uint32_t top = P.fg_top;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const float FINF = __int_as_float(0x7F800000);
  unsigned long long c_rays = 0, c_flag = 0, c_slow = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const rl_ray &ray = Q.rays[idx];
    const D3 wo = ld3(ray.origin), wd = ld3(ray.dir);
    const double time = ray.time;
    c_rays++;
    double closest = Q.tmax;
    uint32_t best = NONE, sp = 0, steps = 0;
    const RayAux32 ra32 = ray_aux32_direct(wo, wd);
    bool amb, unsafe;
    float grow;
    fastq_ray_start(P, wo, ra32, amb, unsafe, grow);
    // (one-line lambdas, not direct calls: called directly, fastq_missed changed 1 line of this kernel, fastq_pop / fastq_push 55)
    auto pop = [&]() -> uint32_t { return fastq_pop<NT>(s_stack, tid, sp); };
    auto push = [&](uint32_t e) { fastq_push<NT, SD>(s_stack, tid, sp, amb, e); };
    // several stages (a scene's unbounded Planes are leaf stages of their own, FastGeneral::stage_roots): walked one after the other
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
        const DevSphere isph = P.fg_spheres[item];
        D3 o, d;
        replay_chain(P, ops, it.chain, wo, wd, o, d);
        const float oimax = fastq_leaf_oimax(ra32, it.chain, o, d);
        if (it.kind == 0) fastg_sphere_hit(isph, it.payload, o, d, time, oimax, item, closest, best, amb);
        else fastg_planar_hit(P.planars[it.payload], o, d, oimax, item, closest, best, amb);
        e = pop();
        continue;
      }
      const float c32 = unsafe ? FINF : (float)closest;
      auto missed = [&](float b0, float b1, float b2, float b3, float b4, float b5, float &tmin) { return fastq_missed(ra32, grow, c32, b0, b1, b2, b3, b4, b5, tmin); };
      // (node fetch, child tests and child order written out: as functions over a node struct, 214 - 1,608 lines of the same kernels changed)
      const Float4 *nd = e < top ? (const Float4 *)(s_top + e * 8u) : (const Float4 *)(nodes + e);
      const Float4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5];
      const uint4 ch = *(const uint4 *)(nd + 6);
      float k0, k1, k2, k3;
      const bool h0 = !missed(lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, k0) && ch.x != NONE;
      const bool h1 = !missed(lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, k1) && ch.y != NONE;
      const bool h2 = !missed(lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, k2) && ch.z != NONE;
      const bool h3 = !missed(lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, k3) && ch.w != NONE;
      const int nh = (int)h0 + (int)h1 + (int)h2 + (int)h3;
      k0 = h0 ? k0 : FINF, k1 = h1 ? k1 : FINF, k2 = h2 ? k2 : FINF, k3 = h3 ? k3 : FINF;
      uint32_t c0 = ch.x, c1 = ch.y, c2 = ch.z, c3 = ch.w;
      uint32_t u0 = (__float_as_uint(k0) & ~1u) | (h0 ? 0u : 1u), u1 = (__float_as_uint(k1) & ~1u) | (h1 ? 0u : 1u);
      uint32_t u2 = (__float_as_uint(k2) & ~1u) | (h2 ? 0u : 1u), u3 = (__float_as_uint(k3) & ~1u) | (h3 ? 0u : 1u);
      auto cex = [&](uint32_t &ka, uint32_t &kb, uint32_t &ca, uint32_t &cb) {  // keys are non-negative floats: integer order = float order
        const bool sw = kb < ka;
        const uint32_t tk = sw ? kb : ka, tc = sw ? cb : ca;
        kb = sw ? ka : kb, cb = sw ? ca : cb;
        ka = tk, ca = tc;
      };
      cex(u0, u1, c0, c1), cex(u2, u3, c2, c3), cex(u0, u2, c0, c2), cex(u1, u3, c1, c3), cex(u1, u2, c1, c2);
      if (nh >= 4) push(c3);
      if (nh >= 3) push(c2);
      if (nh >= 2) push(c1);
      e = nh ? c0 : pop();
    }
    Rec rec = rec_none(Q.tmax);
    uint32_t hit_flags = 0;
    // the winner's HitRecord: the same test once more with ray_t.max = its root, then the POP chain
    // (written out: as one function with features_fast_trace's, tmax passed in, 276 lines of this kernel and 2 - 14 of the pixel renders changed)
    if (!amb && best != NONE) {
      const FastItem it = items[best];
      const DevSphere sph = P.fg_spheres[best];
      const uint32_t wmat = P.fg_material[best];
      D3 o, d;
      replay_chain(P, ops, it.chain, wo, wd, o, d);
      const float oimax = fastq_leaf_oimax(ra32, it.chain, o, d);
      // a finite tmax: a winner within the tie band of it may be one the reference's boxes, cut at tmax, never let it reach
      if (Q.tmax < INF && !(fabs(closest - Q.tmax) > fast_tie_band(fabs(closest) + fabs(Q.tmax), oimax))) amb = true;
      rec.t = closest;
      if (!amb && it.kind == 0) {
        if (sphere_hit_rec(sph, it.payload | SPH_UV, wmat, it.op_pc, o, d, time, rec)) hit_flags++;
        D3 c0 = ld3(sph.c0);
        D3 center = (it.payload & SPH_MOVING) ? c0 + ld3(sph.dc) * time : c0;
        D3 oc = o - center;
        double half_b = dot(oc, d), sq = sph.r2 * sph.inv_r * fabs(dot(d, rec.normal)), a = len2(d);
        double other = 2.0 * sq * (double)__builtin_amdgcn_rcpf((float)a);
        if (fast_hit_is_order_sensitive(oc, d, closest, sph.r2 * sph.inv_r, half_b, sq, closest, fabs(closest) + other, oimax)) amb = true;
      } else if (!amb) {
        if (planar_hit_rec(P.planars[it.payload], it.op_pc, o, d, rec)) hit_flags++;
      }
      if (!amb && !rec.any) amb = true;  // (cannot happen: the same arithmetic found this root)
      hit_flags += pop_rec_chain(P, ops, amb ? NONE : it.chain, rec);
    }
    if (amb) {  // the reference's own fold decides
      rec = rec_none(Q.tmax);
      GenCounters gc{0, 0, 0, 0, 0};
      auto draw = []() { return 0.0; };
      general_trace<false, false, true>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
      c_flag += gc.flagged;
      c_slow++;
    } else c_flag += hit_flags;
    hit_record_store(&Q.hits[idx], rec);
  }
  unsigned long long v;
  v = wave_sum(c_rays);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[0], v);
  v = wave_sum(c_flag);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[6], v);
  v = wave_sum(c_slow);
  if ((tid & 63) == 0 && v) atomicAdd(&P.stats[7], v);
}

// A ray with more than RL_RTC_K intersections is flagged, as in the renders; its count is then RL_RTC_K.
template <int NT, int REGS_FOR>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(REGS_FOR) rtc_intersect_rays_kernel(RtcFullParams F, RayQuery Q) {
  const RtcParams &P = F.R;
  const int tid = threadIdx.x;
  RtcFullCounters cnt{0, 0, 0, 0, 0, 0};
  Ent list[RL_RTC_K];
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const rl_ray &ray = Q.rays[idx];
    cnt.rays++;
    uint32_t n = rtc_intersect_all(F, P.ops, P.tris, ld3(ray.origin), ld3(ray.dir), list, cnt, 1ull);
    int hi = rtc_first_hit(list, n);
    Q.counts[idx] = n;
    if (Q.hit_index) Q.hit_index[idx] = hi < 0 ? NONE : (uint32_t)hi;
    if (Q.isects) {
      const uint32_t m = n < Q.k ? n : Q.k;
      rl_rtc_isect *out = Q.isects + idx * Q.k;
      for (uint32_t i = 0; i < m; i++) {
        out[i].t = list[i].t;
        out[i].normal[0] = list[i].normal.x, out[i].normal[1] = list[i].normal.y, out[i].normal[2] = list[i].normal.z;
        out[i].object = list[i].leaf, out[i]._pad = 0u;
      }
    }
  }
  rtc_query_flush(cnt, P.stats, tid);
}

template <int NT, int REGS_FOR>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(REGS_FOR) rtc_color_at_rays_kernel(RtcFullParams F, RayQuery Q) {
  const RtcParams &P = F.R;
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  const DevTri *tris = P.tris;
  RtcFullCounters cnt{0, 0, 0, 0, 0, 0};
  Ent list[RL_RTC_K];
  Pending stack[RTC_MAX_PENDING];
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const rl_ray &ray = Q.rays[idx];
    const D3 origin = ld3(ray.origin), dir = ld3(ray.dir);
#include "rl_rtc_color_at_body.inc"  // D3 c = color_at(origin, dir)
    double *outp = Q.rgb + idx * 3;
    outp[0] = c.x, outp[1] = c.y, outp[2] = c.z;
  }
  rtc_query_flush(cnt, P.stats, tid);
}

// Camera::get_ray (camera.rs:203-216) for a buffer of (x, y, cursor): GEN's camera arithmetic of the render kernels, expression for
// expression, with the draws taken from the ray's own cursor.  One lane per ray, grid-stride; the lane's ChaCha8 blocks live in a Ring
// column (ODD: a cursor may stand at any word).  Not a hot path: a few draws per ray.
struct CameraRaysQuery {
  rl_rtiow_camera cam;
  uint32_t key[8];
  const uint32_t *px, *py;
  const rl_rng_cursor *cursors;
  rl_ray *rays;
  rl_rng_cursor *out_cursors;
  unsigned long long n;
};
template <int NT>
__global__ void __launch_bounds__(NT) rtiow_camera_rays_kernel(CameraRaysQuery Q) {
  __shared__ unsigned long long s_rng[16 * NT];
  const int tid = threadIdx.x;
  const rl_rtiow_camera &cam = Q.cam;
  Ring<NT, true, true> rng{Q.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const uint64_t *cur = (const uint64_t *)(Q.cursors + idx);
    const uint32_t px = Q.px[idx], y = Q.py[idx];
    rng.pos = (uint32_t)cur[1], rng.nres = 0;
    rng.reset_stream(cur[0]);
    D3 p00 = ld3(cam.pixel_00), du = ld3(cam.pixel_du), dv = ld3(cam.pixel_dv);
    D3 pixel_center = (p00 + du * (double)px) + dv * (double)y;
    double sx = -0.5 + rng.gen_f64();
    double sy = -0.5 + rng.gen_f64();
    D3 pixel_sample = pixel_center + (du * sx + dv * sy);
    D3 wo;
    if (cam.defocus_angle <= 0.0) wo = ld3(cam.lookfrom);
    else {
      double a, b;
      rng.unit_disc(a, b);
      wo = (ld3(cam.lookfrom) + ld3(cam.defocus_disk_u) * a) + ld3(cam.defocus_disk_v) * b;
    }
    const D3 wd = pixel_sample - wo;
    const double time = rng.gen_f64();
    double *r = (double *)(Q.rays + idx);
    r[0] = wo.x, r[1] = wo.y, r[2] = wo.z, r[3] = wd.x, r[4] = wd.y, r[5] = wd.z, r[6] = time;
    uint64_t *oc = (uint64_t *)(Q.out_cursors + idx);
    oc[0] = rng.stream, oc[1] = (uint64_t)rng.pos;
  }
}

}  // namespace rl
