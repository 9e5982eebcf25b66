// Feature renders (include/rl_render.h "Feature renders", rl_rtiow_render_features*): per pixel the sums over S jittered
// camera rays of the first hit's colour factor, normal and depth, and the number of rays that hit — the guide buffers of a denoiser.
//
//   rtiow_features_kernel<NT, STATS, FAST, SD>   one pixel per lane, grid-stride over the frame's or the list's slots; a per-lane loop over
//                                                the samples F .. F + S - 1 in ascending order, every add rounded on its own.
//
// Per sample the kernel joins three texts the library already has, expression for expression, so that the host composition of
// rl_rtiow_camera_rays, rl_rtiow_hit_rays_seeded and rl_rtiow_texture_values gives the same bits (tests/test_gpu_render_features.py):
//   1. the stream start and the camera arithmetic of rtiow_camera_rays_kernel (rl_ray_query.h): Ring in an LDS column, reset_stream at word 0
//   2. the closest-hit trace
//        FAST = false  general_trace<STATS, true, true>, media drawing from the sample's ring (rtiow_hit_rays_seeded_kernel)
//        FAST = true   the flat four-wide SAH walk of rtiow_hit_rays_fast_kernel with tmax = +inf: LDS stack, tree top in LDS, every
//                      order-sensitive ray re-traced by general_trace — the same record, bit for bit
//   3. rec_uv + material_texture / texture_value<2> as rtiow_scatter_rays_kernel (rl_material_query.h) calls them
// The walk of FAST (features_fast_trace below) and rtiow_hit_rays_fast_kernel's are two bodies, not one function: factored into one for
// both, the query kernel came out at 274 VGPRs + 18 AGPRs instead of 247.  What the two CALL, with the other bodies
// that walk this tree, is in rl_rtiow_fast_walk.h: the ray start, the per-lane stack, the leaf's oimax and the box
// test with the filter's threshold.  What remains a copy here: the loop skeleton with its head, the node fetch with the four child
// tests, the nearest-first order and the winner's record (without the finite-tmax tie test: tmax is +inf here) — each failed §3.26's
// rule as a function and says so at its place.  A change to one of those belongs in the other body; the tests hold the two against each
// other through the host composition.
//
// The kernel takes its own parameter struct beside RtiowParams, as the ray queries take RayQuery: RtiowParams does not grow.
// The LDS carve and the counters' way into P.stats are rl_rtiow_pixel_skeleton.h's (pixel_lds, pixel_flush_counters), shared with the AO,
// direct-lighting and NEE kernels; the other texts those kernels repeat stay written out, with a note where each stands.
// LDS (dynamic): [16][NT] u64 ChaCha ring; FAST: + [SD][NT] u32 stack + P.fg_top FastNodeQ.
// stats: [0] rays = samples traced, [5] words drawn (get_ray + media), [6] flagged, [7] rays the fast walk re-traced; STATS: [1..4].
#pragma once
#include "rl_material_query.h"
#include "rl_ray_query.h"
#include "rl_rtiow_pixel_skeleton.h"

namespace rl {

struct FeaturesQuery {
  unsigned long long n;     // slots: nrows * W of the shard, or the list's length
  const uint32_t *xs, *ys;  // pixel list (null: the shard's rows, slot = r * W + x, y = row_first + r * row_step)
  double *albedo_sum;       // [n][3] or null
  double *normal_sum;       // [n][3] or null
  double *depth_sum;        // [n]    or null
  uint32_t *hit_count;      // [n]    or null
};

// rtiow_hit_rays_fast_kernel's walk for one world ray (wo, wd, time) with Interval{1e-10, +inf}: -> rec; `slow`: the ray was re-traced in
// the reference's order; returns the flags (panic sites reached).
template <int NT, int SD>
__device__ __forceinline__ uint32_t features_fast_trace(const RtiowParams &P, const DevOp *ops, uint32_t *s_stack, const uint4 *s_top, int tid, D3 wo, D3 wd,
                                                        double time, Rec &rec, bool &slow) {
  const FastNodeQ *nodes = P.fg_nodes;
  const FastItem *items = P.fg_items;
  const uint32_t top = P.fg_top;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const float FINF = __int_as_float(0x7F800000);
  double closest = INF;
  uint32_t best = NONE, sp = 0, steps = 0;
  const RayAux32 ra32 = ray_aux32_direct(wo, wd);
  bool amb, unsafe;
  float grow;
  fastq_ray_start(P, wo, ra32, amb, unsafe, grow);
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
      e = fastq_pop<NT>(s_stack, tid, sp);
      continue;
    }
    const float c32 = unsafe ? FINF : (float)closest;
    // (node fetch, child tests and child order written out: as functions over a node struct, 214 - 1,608 lines of the same kernels changed)
    const Float4 *nd = e < top ? (const Float4 *)(s_top + e * 8u) : (const Float4 *)(nodes + e);
    const Float4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5];
    const uint4 ch = *(const uint4 *)(nd + 6);
    float k0, k1, k2, k3;
    const bool h0 = !fastq_missed(ra32, grow, c32, lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, k0) && ch.x != NONE;
    const bool h1 = !fastq_missed(ra32, grow, c32, lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, k1) && ch.y != NONE;
    const bool h2 = !fastq_missed(ra32, grow, c32, lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, k2) && ch.z != NONE;
    const bool h3 = !fastq_missed(ra32, grow, c32, lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, k3) && ch.w != NONE;
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
    if (nh >= 4) fastq_push<NT, SD>(s_stack, tid, sp, amb, c3);
    if (nh >= 3) fastq_push<NT, SD>(s_stack, tid, sp, amb, c2);
    if (nh >= 2) fastq_push<NT, SD>(s_stack, tid, sp, amb, c1);
    e = nh ? c0 : fastq_pop<NT>(s_stack, tid, sp);
  }
  rec = rec_none(INF);
  uint32_t hit_flags = 0;
  // the winner's HitRecord: the same test once more with ray_t.max = its root, then the POP chain
  // (written out: as one function with rtiow_hit_rays_fast_kernel's, 2 - 14 lines of the pixel renders and 276 of that kernel changed)
  if (!amb && best != NONE) {
    const FastItem it = items[best];
    const DevSphere sph = P.fg_spheres[best];
    const uint32_t wmat = P.fg_material[best];
    D3 o, d;
    replay_chain(P, ops, it.chain, wo, wd, o, d);
    const float oimax = fastq_leaf_oimax(ra32, it.chain, o, d);
    rec.t = closest;
    if (it.kind == 0) {
      if (sphere_hit_rec(sph, it.payload | SPH_UV, wmat, it.op_pc, o, d, time, rec)) hit_flags++;
      D3 c0 = ld3(sph.c0);
      D3 center = (it.payload & SPH_MOVING) ? c0 + ld3(sph.dc) * time : c0;
      D3 oc = o - center;
      double half_b = dot(oc, d), sq = sph.r2 * sph.inv_r * fabs(dot(d, rec.normal)), a = len2(d);
      double other = 2.0 * sq * (double)__builtin_amdgcn_rcpf((float)a);
      if (fast_hit_is_order_sensitive(oc, d, closest, sph.r2 * sph.inv_r, half_b, sq, closest, fabs(closest) + other, oimax)) amb = true;
    } else {
      if (planar_hit_rec(P.planars[it.payload], it.op_pc, o, d, rec)) hit_flags++;
    }
    if (!amb && !rec.any) amb = true;  // (cannot happen: the same arithmetic found this root)
    hit_flags += pop_rec_chain(P, ops, amb ? NONE : it.chain, rec);
  }
  slow = amb;
  if (amb) {  // the reference's own fold decides
    rec = rec_none(INF);
    GenCounters gc{0, 0, 0, 0, 0};
    auto draw = []() { return 0.0; };
    general_trace<false, false, true>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
    return (uint32_t)gc.flagged;
  }
  return hit_flags;
}

// P: the scene's tables (hit_query_params + materials, textures, images, Perlin), cam, key, first_sample, row_first / row_step / nrows,
// stats; FAST: also the query tree (fg_*, fg_top).
// Register budget: FAST is compiled for two workgroups per SIMD row (launch bounds 2 NT: 256 VGPRs, which its LDS allows too); left to
// itself it takes 315 and runs one wave per SIMD, measured 1.4x - 1.5x slower.  The reference-order instantiations
// carry general_trace with media and the counters at 350 - 376 registers: one wave per SIMD, as rtiow_hit_rays_seeded_kernel.
template <int NT, bool STATS, bool FAST, int SD>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(FAST ? 2 * NT : NT) rtiow_features_kernel(RtiowParams P, FeaturesQuery Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  unsigned long long *s_rng;
  uint32_t *s_stack;
  uint4 *s_top;
  pixel_lds<NT, FAST, SD>(smem, P, tid, s_rng, s_stack, s_top);
  const DevOp *ops = P.ops;
  const rl_rtiow_camera &cam = P.cam;
  const uint32_t W = cam.image_width, H = cam.image_height, S = cam.samples_per_pixel;
  const uint64_t WH = (uint64_t)W * (uint64_t)H;
  const D3 background = ld3(cam.background);
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  Ring<NT, true, true> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  unsigned long long c_rays = 0, c_nodes = 0, c_sph = 0, c_pl = 0, c_inst = 0, c_flag = 0, c_words = 0, c_slow = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    // (written out: as pixel_of_slot(), the operands of three v_add_f64 changed places in every instantiation)
    uint32_t px, y;
    if (Q.xs) px = Q.xs[idx], y = Q.ys[idx];
    else px = (uint32_t)(idx % W), y = P.row_first + (uint32_t)(idx / W) * P.row_step;
    D3 albedo = d3(0.0, 0.0, 0.0), normal = d3(0.0, 0.0, 0.0);
    double depth = 0.0;
    uint32_t hits = 0;
    const bool inside = px < W && y < H;  // (a list element outside the image, device form: zeros, nothing traced)
#pragma unroll 1
    for (uint32_t n = 0; inside && n < S; n++) {
      // (stream start, get_ray and time written out: as one function, 2 - 140 lines of every instantiation changed)
      const uint64_t sample_index = (uint64_t)n + P.first_sample;
      rng.pos = 0u, rng.nres = 0;
      rng.reset_stream(sample_index * WH + (uint64_t)px * (uint64_t)W + (uint64_t)y);
      // 1. Camera::get_ray (rtiow_camera_rays_kernel)
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
      // 2. world.hit(&ray, &Interval{1e-10, +inf})
      // (written out: as one function with general_trace's flags, 1,400 - 15,000 lines of every instantiation changed)
      c_rays++;
      Rec rec;
      if (FAST) {
        bool slow;
        c_flag += features_fast_trace<NT, SD>(P, ops, s_stack, s_top, tid, wo, wd, time, rec, slow);
        if (slow) c_slow++;
      } else {
        rec = rec_none(INF);
        GenCounters gc{0, 0, 0, 0, 0};
        auto draw = [&]() { return rng.gen_f64(); };
        general_trace<STATS, true, true>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
        c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
      }
      c_words += rng.pos;
      // 3. the factor the first vertex puts on the path, its normal and its ray parameter
      D3 a = background, nrm = d3(0.0, 0.0, 0.0);
      double dpt = 0.0;
      if (rec.any) {
        const DevMaterial &m = P.materials[rec.mat];
        a = material_texture<true>(m, [&](uint32_t tex) {
          double tu, tv;
          rec_uv(rec, tu, tv);
          return texture_value<2>(P, tex, tu, tv, rec.p);
        });
        if (m.kind == RL_MAT_METAL) a = ld3(m.albedo);
        else if (m.kind == RL_MAT_DIELECTRIC) a = d3(1.0, 1.0, 1.0);
        nrm = rec.normal, dpt = rec.t, hits++;
      }
      albedo = albedo + a, normal = normal + nrm, depth = depth + dpt;
    }
    if (Q.albedo_sum) {
      double *o = Q.albedo_sum + idx * 3;
      o[0] = albedo.x, o[1] = albedo.y, o[2] = albedo.z;
    }
    if (Q.normal_sum) {
      double *o = Q.normal_sum + idx * 3;
      o[0] = normal.x, o[1] = normal.y, o[2] = normal.z;
    }
    if (Q.depth_sum) Q.depth_sum[idx] = depth;
    if (Q.hit_count) Q.hit_count[idx] = hits;
  }
  pixel_flush_counters<STATS, FAST>(P.stats, tid, c_rays, c_words, c_flag, c_slow, c_nodes, c_sph, c_pl, c_inst);
}

}  // namespace rl
