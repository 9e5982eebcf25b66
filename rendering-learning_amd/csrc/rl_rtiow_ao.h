// Ambient-occlusion renders (include/rl_render.h "Ambient-occlusion renders", rl_rtiow_render_ao*): per pixel, over S
// jittered camera rays, the number that hit (hit_count) and, over the K cosine-weighted rays sent from each first hit, the number that
// reach the distance R unoccluded (open_count).  Both outputs are integers: any launch geometry gives the same bytes.
//
//   rtiow_ao_kernel<NT, STATS, FAST, SD>   one pixel per lane, grid-stride over the frame's or the list's slots; per lane a loop over the
//                                          samples F .. F + S - 1 and, inside a sample that hit, over its K ambient rays.
//
// Per sample the kernel joins texts the library already has, so that the host composition of rl_rtiow_camera_rays, rl_rtiow_hit_rays,
// rl_rtiow_scatter_rays (on a Lambertian) and rl_rtiow_occluded_rays gives the same counts (tests/test_gpu_render_ao.py):
//   1. the stream start and the camera arithmetic of every pixel-render kernel: Ring in an LDS column, word 0
//   2. the first hit, Interval{1e-10, +inf}
//        FAST = false  general_trace<STATS, false>
//        FAST = true   features_fast_trace, the function the feature kernel calls (no further copy of the closest-hit walk)
//   3. K times: the Lambertian direction from material_scatter (rl_rtiow_scatter.h, the one statement of it) drawing from the sample's
//      ring, normalize(), and the any-hit test of Interval{1e-10, R} from the hit point at the camera ray's time
//        FAST = false  general_trace<STATS, false>, rec.any
//        FAST = true   ao_any_hit_walk below, then general_trace for a ray the walk leaves undecided (stats[7])
// ao_any_hit_walk is the per-ray text of rtiow_occluded_rays_fast_kernel (rl_occlusion_query.h) as a function; the kernel does not call
// it (two more spilled SGPRs there).  Both call the pieces of rl_rtiow_fast_walk.h: the ray start,
// the per-lane stack, the leaf's oimax, the box test with the filter's threshold.  What remains a second copy of the any-hit form: the
// loop skeleton with its head, the node fetch with the four child tests, the stored-order visit.  A change to one of those belongs in
// the other body, and the tests hold the two against each other through the host composition.
//
// Scenes with ConstantMedium objects are refused on the host (there is no seeded any-hit), so no trace here draws.
// No barrier and no wave-wide operation inside a lane's loops: lanes leave their walks, their K loops and their samples at different times.
// The LDS carve and the counters' way into P.stats are rl_rtiow_pixel_skeleton.h's (pixel_lds, pixel_flush_counters); the other texts this
// kernel has in common with the feature, direct-lighting and NEE kernels stay written out, with a note where each stands.
// LDS (dynamic): [16][NT] u64 ChaCha ring; FAST: + [SD][NT] u32 stack, used by the two walks in turn, + P.fg_top FastNodeQ staged once.
// stats: [0] rays = camera rays + ambient rays, [5] words drawn (get_ray + the K unit vectors), [6] flagged, [7] ambient rays AND camera
// rays the fast walks handed to general_trace; STATS: [1..4] over both kinds of ray.
#pragma once
#include "rl_occlusion_query.h"
#include "rl_rtiow_features.h"
#include "rl_rtiow_scatter.h"

namespace rl {

struct AoQuery {
  unsigned long long n;     // slots: nrows * W of the shard, or the list's length
  const uint32_t *xs, *ys;  // pixel list (null: the shard's rows, slot = r * W + x, y = row_first + r * row_step)
  uint32_t ao_rays;         // K >= 1
  double radius;            // R > 0, +inf allowed: the closed end of the ambient rays' interval
  uint32_t *open_count;     // [n] or null
  uint32_t *hit_count;      // [n] or null
};

enum AoWalk : int { AO_WALK_OPEN = 0, AO_WALK_OCCLUDED = 1, AO_WALK_UNDECIDED = 2 };

// rtiow_occluded_rays_fast_kernel's walk for one world ray (wo, wd, time) with Interval{1e-10, tmax}: stored child order, the pruning
// bound fixed at tmax, roots classified by occ_sphere_root / occ_planar_root.  AO_WALK_UNDECIDED: only uncertain roots were seen, or the
// walk gave up (filter range, grow, stack, step budget) — the reference's fold decides.
template <int NT, int SD>
__device__ __forceinline__ int ao_any_hit_walk(const RtiowParams &P, const DevOp *ops, uint32_t *s_stack, const uint4 *s_top, int tid, D3 wo, D3 wd, double time,
                                               double tmax) {
  const FastNodeQ *nodes = P.fg_nodes;
  const FastItem *items = P.fg_items;
  const uint32_t top = P.fg_top;
  const float FINF = __int_as_float(0x7F800000);
  uint32_t sp = 0, steps = 0;
  const RayAux32 ra32 = ray_aux32_direct(wo, wd);
  bool amb, unsafe;
  bool unc = false;  // an uncertain root was seen
  float grow;
  fastq_ray_start(P, wo, ra32, amb, unsafe, grow);
  const float c32 = unsafe ? FINF : (float)tmax;  // the pruning bound: R, first step to last
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
      if (found == OCC_CERTAIN) return AO_WALK_OCCLUDED;
      unc = unc || found == OCC_UNCERTAIN;
      e = fastq_pop<NT>(s_stack, tid, sp);
      continue;
    }
    // (node fetch, child tests and child order written out: as functions over a node struct, 214 - 1,608 lines of the same kernels changed)
    const Float4 *nd = e < top ? (const Float4 *)(s_top + e * 8u) : (const Float4 *)(nodes + e);
    const Float4 lx = nd[0], ly = nd[1], lz = nd[2], hx = nd[3], hy = nd[4], hz = nd[5];
    const uint4 ch = *(const uint4 *)(nd + 6);
    float k0, k1, k2, k3;  // (the entry distances: not used, the children are visited in stored order)
    const bool h0 = !fastq_missed(ra32, grow, c32, lx.x, hx.x, ly.x, hy.x, lz.x, hz.x, k0) && ch.x != NONE;
    const bool h1 = !fastq_missed(ra32, grow, c32, lx.y, hx.y, ly.y, hy.y, lz.y, hz.y, k1) && ch.y != NONE;
    const bool h2 = !fastq_missed(ra32, grow, c32, lx.z, hx.z, ly.z, hy.z, lz.z, hz.z, k2) && ch.z != NONE;
    const bool h3 = !fastq_missed(ra32, grow, c32, lx.w, hx.w, ly.w, hy.w, lz.w, hz.w, k3) && ch.w != NONE;
    uint32_t first = NONE;  // children in STORED order (rtiow_occluded_rays_fast_kernel says why)
    auto visit = [&](bool h, uint32_t c) {
      if (!h) return;
      if (first != NONE) fastq_push<NT, SD>(s_stack, tid, sp, amb, first);
      first = c;
    };
    visit(h3, ch.w), visit(h2, ch.z), visit(h1, ch.y), visit(h0, ch.x);
    e = first != NONE ? first : fastq_pop<NT>(s_stack, tid, sp);
  }
  return (amb || unc) ? AO_WALK_UNDECIDED : AO_WALK_OPEN;
}

// P: the scene's tables (hit_query_params), cam, key, first_sample, row_first / row_step, stats; FAST: also the query tree (fg_*, fg_top).
// Register budget: FAST is compiled for two workgroups per SIMD row, as rtiow_features_kernel is and for its reason.
template <int NT, bool STATS, bool FAST, int SD>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(FAST ? 2 * NT : NT) rtiow_ao_kernel(RtiowParams P, AoQuery Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  unsigned long long *s_rng;
  uint32_t *s_stack;
  uint4 *s_top;
  pixel_lds<NT, FAST, SD>(smem, P, tid, s_rng, s_stack, s_top);
  const DevOp *ops = P.ops;
  const rl_rtiow_camera &cam = P.cam;
  const uint32_t W = cam.image_width, H = cam.image_height, S = cam.samples_per_pixel, K = Q.ao_rays;
  const uint64_t WH = (uint64_t)W * (uint64_t)H;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const double R = Q.radius;
  DevMaterial lambertian{};  // Lambertian::scatter's direction whatever the hit's material: the kind is all material_scatter reads of it
  lambertian.kind = RL_MAT_LAMBERTIAN;
  Ring<NT, true, true> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  unsigned long long c_rays = 0, c_nodes = 0, c_sph = 0, c_pl = 0, c_inst = 0, c_flag = 0, c_words = 0, c_slow = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    // (written out: as pixel_of_slot(), the operands of three v_add_f64 changed places in every instantiation)
    uint32_t px, y;
    if (Q.xs) px = Q.xs[idx], y = Q.ys[idx];
    else px = (uint32_t)(idx % W), y = P.row_first + (uint32_t)(idx / W) * P.row_step;
    uint32_t open = 0, hits = 0;
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
        auto draw = []() { return 0.0; };
        general_trace<STATS, false, false>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
        c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
      }
      if (rec.any) {
        hits++;
        const D3 hp = rec.p, hn = rec.normal;
        const bool front = rec.front;
        // 3. K ambient rays: Ray{hit.p, (normal + random_unit_vector).normalize(), ray.time} against Interval{1e-10, R}
#pragma unroll 1
        for (uint32_t k = 0; k < K; k++) {
          const Scatter sc = material_scatter<false>(lambertian, wd, hn, front, [] { return d3(0.0, 0.0, 0.0); }, rng);
          const D3 ad = normalize(sc.dir);
          c_rays++;
          // (written out: as one function, 500 - 9,700 lines of every instantiation changed)
          bool occluded = false, fold = !FAST;
          if (FAST) {
            const int w = ao_any_hit_walk<NT, SD>(P, ops, s_stack, s_top, tid, hp, ad, time, R);
            occluded = w == AO_WALK_OCCLUDED;
            if (w == AO_WALK_UNDECIDED) fold = true, c_slow++;
          }
          if (fold) {  // the reference's own fold: every ray of !FAST, the undecided ones of FAST
            Rec orec = rec_none(R);
            GenCounters gc{0, 0, 0, 0, 0};
            auto draw = []() { return 0.0; };
            general_trace<STATS, false, false>(P, ops, 0u, NONE, hp, ad, hp, ad, time, 1e-10, orec, gc, draw);
            c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
            occluded = orec.any;
          }
          open += occluded ? 0u : 1u;
        }
      }
      c_words += rng.pos;
    }
    if (Q.open_count) Q.open_count[idx] = open;
    if (Q.hit_count) Q.hit_count[idx] = hits;
  }
  pixel_flush_counters<STATS, FAST>(P.stats, tid, c_rays, c_words, c_flag, c_slow, c_nodes, c_sph, c_pl, c_inst);
}

}  // namespace rl
