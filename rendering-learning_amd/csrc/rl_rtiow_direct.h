// Direct-lighting renders (include/rl_render.h "Direct-lighting renders", rl_rtiow_render_direct*): per pixel, over S
// jittered camera rays, the number that hit (hit_count) and, over K points drawn on each of L quad lights from every first hit, the sum
// of E * (cos cos_l area / |d|^2) over all of them (unshadowed) and over those whose segment hit -> light point is free (direct).
//
//   rtiow_direct_kernel<NT, STATS, FAST, SD>   one pixel per lane, grid-stride over the frame's or the list's slots; per lane a loop over
//                                              the samples F .. F + S - 1 and, inside a sample that hit, over the L lights and their K points.
//
// Per sample the kernel joins texts the library already has, so that the host composition of rl_rtiow_camera_rays, rl_rtiow_hit_rays, the
// definition's arithmetic and rl_rtiow_occluded_rays gives the same bytes (tests/test_gpu_render_direct.py):
//   1. the stream start and the camera arithmetic of every pixel-render kernel: Ring in an LDS column, word 0
//   2. the first hit, Interval{1e-10, +inf}
//        FAST = false  general_trace<STATS, false>
//        FAST = true   features_fast_trace, the function the feature and the AO kernel call
//   3. L x K times: two gen::<f64>() from the sample's ring, the light point, the geometry term in the header's operation order (binary64,
//      + - x / only, the file is compiled without contraction), and for a term that counts the any-hit test of Interval{1e-10, T} on the
//      segment Ray{hit.p, yl - hit.p, ray.time}
//        FAST = false  general_trace<STATS, false>, rec.any
//        FAST = true   ao_any_hit_walk (rl_rtiow_ao.h) CALLED, not copied: it takes an un-normalised direction and a pruning bound, which
//                      is a segment with tmax = T; then general_trace for a segment the walk leaves undecided (stats[7])
// The lights travel by value in the kernel argument (DirectQuery::lights, indexed by the loop counter alone: scalar loads), nl = u x v
// computed once on the host by vec3.rs's cross.  The sums are folded per lane in the definition's order and stored once: no atomics.
//
// Scenes with ConstantMedium objects are refused on the host (there is no seeded any-hit), so no trace here draws.
// No barrier and no wave-wide operation inside a lane's loops: lanes leave their walks, their L x K loops and their samples at different times.
// The LDS carve and the counters' way into P.stats are rl_rtiow_pixel_skeleton.h's (pixel_lds, pixel_flush_counters); the other texts this
// kernel has in common with the feature, AO and NEE kernels stay written out, with a note where each stands.
// LDS (dynamic): pixel_lds' plan.  stats: [0] rays = camera rays + segments traced, [5] words drawn (get_ray + 4 per light point),
// [6] flagged, [7] segments AND camera rays the fast walks handed to general_trace; STATS: [1..4] over both kinds of ray.
#pragma once
#include "rl_rtiow_ao.h"

namespace rl {

struct DirectLight {
  double Q[3], u[3], v[3], E[3];  // the caller's 12 doubles
  double nl[3];                   // u.cross(v), host-side (rl_direct_api.h)
};

struct DirectQuery {
  unsigned long long n;     // slots: nrows * W of the shard, or the list's length
  const uint32_t *xs, *ys;  // pixel list (null: the shard's rows, slot = r * W + x, y = row_first + r * row_step)
  uint32_t n_lights;        // L in 1 .. RL_DIRECT_MAX_LIGHTS
  uint32_t light_samples;   // K >= 1
  double seg_tmax;          // T in (1e-10, 1]: the closed end of the segments' interval
  double *direct;           // [n][3] or null
  double *unshadowed;       // [n][3] or null
  uint32_t *hit_count;      // [n] or null
  DirectLight lights[RL_DIRECT_MAX_LIGHTS];
};
static_assert(sizeof(RtiowParams) + sizeof(DirectQuery) <= 4096, "the two by-value kernel arguments must fit the 4 KiB kernarg segment");

// P: the scene's tables (hit_query_params), cam, key, first_sample, row_first / row_step, stats; FAST: also the query tree (fg_*, fg_top).
// Register budget: FAST is compiled for two workgroups per SIMD row, as rtiow_ao_kernel is and for its reason.
template <int NT, bool STATS, bool FAST, int SD>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(FAST ? 2 * NT : NT) rtiow_direct_kernel(RtiowParams P, DirectQuery Q) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  unsigned long long *s_rng;
  uint32_t *s_stack;
  uint4 *s_top;
  pixel_lds<NT, FAST, SD>(smem, P, tid, s_rng, s_stack, s_top);
  const DevOp *ops = P.ops;
  const rl_rtiow_camera &cam = P.cam;
  const uint32_t W = cam.image_width, H = cam.image_height, S = cam.samples_per_pixel, L = Q.n_lights, K = Q.light_samples;
  const uint64_t WH = (uint64_t)W * (uint64_t)H;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const double T = Q.seg_tmax;
  Ring<NT, true, true> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  unsigned long long c_rays = 0, c_nodes = 0, c_sph = 0, c_pl = 0, c_inst = 0, c_flag = 0, c_words = 0, c_slow = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    // (written out: as pixel_of_slot(), the operands of three v_add_f64 changed places in every instantiation)
    uint32_t px, y;
    if (Q.xs) px = Q.xs[idx], y = Q.ys[idx];
    else px = (uint32_t)(idx % W), y = P.row_first + (uint32_t)(idx / W) * P.row_step;
    double dr = 0.0, dg = 0.0, db = 0.0, ur = 0.0, ug = 0.0, ub = 0.0;
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
        auto draw = []() { return 0.0; };
        general_trace<STATS, false, false>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
        c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
      }
      if (rec.any) {
        hits++;
        const D3 hp = rec.p, hn = rec.normal;
        // 3. L x K light points: Ray{hit.p, yl - hit.p, ray.time} against Interval{1e-10, T}
#pragma unroll 1
        for (uint32_t l = 0; l < L; l++) {
          const DirectLight &lt = Q.lights[l];
#pragma unroll 1
          for (uint32_t k = 0; k < K; k++) {
            const double a = rng.gen_f64();
            const double b = rng.gen_f64();
            const D3 yl = (ld3(lt.Q) + ld3(lt.u) * a) + ld3(lt.v) * b;
            const D3 sd = yl - hp;
            const double d2 = len2(sd);
            const double cs = dot(hn, sd);
            const double cl = fabs(dot(ld3(lt.nl), sd));
            if (!(cs > 0.0) || !(cl > 0.0) || !(d2 > 0.0)) continue;  // faces away, edge-on or degenerate: nothing traced
            const double g = (cs * cl) / (d2 * d2);
            c_rays++;
            // (written out: as one function, 500 - 9,700 lines of every instantiation changed)
            bool occluded = false, fold = !FAST;
            if (FAST) {
              const int w = ao_any_hit_walk<NT, SD>(P, ops, s_stack, s_top, tid, hp, sd, time, T);
              occluded = w == AO_WALK_OCCLUDED;
              if (w == AO_WALK_UNDECIDED) fold = true, c_slow++;
            }
            if (fold) {  // the reference's own fold: every segment of !FAST, the undecided ones of FAST
              Rec orec = rec_none(T);
              GenCounters gc{0, 0, 0, 0, 0};
              auto draw = []() { return 0.0; };
              general_trace<STATS, false, false>(P, ops, 0u, NONE, hp, sd, hp, sd, time, 1e-10, orec, gc, draw);
              c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
              occluded = orec.any;
            }
            const double er = lt.E[0] * g, eg = lt.E[1] * g, eb = lt.E[2] * g;
            ur = ur + er, ug = ug + eg, ub = ub + eb;
            if (!occluded) dr = dr + er, dg = dg + eg, db = db + eb;
          }
        }
      }
      c_words += rng.pos;
    }
    if (Q.direct) Q.direct[idx * 3 + 0] = dr, Q.direct[idx * 3 + 1] = dg, Q.direct[idx * 3 + 2] = db;
    if (Q.unshadowed) Q.unshadowed[idx * 3 + 0] = ur, Q.unshadowed[idx * 3 + 1] = ug, Q.unshadowed[idx * 3 + 2] = ub;
    if (Q.hit_count) Q.hit_count[idx] = hits;
  }
  pixel_flush_counters<STATS, FAST>(P.stats, tid, c_rays, c_words, c_flag, c_slow, c_nodes, c_sph, c_pl, c_inst);
}

}  // namespace rl
