// NEE path renders (include/rl_render.h "NEE path renders", rl_rtiow_render_nee*): per pixel, over S jittered camera rays,
// the sum and the sum of squares of a path estimate of max_depth vertices that connects every Lambertian vertex but the last to K points
// drawn on each of L quad lights and, in exchange, does not count the emission the scattered ray of such a vertex finds.
//
//   rtiow_nee_kernel<NT, STATS, FAST, SD, MIS, SPH>   one pixel per lane, grid-stride over the frame's or the list's slots; per lane a loop over
//                                                the samples F .. F + S - 1, inside it over the path's vertices and, at a vertex that
//                                                samples the lights, over the L lights and their K points.
// MIS = true is the flavour of the renders with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance
// sampling", rl_rtiow_render_nee_mis*): every light point's g becomes wl, and the scattered ray of a vertex that sampled
// the lights is intersected with each light's parallelogram and, where it crosses one, connected with wb.  The heuristic is a runtime
// scalar of the launch (NeeMisQuery::heuristic).
// SPH = true (with MIS) is the flavour of the renders with sphere lights (include/rl_render.h "NEE path renders with sphere lights",
// rl_rtiow_render_nee_mis_spheres*): behind the L quads the light loop runs over Ls sphere lights, whose points are drawn
// with rng.unit_sphere() (pass 0) and whose near root the scattered ray is tested for (pass 1).  The light kind picks only how the
// candidate (sd, co) is made; d2, cs, g, the weight, the walk, the fold and the sum are the MIS flavour's one statement, under
// `if constexpr (SPH)` inside its body: the three MIS instantiations came out as the parent's, instruction for instruction, except with
// the skip stated once over a flag (two compares and their s_and_b64 changed places), hence the skip's two statements.
//
// Per vertex the kernel joins texts the library already has, so that the host composition of rl_rtiow_camera_rays, rl_rtiow_hit_rays, the
// definition's arithmetic, rl_rtiow_occluded_rays and rl_rtiow_scatter_rays gives the same bytes (tests/test_gpu_render_nee.py):
//   1. the stream start and the camera arithmetic of every pixel-render kernel: Ring in an LDS column, word 0
//   2. the closest hit of the path's ray, Interval{1e-10, +inf}
//        FAST = false  general_trace<STATS, false>
//        FAST = true   features_fast_trace, the function the feature, the AO and the direct kernel call (it takes any world ray)
//   3. material_texture (rl_rtiow_scatter.h), BEFORE anything of the scatter is live, as that file asks
//   4. at a Lambertian vertex that is not the last: rtiow_direct_kernel's L x K loop with the record's normal, the sum kept per vertex
//        FAST = false  general_trace<STATS, false>, rec.any
//        FAST = true   ao_any_hit_walk (rl_rtiow_ao.h), then general_trace for a segment the walk leaves undecided (stats[7])
//   5. material_scatter (rl_rtiow_scatter.h) drawing from the sample's ring AFTER the light points
//   MIS, at a vertex that took step 4, behind step 5's thr = thr * att: the ray-parallelogram crossing and the weights are this file's own
//        text (the header's lines, one rounded operation each; dot, cross and len2 are rl_device.h's, in vec3.rs' order); the segment from
//        the crossing point goes through step 4's segment statement, so the flavour has ONE inlined copy of ao_any_hit_walk and of the fold.
//        A vertex of the MIS flavour is a loop of two passes for that: pass 0 the light points, pass 1 step 5 and then the scattered ray's
//        candidates, one per light, through the same inner statement.
// The plain flavour's vertex body is kept VERBATIM beside the MIS flavour's under `if constexpr`: with the segment statement moved into a
// lambda shared by both (alone, or with the loops and step 5 shared as well), the three plain instantiations came out as other code (hundreds
// to thousands of changed lines, 328 -> 340 VGPRs for the counting one); kept apart they are the parent's instruction for instruction.
// None of the walks, of the texture or of the scatter is copied here.  The lights travel by value in the kernel argument (NeeQuery::lights,
// indexed by the loop counter alone: scalar loads), nl = u x v and kf = 1 / (pi K) computed once on the host.  c, thr and the two sums
// live in registers and are stored once per pixel: no atomics.
//
// Scenes with ConstantMedium objects are refused on the host (there is no seeded any-hit), so no trace here draws.
// No barrier and no wave-wide operation inside a lane's loops: lanes leave their walks, their loops and their paths at different times.
// The LDS carve and the counters' way into P.stats are rl_rtiow_pixel_skeleton.h's (pixel_lds, pixel_flush_counters); the other texts this
// kernel has in common with the feature, AO and direct-lighting kernels stay written out, with a note where each stands.
// LDS (dynamic): pixel_lds' plan; the one [SD][NT] stack serves the closest-hit and the any-hit walk in turn.
// stats (MIS: the scattered rays' segments are segments): [0] rays = path rays + segments traced, [5] words drawn, [6] flagged (the walks' and the Dielectric's panic site), [7] segments AND
// path rays the fast walks handed to general_trace; STATS: [1..4] over both kinds of ray.
#pragma once
#include "rl_rtiow_direct.h"

namespace rl {

struct NeeQuery {
  unsigned long long n;     // slots: nrows * W of the shard, or the list's length
  const uint32_t *xs, *ys;  // pixel list (null: the shard's rows, slot = r * W + x, y = row_first + r * row_step)
  uint32_t n_lights;        // L in 1 .. RL_DIRECT_MAX_LIGHTS
  uint32_t light_samples;   // K >= 1
  double seg_tmax;          // T in (1e-10, 1]: the closed end of the segments' interval
  double kf;                // 1.0 / (M_PI * (double)K), the host's double
  double *sums;             // [n][3] or null
  double *sq;               // [n][3] or null
  DirectLight lights[RL_DIRECT_MAX_LIGHTS];
};
// The MIS flavour's argument: one scalar more, in a type of its own so that the plain flavour's kernarg segment keeps its size
struct NeeMisQuery : NeeQuery {
  uint32_t heuristic;  // RL_MIS_BALANCE or RL_MIS_POWER (wave-uniform: a scalar load and a scalar branch)
};
// The sphere-light flavour's argument: the number of sphere lights, again in a type of its own.  The two kinds share the RL_DIRECT_MAX_LIGHTS
// slots: lights[0 .. n_lights) are the quads, lights[n_lights .. n_lights + n_sphere_lights) the spheres, a sphere in a slot as
//   Q = C, E = E, u[0] = r, u[1] = A = (4.0 * M_PI) * (r * r), the host's double (sphere_r, sphere_A below); v and nl are not read.
struct NeeSpheresQuery : NeeMisQuery {
  uint32_t n_sphere_lights;  // Ls; L + Ls in 1 .. RL_DIRECT_MAX_LIGHTS, L may be 0
};
__host__ __device__ inline double &sphere_r(DirectLight &l) { return l.u[0]; }
__host__ __device__ inline double &sphere_A(DirectLight &l) { return l.u[1]; }
template <bool MIS, bool SPH = false>
using NeeQueryOf = typename std::conditional<SPH, NeeSpheresQuery, typename std::conditional<MIS, NeeMisQuery, NeeQuery>::type>::type;
static_assert(sizeof(RtiowParams) + sizeof(NeeSpheresQuery) <= 4096, "the two by-value kernel arguments must fit the 4 KiB kernarg segment");

// P: the scene's tables (hit_query_params + materials, textures, images, Perlin), cam, key, first_sample, row_first / row_step, stats;
// FAST: also the query tree (fg_*, fg_top).
// Register budget (DESIGN.md §3.22 has the table): compiled for two workgroups per SIMD row as rtiow_direct_kernel is, FAST takes all 256
// VGPRs and spills 68 more to 276 bytes of scratch, so it is compiled for ONE (NEE_FAST_WG = 1) and spills nothing.  The MIS flavour at one
// (DESIGN.md §3.23): FAST 338 VGPRs + 82 AGPRs, counting 324 + 68, counter-free reference order 308 + 52; no VGPR spilled, no scratch.
// The sphere-light flavour at one: FAST 344 + 88, counting 328 + 72, counter-free reference order 312 + 56; again no VGPR
// spilled and no scratch.
constexpr int NEE_FAST_WG = 1;
template <int NT, bool STATS, bool FAST, int SD, bool MIS, bool SPH = false>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(FAST ? NEE_FAST_WG * NT : NT) rtiow_nee_kernel(RtiowParams P, NeeQueryOf<MIS, SPH> Q) {
  static_assert(MIS || !SPH, "sphere lights are a flavour of the renders with multiple importance sampling");
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x;
  unsigned long long *s_rng;
  uint32_t *s_stack;
  uint4 *s_top;
  pixel_lds<NT, FAST, SD>(smem, P, tid, s_rng, s_stack, s_top);
  const DevOp *ops = P.ops;
  const rl_rtiow_camera &cam = P.cam;
  const uint32_t W = cam.image_width, H = cam.image_height, S = cam.samples_per_pixel, L = Q.n_lights, K = Q.light_samples;
  const uint32_t max_depth = cam.max_depth;
  const uint64_t WH = (uint64_t)W * (uint64_t)H;
  const double INF = __longlong_as_double(0x7FF0000000000000ll);
  const double T = Q.seg_tmax, kf = Q.kf;
  Ring<NT, true, true> rng{P.key, s_rng, tid, 0ull, 0u, 0u, 0u};
  unsigned long long c_rays = 0, c_nodes = 0, c_sph = 0, c_pl = 0, c_inst = 0, c_flag = 0, c_words = 0, c_slow = 0;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    // (written out: as pixel_of_slot(), the operands of three v_add_f64 changed places in every instantiation)
    uint32_t px, y;
    if (Q.xs) px = Q.xs[idx], y = Q.ys[idx];
    else px = (uint32_t)(idx % W), y = P.row_first + (uint32_t)(idx / W) * P.row_step;
    D3 sum = d3(0.0, 0.0, 0.0), sum2 = d3(0.0, 0.0, 0.0);
    const bool inside = px < W && y < H;  // (a list element outside the image, device form: zeros, nothing traced)
#pragma unroll 1
    for (uint32_t n = 0; inside && n < S; n++) {
      // (stream start, get_ray and time written out: as one function, 2 - 140 lines of every instantiation changed)
      const uint64_t sample_index = (uint64_t)n + P.first_sample;
      rng.pos = 0u, rng.nres = 0;
      rng.reset_stream(sample_index * WH + (uint64_t)px * (uint64_t)W + (uint64_t)y);
      // 1. Camera::get_ray (rtiow_camera_rays_kernel)
      D3 wo, wd;
      {
        D3 p00 = ld3(cam.pixel_00), du = ld3(cam.pixel_du), dv = ld3(cam.pixel_dv);
        D3 pixel_center = (p00 + du * (double)px) + dv * (double)y;
        double sx = -0.5 + rng.gen_f64();
        double sy = -0.5 + rng.gen_f64();
        D3 pixel_sample = pixel_center + (du * sx + dv * sy);
        if (cam.defocus_angle <= 0.0) wo = ld3(cam.lookfrom);
        else {
          double a, b;
          rng.unit_disc(a, b);
          wo = (ld3(cam.lookfrom) + ld3(cam.defocus_disk_u) * a) + ld3(cam.defocus_disk_v) * b;
        }
        wd = pixel_sample - wo;
      }
      const double time = rng.gen_f64();
      D3 c = d3(0.0, 0.0, 0.0), thr = d3(1.0, 1.0, 1.0);
      bool count_emission = true;
#pragma unroll 1
      for (uint32_t i = 1; i <= max_depth; i++) {
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
          general_trace<STATS, false, true>(P, ops, 0u, NONE, wo, wd, wo, wd, time, 1e-10, rec, gc, draw);
          c_nodes += gc.nodes, c_sph += gc.spheres, c_pl += gc.planars, c_inst += gc.instances, c_flag += gc.flagged;
        }
        if (!rec.any) {
          c = c + thr * ld3(cam.background);
          break;
        }
        const DevMaterial &m = P.materials[rec.mat];
        // 3. the texture value: the Lambertian attenuation, the DiffuseLight emission
        const D3 texc = material_texture<true>(m, [&](uint32_t tex) {
          double tu, tv;
          rec_uv(rec, tu, tv);
          return texture_value<2>(P, tex, tu, tv, rec.p);
        });
        const D3 hp = rec.p, hn = rec.normal;
        const bool sampled = m.kind == RL_MAT_LAMBERTIAN && i < max_depth;
        if constexpr (!MIS) {
          // 4. L x K light points: Ray{hit.p, yl - hit.p, ray.time} against Interval{1e-10, T}
          if (sampled) {
            D3 dsum = d3(0.0, 0.0, 0.0);
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
                if (!occluded) dsum = d3(dsum.x + lt.E[0] * g, dsum.y + lt.E[1] * g, dsum.z + lt.E[2] * g);
              }
            }
            c = c + ((thr * texc) * dsum) * kf;
          }
          // 5. mat.emitted and mat.scatter, drawing after the light points
          const Scatter s = material_scatter<true>(m, wd, hn, rec.front, [&] { return texc; }, rng);
          if (s.flagged) c_flag++;
          if (count_emission) c = c + thr * s.emitted;  // (zeros unless the material is a DiffuseLight)
          if (s.what != SCATTER_RAY) break;
          thr = thr * s.att;
          wo = hp, wd = s.dir;
          count_emission = !sampled;
        } else {
          // MIS.  pass 0: step 4 at a sampling vertex with wl in g's place; pass 1: step 5 and, behind a sampling vertex, its scattered ray
          // against each light's parallelogram with wb (no draw).  Both passes run the ONE segment statement below: one copy of the walks.
          bool ended = false;
#pragma unroll 1
          for (uint32_t pass = sampled ? 0u : 1u; pass < 2u; pass++) {
            if (pass) {
              const Scatter s = material_scatter<true>(m, wd, hn, rec.front, [&] { return texc; }, rng);
              if (s.flagged) c_flag++;
              if (count_emission) c = c + thr * s.emitted;
              if (s.what != SCATTER_RAY) {
                ended = true;
                break;
              }
              thr = thr * s.att;
              wo = hp, wd = s.dir;
              count_emission = !sampled;
              if (!sampled) break;
            }
            D3 dsum = d3(0.0, 0.0, 0.0);
            uint32_t LT = L;  // SPH: the Ls sphere lights follow the L quads in Q.lights
            if constexpr (SPH) LT = L + Q.n_sphere_lights;
#pragma unroll 1
            for (uint32_t l = 0; l < LT; l++) {
              const DirectLight &lt = Q.lights[l];
#pragma unroll 1
              for (uint32_t k = 0; k < (pass ? 1u : K); k++) {
                D3 sd;
                // SPH, a sphere light: only how the candidate (sd, co) is made differs; co * A stands where a quad has |nl . sd|
                bool sph = false;
                double co = 0.0;
                if constexpr (SPH) sph = l >= L;
                if (SPH && sph) {
                  const D3 C = ld3(lt.Q);
                  const double r = lt.u[0];
                  if (!pass) {  // UnitSphere.sample(rng): 4 words per try, drawn whether or not the point counts
                    const D3 w = rng.unit_sphere();
                    const D3 yl = C + w * r;
                    sd = yl - hp;
                    co = -dot(w, sd);
                  } else {  // Sphere::hit's order (sphere.rs:36-49), the near root only: a vertex inside the sphere gets nothing
                    const D3 oc = hp - C;
                    const double a = len2(wd);
                    const double hb = dot(oc, wd);
                    const double cc = len2(oc) - r * r;
                    const double disc = hb * hb - a * cc;
                    if (!(disc > 0.0)) continue;  // beside the sphere, or grazing it
                    const double t = (-hb - sqrt(disc)) / a;
                    if (!(t > 0.0) || !(t < INF)) continue;  // the sphere is behind the vertex, or the vertex is inside it
                    sd = wd * t;
                    const D3 yc = (hp + sd) - C;
                    const D3 wn = d3(yc.x / r, yc.y / r, yc.z / r);
                    co = -dot(wn, sd);
                  }
                } else if (!pass) {
                  const double a = rng.gen_f64();
                  const double b = rng.gen_f64();
                  const D3 yl = (ld3(lt.Q) + ld3(lt.u) * a) + ld3(lt.v) * b;
                  sd = yl - hp;
                } else {  // wd is the scattered direction by now, as material_scatter gives it (not normalised)
                  const D3 nl = ld3(lt.nl);
                  const double den = dot(nl, wd);
                  if (!(fabs(den) > 0.0)) continue;  // along the light's plane
                  const double t = dot(nl, ld3(lt.Q) - hp) / den;
                  if (!(t > 0.0) || !(t < INF)) continue;  // the plane is behind the vertex
                  sd = wd * t;
                  const D3 h = (hp + sd) - ld3(lt.Q);
                  const double nn = dot(nl, nl);
                  const double al = dot(nl, cross(h, ld3(lt.v))) / nn;
                  const double be = dot(nl, cross(ld3(lt.u), h)) / nn;
                  if (!(0.0 <= al && al <= 1.0) || !(0.0 <= be && be <= 1.0)) continue;  // beside the parallelogram
                }
                const double d2 = len2(sd);
                const double cs = dot(hn, sd);
                const double cl = (SPH && sph) ? co * lt.u[1] : fabs(dot(ld3(lt.nl), sd));
                // (the skip twice: with one statement over a flag, the MIS instantiations ordered these compares otherwise)
                if constexpr (SPH) {  // a quad emits from both sides, a sphere outward only: its far side costs draws but no trace
                  if (!(cs > 0.0) || !(sph ? co > 0.0 : cl > 0.0) || !(d2 > 0.0)) continue;
                } else if (!(cs > 0.0) || !(cl > 0.0) || !(d2 > 0.0)) continue;  // faces away, edge-on or degenerate: nothing traced
                const double g = (cs * cl) / (d2 * d2);
                if (!(g < INF)) continue;
                // q = p_bsdf / (K p_light) exactly; wl = g / (1 + q^b), wb = q^b / (1 + q^b), b = 1 (balance) or 2 (power)
                const double q = g * kf;
                const double qb = Q.heuristic == RL_MIS_POWER ? q * q : q;
                const double wt = (pass ? qb : g) / (1.0 + qb);
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
                if (!occluded) dsum = d3(dsum.x + lt.E[0] * wt, dsum.y + lt.E[1] * wt, dsum.z + lt.E[2] * wt);
              }
            }
            c = pass ? c + thr * dsum : c + ((thr * texc) * dsum) * kf;
          }
          if (ended) break;
        }
      }
      c_words += rng.pos;
      sum = sum + c, sum2 = sum2 + c * c;
    }
    if (Q.sums) Q.sums[idx * 3 + 0] = sum.x, Q.sums[idx * 3 + 1] = sum.y, Q.sums[idx * 3 + 2] = sum.z;
    if (Q.sq) Q.sq[idx * 3 + 0] = sum2.x, Q.sq[idx * 3 + 1] = sum2.y, Q.sq[idx * 3 + 2] = sum2.z;
  }
  pixel_flush_counters<STATS, FAST>(P.stats, tid, c_rays, c_words, c_flag, c_slow, c_nodes, c_sph, c_pl, c_inst);
}

}  // namespace rl
