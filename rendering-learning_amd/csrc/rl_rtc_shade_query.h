// RTC shading queries (include/rl_render.h rl_rtc_prepare_rays*, rl_rtc_shade_hits*, rl_rtc_shadow_attenuation*, rl_rtc_lighting*): what
// World::color_at does with a hit, as kernels of their own.
//
//   rtc_prepare_rays_kernel        hit(&World::intersect(&ray)).map(|h| h.prepare_computations(&ray, &xs)) (intersect.rs:48-115, :159-168):
//                                  rtc_intersect_all, the hit fold, the containers walk (always: the reference computes n1 / n2 for every
//                                  material) and the hit's Surface::color_at (rtc_hit_color)
//   rtc_shade_hits_kernel          World::shade_hit (world.rs:57-87) up to its recursion: per light a shadow rtc_intersect_all from over_point
//                                  and material::lighting, summed in light order; then Precomputation::schlick (intersect.rs:139-156) and
//                                  the reflected / refracted rays (world.rs:128-159)
//   rtc_shadow_attenuation_kernel  World::shadow_attenuation (world.rs:104-126) for arbitrary (point, light position) pairs
//   rtc_lighting_kernel            material::lighting (material.rs:54-90), pointwise: no Ent list, no traversal
//
// The kernels move records; the steps they take are the functions the render's color_at body calls (rl_rtc_shading.h, and the list
// steps of rl_rtc_full_kernel.h), so a host loop of prepare_rays + shade_hits reproduces rl_rtc_color_at_rays bit for bit
// (tests/test_gpu_rtc_shade_query.py).  One kept text: shade_hits writes rtc_schlick out, expression for expression (measured slower
// with the call).  Where the render skips a step whose result it would not use, the query takes it.  One
// element per lane, grid-stride over the batch, the launch shape of rtc_color_at_rays_kernel.  Records move as whole 8-byte words:
// rl_rtc_comps is 26 of them, rl_rtc_shade 19.
#pragma once
#include "rl_ray_query.h"

namespace rl {

static constexpr int RTC_COMPS_WORDS = 26;  // sizeof(rl_rtc_comps) / 8
static constexpr int RTC_SHADE_WORDS = 19;  // sizeof(rl_rtc_shade) / 8

struct RtcShadeQuery {
  unsigned long long n;
  uint32_t n_materials;
  // prepare
  const rl_ray *rays;
  rl_rtc_comps *out_comps;
  // shade / lighting
  const rl_rtc_comps *comps;
  rl_rtc_shade *out;
  double *out_shadow;  // [n][n_lights] (null: not wanted)
  // shadow attenuation / lighting
  const double *points;      // [n][3]
  const double *light_pos;   // [n][3]
  const double *light_int;   // [n][3]
  const double *shadow_att;  // [n]
  double *out_att;           // [n]
  double *out_rgb;           // [n][3]
};

template <int NT, int REGS_FOR>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(REGS_FOR) rtc_prepare_rays_kernel(RtcFullParams F, RtcShadeQuery Q) {
  const RtcParams &P = F.R;
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  const DevTri *tris = P.tris;
  RtcFullCounters cnt{0, 0, 0, 0, 0, 0};
  Ent list[RL_RTC_K];
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const rl_ray &ray = Q.rays[idx];
    const D3 origin = ld3(ray.origin), dir = ld3(ray.dir);
    double *out = (double *)(Q.out_comps + idx);
    cnt.rays += 1ull;
    uint32_t n = rtc_intersect_all(F, ops, tris, origin, dir, list, cnt, 1ull);
    int hi = rtc_first_hit(list, n);
    if (hi < 0) {
#pragma unroll
      for (int i = 0; i < RTC_COMPS_WORDS - 2; i++) out[i] = 0.0;
      ((uint64_t *)out)[24] = 0ull, ((uint64_t *)out)[25] = 0ull;
      continue;
    }
    Ent h = list[hi];
    const uint32_t mat = rtc_leaf_material(F, tris, h.leaf);
    const rl_rtc_material &m = P.materials[mat];
    const RtcComps c = rtc_prepare_computations(origin, dir, h.t, h.normal, cnt.flagged);
    double n1 = 1.0, n2 = 1.0;
    rtc_refractive_indices(F, tris, list, n, h, n1, n2);  // for every material, as the reference
    D3 object_color = rtc_hit_color(F, ops, m, h.chain, h.t, origin, dir);
    out[0] = h.t;
    out[1] = c.point.x, out[2] = c.point.y, out[3] = c.point.z;
    out[4] = c.eye_v.x, out[5] = c.eye_v.y, out[6] = c.eye_v.z;
    out[7] = c.normal_v.x, out[8] = c.normal_v.y, out[9] = c.normal_v.z;
    out[10] = c.over_point.x, out[11] = c.over_point.y, out[12] = c.over_point.z;
    out[13] = c.under_point.x, out[14] = c.under_point.y, out[15] = c.under_point.z;
    out[16] = c.reflect_v.x, out[17] = c.reflect_v.y, out[18] = c.reflect_v.z;
    out[19] = n1, out[20] = n2;
    out[21] = object_color.x, out[22] = object_color.y, out[23] = object_color.z;
    ((uint64_t *)out)[24] = 1ull | ((uint64_t)(c.inside ? 1u : 0u) << 32);  // hit | inside << 32
    ((uint64_t *)out)[25] = (uint64_t)h.leaf | ((uint64_t)mat << 32);      // object | material << 32
  }
  rtc_query_flush(cnt, P.stats, tid);
}

template <int NT, int REGS_FOR>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(REGS_FOR) rtc_shade_hits_kernel(RtcFullParams F, RtcShadeQuery Q) {
  const RtcParams &P = F.R;
  const int tid = threadIdx.x;
  const DevOp *ops = P.ops;
  const DevTri *tris = P.tris;
  RtcFullCounters cnt{0, 0, 0, 0, 0, 0};
  Ent list[RL_RTC_K];
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const double *k = (const double *)(Q.comps + idx);
    const uint64_t kw24 = ((const uint64_t *)k)[24], kw25 = ((const uint64_t *)k)[25];  // hit | inside << 32, object | material << 32
    const uint32_t mat = (uint32_t)(kw25 >> 32);
    double *out = (double *)(Q.out + idx);
    double *sh = Q.out_shadow ? Q.out_shadow + idx * P.n_lights : nullptr;
    if ((uint32_t)kw24 == 0u || mat >= Q.n_materials) {  // None, or an index outside the table (device form; the host form refuses it): zeros
#pragma unroll
      for (int i = 0; i < RTC_SHADE_WORDS - 1; i++) out[i] = 0.0;
      ((uint64_t *)out)[18] = 0ull;
      if (sh)
        for (uint32_t li = 0; li < P.n_lights; li++) sh[li] = 0.0;
      continue;
    }
    const rl_rtc_material &m = P.materials[mat];
    const D3 point = d3(k[1], k[2], k[3]), eye_v = d3(k[4], k[5], k[6]), normal_v = d3(k[7], k[8], k[9]);
    const D3 over_point = d3(k[10], k[11], k[12]);
    const D3 object_color = d3(k[21], k[22], k[23]);
    // shade_hit (world.rs:57-87): the first light's value starts the sum
    D3 lsum = d3(0.0, 0.0, 0.0);
    for (uint32_t li = 0; li < P.n_lights; li++) {
      const rl_rtc_light &light = P.lights[li];
      D3 lpos = ld3(light.position), intensity = ld3(light.intensity);
      double shadow_att = rtc_shadow_walk(F, ops, tris, over_point, lpos, list, cnt, 1ull);
      if (sh) sh[li] = shadow_att;
      D3 surface = rtc_lighting(m, point, object_color, lpos, intensity, eye_v, normal_v, shadow_att);
      lsum = (li == 0) ? surface : lsum + surface;
    }
    const double n1 = k[19], n2 = k[20];
    double reflectance;
    {  // rtc_schlick written out: with the call this kernel measured slower than before (profiles/rtc_shading_shared.txt 4d)
      double cosv = dot(eye_v, normal_v);
      double nn = n1 / n2;
      double sin2_t = nn * nn * (1.0 - cosv * cosv);
      double cos_t = sqrt(1.0 - sin2_t);
      double cos_adj = nn > 1.0 ? cos_t : cosv;
      if (sin2_t > 1.0 && nn > 1.0) reflectance = 1.0;
      else {
        double q = (n1 - n2) / (n1 + n2);
        double r0 = q * q;
        double x = 1.0 - cos_adj;
        double x2 = x * x;
        reflectance = r0 + (1.0 - r0) * (x * (x2 * x2));
      }
    }
    // reflected_color / refracted_color (world.rs:128-159): the rays they trace.  No light: the reference's reduce is None, no ray
    bool refract = false, reflect_ = false;
    D3 direction = d3(0.0, 0.0, 0.0);
    if (P.n_lights != 0 && m.transparency != 0.0) refract = rtc_refracted_direction(eye_v, normal_v, n1, n2, direction);
    if (P.n_lights != 0 && m.reflectivity != 0.0) reflect_ = true;
    out[0] = lsum.x, out[1] = lsum.y, out[2] = lsum.z;
    out[3] = reflectance;
    if (reflect_) {
      out[4] = over_point.x, out[5] = over_point.y, out[6] = over_point.z;
      out[7] = k[16], out[8] = k[17], out[9] = k[18];
    } else {
#pragma unroll
      for (int i = 4; i < 10; i++) out[i] = 0.0;
    }
    out[10] = 0.0;
    if (refract) {
      out[11] = k[13], out[12] = k[14], out[13] = k[15];
      out[14] = direction.x, out[15] = direction.y, out[16] = direction.z;
    } else {
#pragma unroll
      for (int i = 11; i < 17; i++) out[i] = 0.0;
    }
    out[17] = 0.0;
    ((uint64_t *)out)[18] = (uint64_t)(reflect_ ? 1u : 0u) | ((uint64_t)(refract ? 1u : 0u) << 32);  // reflect | refract << 32
  }
  rtc_query_flush(cnt, P.stats, tid);
}

template <int NT, int REGS_FOR>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(REGS_FOR) rtc_shadow_attenuation_kernel(RtcFullParams F, RtcShadeQuery Q) {
  const RtcParams &P = F.R;
  const int tid = threadIdx.x;
  RtcFullCounters cnt{0, 0, 0, 0, 0, 0};
  Ent list[RL_RTC_K];
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT)
    Q.out_att[idx] = rtc_shadow_walk(F, P.ops, P.tris, ld3(Q.points + idx * 3), ld3(Q.light_pos + idx * 3), list, cnt, 1ull);
  rtc_query_flush(cnt, P.stats, tid);
}

// materials: the scene's table (Q.n_materials entries).  An element with hit == 0 or a material outside the table gives zeros.
template <int NT>
__global__ void RL_KERNEL_ALIGN __launch_bounds__(NT) rtc_lighting_kernel(const rl_rtc_material *materials, RtcShadeQuery Q) {
  const int tid = threadIdx.x;
  for (unsigned long long idx = (unsigned long long)blockIdx.x * NT + tid; idx < Q.n; idx += (unsigned long long)gridDim.x * NT) {
    const double *k = (const double *)(Q.comps + idx);
    const uint64_t kw24 = ((const uint64_t *)k)[24], kw25 = ((const uint64_t *)k)[25];
    const uint32_t mat = (uint32_t)(kw25 >> 32);
    D3 c = d3(0.0, 0.0, 0.0);
    if ((uint32_t)kw24 != 0u && mat < Q.n_materials)
      c = rtc_lighting(materials[mat], d3(k[1], k[2], k[3]), d3(k[21], k[22], k[23]), ld3(Q.light_pos + idx * 3), ld3(Q.light_int + idx * 3),
                       d3(k[4], k[5], k[6]), d3(k[7], k[8], k[9]), Q.shadow_att[idx]);
    double *o = Q.out_rgb + idx * 3;
    o[0] = c.x, o[1] = c.y, o[2] = c.z;
  }
}

}  // namespace rl
