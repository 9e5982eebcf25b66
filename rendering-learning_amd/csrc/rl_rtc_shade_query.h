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
// The shading arithmetic is rl_rtc_color_at_body.inc restated here, expression for expression: a host loop of prepare_rays + shade_hits
// reproduces rl_rtc_color_at_rays bit for bit (tests/test_gpu_rtc_shade_query.py), and the render body carries none of this code.  One
// element per lane, grid-stride over the batch, the launch shape of rtc_color_at_rays_kernel.  Records move as whole 8-byte words:
// rl_rtc_comps is 26 of them, rl_rtc_shade 19.
#pragma once
#include "rl_ray_query.h"  // rtc_query_flush

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

// World::shadow_attenuation(&point, light) (world.rs:104-126); the list is scratch for the shadow ray's intersections
__device__ __forceinline__ double rtc_shadow_walk(const RtcFullParams &F, const DevOp *ops, const DevTri *tris, D3 point, D3 lpos, Ent *list,
                                                  RtcFullCounters &cnt) {
  const RtcParams &P = F.R;
  D3 v = lpos - point;
  double distance = mag(v);
  D3 sdir;
  double shadow_att = 1.0;
  if (norm(v, sdir)) {
    cnt.rays += 1ull;
    uint32_t ns = rtc_intersect_all(F, ops, tris, point, sdir, list, cnt, 1ull);
    for (uint32_t i = 0; i < ns; i++) {
      if (!(list[i].t > 0.0 && list[i].t < distance)) continue;
      bool dup = false;  // take_while(seen.insert): every earlier in-range entry is in `seen`
      for (uint32_t k = 0; k < i; k++) dup |= list[k].t > 0.0 && list[k].t < distance && list[k].leaf == list[i].leaf;
      if (dup) break;
      shadow_att = shadow_att * P.materials[rtc_leaf_material(F, tris, list[i].leaf)].transparency;
    }
  }
  return shadow_att;
}

// material::lighting (material.rs:54-90)
__device__ __forceinline__ D3 rtc_lighting(const rl_rtc_material &m, D3 point, D3 object_color, D3 lpos, D3 intensity, D3 eye_v, D3 normal_v,
                                           double shadow_att) {
  D3 effective = object_color * intensity;
  D3 lightv;
  if (!norm(lpos - point, lightv)) lightv = d3(0.0, 0.0, 0.0);
  D3 ambient = effective * m.ambient;
  double ldn = dot(lightv, normal_v);
  D3 diffuse = d3(0.0, 0.0, 0.0), specular = d3(0.0, 0.0, 0.0);
  if (!(ldn < 0.0)) {
    D3 diff = (effective * m.diffuse) * ldn;
    D3 reflectv = -reflect(lightv, normal_v);
    double rde = dot(reflectv, eye_v);
    diffuse = diff * shadow_att;
    if (!(rde <= 0.0)) {
      double factor = pow(rde, m.shininess);
      specular = intensity * (m.specular * factor * shadow_att);
    }
  }
  return (ambient + diffuse) + specular;
}

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
    int hi = -1;  // intersect.rs:159-168: lowest t >= 0, later wins ties
    for (uint32_t i = 0; i < n; i++)
      if (list[i].t >= 0.0 && (hi < 0 || !(list[hi].t < list[i].t))) hi = (int)i;
    if (hi < 0) {
#pragma unroll
      for (int i = 0; i < RTC_COMPS_WORDS - 2; i++) out[i] = 0.0;
      ((uint64_t *)out)[24] = 0ull, ((uint64_t *)out)[25] = 0ull;
      continue;
    }
    // prepare_computations (intersect.rs:48-115)
    Ent h = list[hi];
    const uint32_t mat = rtc_leaf_material(F, tris, h.leaf);
    const rl_rtc_material &m = P.materials[mat];
    D3 point = origin + dir * h.t;
    D3 eye_v;
    if (!norm(-dir, eye_v)) {
      cnt.flagged++;
      eye_v = -dir;
    }
    D3 normal_v = h.normal;
    const bool inside = dot(normal_v, eye_v) < 0.0;
    if (inside) normal_v = -normal_v;
    D3 over_point = point + normal_v * 1e-5;
    D3 under_point = point - normal_v * 1e-5;
    D3 reflect_v;
    if (!norm(reflect(dir, normal_v), reflect_v)) {
      cnt.flagged++;
      reflect_v = dir;
    }
    double n1 = 1.0, n2 = 1.0;
    {  // the containers walk, for every material (intersect.rs:72-99)
      uint32_t is = 0;
      while (is < n && !(rtc_are_equal(list[is].t, h.t) && list[is].leaf == h.leaf)) is++;
      if (is < n) {
        uint32_t c1 = rtc_last_container(list, is), c2 = rtc_last_container(list, is + 1);
        if (c1 != NONE) n1 = P.materials[rtc_leaf_material(F, tris, c1)].refractive_index;
        if (c2 != NONE) n2 = P.materials[rtc_leaf_material(F, tris, c2)].refractive_index;
      }
    }
    D3 object_color = rtc_hit_color(F, ops, m, h.chain, h.t, origin, dir);
    out[0] = h.t;
    out[1] = point.x, out[2] = point.y, out[3] = point.z;
    out[4] = eye_v.x, out[5] = eye_v.y, out[6] = eye_v.z;
    out[7] = normal_v.x, out[8] = normal_v.y, out[9] = normal_v.z;
    out[10] = over_point.x, out[11] = over_point.y, out[12] = over_point.z;
    out[13] = under_point.x, out[14] = under_point.y, out[15] = under_point.z;
    out[16] = reflect_v.x, out[17] = reflect_v.y, out[18] = reflect_v.z;
    out[19] = n1, out[20] = n2;
    out[21] = object_color.x, out[22] = object_color.y, out[23] = object_color.z;
    ((uint64_t *)out)[24] = 1ull | ((uint64_t)(inside ? 1u : 0u) << 32);  // hit | inside << 32
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
      double shadow_att = rtc_shadow_walk(F, ops, tris, over_point, lpos, list, cnt);
      if (sh) sh[li] = shadow_att;
      D3 surface = rtc_lighting(m, point, object_color, lpos, intensity, eye_v, normal_v, shadow_att);
      lsum = (li == 0) ? surface : lsum + surface;
    }
    const double n1 = k[19], n2 = k[20];
    double reflectance;
    {  // Precomputation::schlick (intersect.rs:139-156)
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
    if (P.n_lights != 0 && m.transparency != 0.0) {
      double n_ratio = n1 / n2;
      double cos_i = dot(eye_v, normal_v);
      double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
      if (!(sin2_t > 1.0)) {
        double cos_t = sqrt(1.0 - sin2_t);
        direction = normal_v * (n_ratio * cos_i - cos_t) - eye_v * n_ratio;
        refract = true;
      }
    }
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
    Q.out_att[idx] = rtc_shadow_walk(F, P.ops, P.tris, ld3(Q.points + idx * 3), ld3(Q.light_pos + idx * 3), list, cnt);
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
