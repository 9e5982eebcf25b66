// The steps of World::color_at (ray-tracer-challenge/src/scene/world.rs:57-159) that work on points and vectors alone, each written once
// for every RTC kernel: the triangle kernel (rl_rtc_render_body.inc: rtc_lighting), the color_at body of the full kernel and of
// rtc_color_at_rays_kernel (rl_rtc_color_at_body.inc) and the shading queries (rl_rtc_shade_query.h).  The steps that read a ray's Ent
// list (rtc_first_hit, rtc_refractive_indices, rtc_shadow_product, rtc_shadow_walk) stand next to that list in rl_rtc_full_kernel.h.
// No scene and no counters in here: D3 (rl_device.h) and rl_rtc_material are all these need, so rl_rtc_kernel.h includes it first.
// -ffp-contract=off: an expression here gives the same bits in every caller, which tests/test_gpu_rtc_shade_query.py pins.
#pragma once
#include "rl_device.h"

namespace rl {

__device__ __forceinline__ double mag(D3 v) { return sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }  // vector.rs:32
// vector.rs:36-43 / 142-156: TRUE division by the magnitude; false when the magnitude is 0
__device__ __forceinline__ bool norm(D3 v, D3 &out) {
  double m = mag(v);
  if (m == 0.0) return false;
  out = D3{v.x / m, v.y / m, v.z / m};
  return true;
}
__device__ __forceinline__ D3 reflect(D3 v, D3 n) { return v - (n * 2.0) * dot(v, n); }  // vector.rs:57-59

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

// Intersection::prepare_computations (intersect.rs:48-71) up to the containers walk.  `flagged` counts the two fallbacks the reference
// has no case for: a ray or a reflection of zero length, which it would normalise to NaN.
struct RtcComps {
  D3 point, eye_v, normal_v, over_point, under_point, reflect_v;
  bool inside;
};
__device__ __forceinline__ RtcComps rtc_prepare_computations(D3 origin, D3 dir, double t, D3 normal, unsigned long long &flagged) {
  RtcComps k;
  k.point = origin + dir * t;
  if (!norm(-dir, k.eye_v)) {
    flagged++;
    k.eye_v = -dir;
  }
  k.normal_v = normal;
  k.inside = dot(k.normal_v, k.eye_v) < 0.0;
  if (k.inside) k.normal_v = -k.normal_v;
  k.over_point = k.point + k.normal_v * 1e-5;
  k.under_point = k.point - k.normal_v * 1e-5;
  if (!norm(reflect(dir, k.normal_v), k.reflect_v)) {
    flagged++;
    k.reflect_v = dir;
  }
  return k;
}

// Precomputation::schlick (intersect.rs:139-156)
__device__ __forceinline__ double rtc_schlick(D3 eye_v, D3 normal_v, double n1, double n2) {
  double cosv = dot(eye_v, normal_v);
  double nn = n1 / n2;
  double sin2_t = nn * nn * (1.0 - cosv * cosv);
  double cos_t = sqrt(1.0 - sin2_t);
  double cos_adj = nn > 1.0 ? cos_t : cosv;
  if (sin2_t > 1.0 && nn > 1.0) return 1.0;
  double q = (n1 - n2) / (n1 + n2);
  double r0 = q * q;
  double x = 1.0 - cos_adj;
  double x2 = x * x;
  return r0 + (1.0 - r0) * (x * (x2 * x2));
}

// The refracted ray's direction (world.rs:141-159); false on total internal reflection, `direction` then untouched
__device__ __forceinline__ bool rtc_refracted_direction(D3 eye_v, D3 normal_v, double n1, double n2, D3 &direction) {
  double n_ratio = n1 / n2;
  double cos_i = dot(eye_v, normal_v);
  double sin2_t = n_ratio * n_ratio * (1.0 - cos_i * cos_i);
  if (sin2_t > 1.0) return false;
  double cos_t = sqrt(1.0 - sin2_t);
  direction = normal_v * (n_ratio * cos_i - cos_t) - eye_v * n_ratio;
  return true;
}

}  // namespace rl
