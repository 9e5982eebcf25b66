// The host side of the direct-lighting renders (include/rl_render.h "Direct-lighting renders", rl_rtiow_render_direct*; DESIGN.md §3.21;
// kernel: rl_rtiow_direct.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernel is
// instantiated behind every other one).  The four entry forms, the launch and the launch geometry are rl_pixel_render_api.h's; here:
// what is particular to the family.
#pragma once

namespace {
// What is particular to these calls and decided before a device is looked at.  On success `out` holds the lights as the kernel reads
// them: the caller's 12 doubles and nl = u.cross(v) (vec3.rs:48-54; this file is compiled without contraction, every product is rounded).
bool direct_ok(const rl_rtiow_camera *cam, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, const void *direct,
               const void *unshadowed, const void *hit_count, DirectLight *out) {
  if (n_lights == 0 || n_lights > RL_DIRECT_MAX_LIGHTS || !lights || light_samples == 0) return false;
  if (!(seg_tmax > 1e-10) || !(seg_tmax <= 1.0) || (!direct && !unshadowed && !hit_count)) return false;
  if (cam) {  // S L K beyond 32 bits: the counters of a pixel's segments would wrap
    const uint64_t lk = (uint64_t)n_lights * (uint64_t)light_samples;  // < 2^36
    if (lk >= ((uint64_t)1 << 32) || (uint64_t)cam->samples_per_pixel * lk >= ((uint64_t)1 << 32)) return false;
  }
  for (uint32_t l = 0; l < n_lights; l++) {
    const double *p = lights + (size_t)l * 12;
    for (int i = 0; i < 12; i++)
      if (!std::isfinite(p[i])) return false;
    DirectLight &d = out[l];
    for (int i = 0; i < 3; i++) d.Q[i] = p[i], d.u[i] = p[3 + i], d.v[i] = p[6 + i], d.E[i] = p[9 + i];
    d.nl[0] = d.u[1] * d.v[2] - d.u[2] * d.v[1];
    d.nl[1] = d.u[2] * d.v[0] - d.u[0] * d.v[2];
    d.nl[2] = d.u[0] * d.v[1] - d.u[1] * d.v[0];
    if (d.nl[0] == 0.0 && d.nl[1] == 0.0 && d.nl[2] == 0.0) return false;
  }
  return true;
}

// what the calls add to render_check: rl_rtiow_occluded_rays' refusal of media scenes
int direct_rules(const rl_scene *scene) {
  if (scene->rt().has_media)
    return set_err(RL_E_UNSUPPORTED, "ConstantMedium::hit draws from the pixel's RNG stream (constant_medium.rs:55); there is no seeded any-hit for the shadow segments");
  return RL_OK;
}

// what an entry point gives direct_ok, and what direct_ok makes of the lights
struct DirectArgs {
  uint32_t n_lights, light_samples;
  double seg_tmax;
  DirectLight lights[RL_DIRECT_MAX_LIGHTS];
};

// (A.lights is filled here; the callable reads A when it runs, behind every check)
PixelFamily direct_family(const rl_rtiow_camera *cam, const double *lights, void *direct, void *unshadowed, void *hit_count, DirectArgs &A) {
  return {direct_ok(cam, A.n_lights, lights, A.light_samples, A.seg_tmax, direct, unshadowed, hit_count, A.lights),
          direct_rules,
          {{direct, 3 * sizeof(double)}, {unshadowed, 3 * sizeof(double)}, {hit_count, sizeof(uint32_t)}}};
}

// the family's query struct filled from the entry form's target, and the launch
auto direct_run(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const DirectArgs &A) {
  return [=, &A](const PixelTarget &T) -> int {
    DirectQuery Q{};
    Q.n = T.n, Q.xs = (const uint32_t *)T.d_xs, Q.ys = (const uint32_t *)T.d_ys;
    Q.n_lights = A.n_lights, Q.light_samples = A.light_samples, Q.seg_tmax = A.seg_tmax;
    Q.direct = (double *)T.out[0], Q.unshadowed = (double *)T.out[1], Q.hit_count = (uint32_t *)T.out[2];
    for (uint32_t l = 0; l < A.n_lights; l++) Q.lights[l] = A.lights[l];
    return pixel_render_launch(scene, pixel_render_params(scene, cam, first_sample, T, false), Q, rtiow_direct_kernel<FEATURES_NT, true, false, FEATURES_SD>,
                               rtiow_direct_kernel<FEATURES_NT, false, false, FEATURES_SD>, rtiow_direct_kernel<FEATURES_NT, false, true, FEATURES_SD>,
                               LAST_QUERY_DIRECT_REFERENCE, LAST_QUERY_DIRECT_FAST, T);
  };
}
}  // namespace

extern "C" {

int rl_rtiow_render_direct_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_direct, void *d_unshadowed,
                                  void *d_hit_count, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_rows_device(direct_family(cam, lights, d_direct, d_unshadowed, d_hit_count, A), scene, cam, row_first, row_step, hip_stream, st,
                           direct_run(scene, cam, first_sample, A));
}

int rl_rtiow_render_direct_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *direct, double *unshadowed,
                                uint32_t *hit_count, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_rows_host(direct_family(cam, lights, direct, unshadowed, hit_count, A), scene, cam, row_first, row_step, st, direct_run(scene, cam, first_sample, A));
}

int rl_rtiow_render_pixels_direct_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                         uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_direct, void *d_unshadowed,
                                         void *d_hit_count, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_list_device(direct_family(cam, lights, d_direct, d_unshadowed, d_hit_count, A), scene, cam, d_xs, d_ys, n, hip_stream, st,
                           direct_run(scene, cam, first_sample, A));
}

int rl_rtiow_render_pixels_direct(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                  uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *direct, double *unshadowed,
                                  uint32_t *hit_count, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_list_host(direct_family(cam, lights, direct, unshadowed, hit_count, A), scene, cam, xs, ys, n, st, direct_run(scene, cam, first_sample, A));
}

}  // extern "C"
