// The host side of the ambient-occlusion renders (include/rl_render.h "Ambient-occlusion renders", rl_rtiow_render_ao*; DESIGN.md §3.20;
// kernel: rl_rtiow_ao.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernel is
// instantiated behind every other one).  The four entry forms, the launch and the launch geometry are rl_pixel_render_api.h's; here:
// what is particular to the family.
#pragma once

namespace {
// What is particular to these calls and decided before a device is looked at: K = 0, S K beyond 32 bits (open_count could wrap), a
// radius that is NaN or not positive, no output asked for.
bool ao_ok(const rl_rtiow_camera *cam, uint32_t ao_rays, double radius, const void *open_count, const void *hit_count) {
  if (ao_rays == 0 || !(radius > 0.0) || (!open_count && !hit_count)) return false;
  return !cam || (uint64_t)cam->samples_per_pixel * (uint64_t)ao_rays < ((uint64_t)1 << 32);
}

// what the calls add to render_check: rl_rtiow_occluded_rays' refusal of media scenes
int ao_rules(const rl_scene *scene) {
  if (scene->rt().has_media)
    return set_err(RL_E_UNSUPPORTED, "ConstantMedium::hit draws from the pixel's RNG stream (constant_medium.rs:55); there is no seeded any-hit for the ambient rays");
  return RL_OK;
}

PixelFamily ao_family(const rl_rtiow_camera *cam, uint32_t ao_rays, double radius, void *open_count, void *hit_count) {
  return {ao_ok(cam, ao_rays, radius, open_count, hit_count), ao_rules, {{open_count, sizeof(uint32_t)}, {hit_count, sizeof(uint32_t)}}};
}

// the family's query struct filled from the entry form's target, and the launch
auto ao_run(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t ao_rays, double radius) {
  return [=](const PixelTarget &T) -> int {
    AoQuery Q{};
    Q.n = T.n, Q.xs = (const uint32_t *)T.d_xs, Q.ys = (const uint32_t *)T.d_ys;
    Q.ao_rays = ao_rays, Q.radius = radius, Q.open_count = (uint32_t *)T.out[0], Q.hit_count = (uint32_t *)T.out[1];
    return pixel_render_launch(scene, pixel_render_params(scene, cam, first_sample, T, false), Q, rtiow_ao_kernel<FEATURES_NT, true, false, FEATURES_SD>,
                               rtiow_ao_kernel<FEATURES_NT, false, false, FEATURES_SD>, rtiow_ao_kernel<FEATURES_NT, false, true, FEATURES_SD>,
                               LAST_QUERY_AO_REFERENCE, LAST_QUERY_AO_FAST, T);
  };
}
}  // namespace

extern "C" {

int rl_rtiow_render_ao_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t ao_rays,
                              double radius, void *d_open_count, void *d_hit_count, void *hip_stream, rl_stats *st) {
  return pixel_rows_device(ao_family(cam, ao_rays, radius, d_open_count, d_hit_count), scene, cam, row_first, row_step, hip_stream, st,
                           ao_run(scene, cam, first_sample, ao_rays, radius));
}

int rl_rtiow_render_ao_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t ao_rays,
                            double radius, uint32_t *open_count, uint32_t *hit_count, rl_stats *st) {
  return pixel_rows_host(ao_family(cam, ao_rays, radius, open_count, hit_count), scene, cam, row_first, row_step, st,
                         ao_run(scene, cam, first_sample, ao_rays, radius));
}

int rl_rtiow_render_pixels_ao_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                     uint32_t ao_rays, double radius, void *d_open_count, void *d_hit_count, void *hip_stream, rl_stats *st) {
  return pixel_list_device(ao_family(cam, ao_rays, radius, d_open_count, d_hit_count), scene, cam, d_xs, d_ys, n, hip_stream, st,
                           ao_run(scene, cam, first_sample, ao_rays, radius));
}

int rl_rtiow_render_pixels_ao(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                              uint32_t ao_rays, double radius, uint32_t *open_count, uint32_t *hit_count, rl_stats *st) {
  return pixel_list_host(ao_family(cam, ao_rays, radius, open_count, hit_count), scene, cam, xs, ys, n, st, ao_run(scene, cam, first_sample, ao_rays, radius));
}

}  // extern "C"
