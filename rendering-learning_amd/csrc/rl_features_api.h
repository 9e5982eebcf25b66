// The host side of the feature renders (include/rl_render.h "Feature renders", rl_rtiow_render_features*; kernel:
// rl_rtiow_features.h).  Not a translation unit of its own: rl_render.hip includes it once, behind rl_pixel_render_api.h, which has the
// four entry forms, the launch and the launch geometry of every pixel render.  Here: what is particular to the family.
#pragma once

namespace {
// NULL, or no output asked for: refused before anything else is looked at
bool features_ok(const rl_rtiow_features *f) { return f && (f->albedo_sum || f->normal_sum || f->depth_sum || f->hit_count); }

PixelFamily features_family(const rl_rtiow_features *f) {
  if (!features_ok(f)) return {false, nullptr, {}};
  return {true, nullptr, {{f->albedo_sum, 3 * sizeof(double)}, {f->normal_sum, 3 * sizeof(double)}, {f->depth_sum, sizeof(double)}, {f->hit_count, sizeof(uint32_t)}}};
}

// the family's query struct filled from the entry form's target, and the launch
auto features_run(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample) {
  return [=](const PixelTarget &T) -> int {
    FeaturesQuery Q{};
    Q.n = T.n, Q.xs = (const uint32_t *)T.d_xs, Q.ys = (const uint32_t *)T.d_ys;
    Q.albedo_sum = (double *)T.out[0], Q.normal_sum = (double *)T.out[1], Q.depth_sum = (double *)T.out[2], Q.hit_count = (uint32_t *)T.out[3];
    return pixel_render_launch(scene, pixel_render_params(scene, cam, first_sample, T, true), Q, rtiow_features_kernel<FEATURES_NT, true, false, FEATURES_SD>,
                               rtiow_features_kernel<FEATURES_NT, false, false, FEATURES_SD>, rtiow_features_kernel<FEATURES_NT, false, true, FEATURES_SD>,
                               LAST_QUERY_FEATURES_REFERENCE, LAST_QUERY_FEATURES_FAST, T);
  };
}
}  // namespace

extern "C" {

// the most lanes one feature launch has on the current device: a frame or list beyond it puts several pixels through one lane
unsigned long long rl_debug_features_lanes(void) { return (unsigned long long)std::max(1, g_cus) * FEATURES_MAX_BLOCKS_PER_CU * FEATURES_NT; }

int rl_rtiow_render_features_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                    const rl_rtiow_features *d_out, void *hip_stream, rl_stats *st) {
  return pixel_rows_device(features_family(d_out), scene, cam, row_first, row_step, hip_stream, st, features_run(scene, cam, first_sample));
}

int rl_rtiow_render_features_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  const rl_rtiow_features *out, rl_stats *st) {
  return pixel_rows_host(features_family(out), scene, cam, row_first, row_step, st, features_run(scene, cam, first_sample));
}

int rl_rtiow_render_pixels_features_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                           const rl_rtiow_features *d_out, void *hip_stream, rl_stats *st) {
  return pixel_list_device(features_family(d_out), scene, cam, d_xs, d_ys, n, hip_stream, st, features_run(scene, cam, first_sample));
}

int rl_rtiow_render_pixels_features(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                    const rl_rtiow_features *out, rl_stats *st) {
  return pixel_list_host(features_family(out), scene, cam, xs, ys, n, st, features_run(scene, cam, first_sample));
}

}  // extern "C"
