// Camera::render for both crates, on the GPU through the C ABI of include/rl_render.h: the host-side
// call a maintainer of the reference would add beside the CPU render.
//   rtiow::Camera::render / render_from_checkpoint  <- ray-tracing-one-weekend/src/camera.rs:122,136
//   rtc::Camera::render                              <- ray-tracer-challenge/src/scene/camera.rs:93
#include <stdexcept>
#include <string>

#include "rtc_host.hpp"
#include "rtiow_host.hpp"

namespace rtiow {
Canvas Camera::render_internal(uint64_t samples_already_rendered, const Hittable &world) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  Canvas c{params.samples_per_pixel, params.image_width, image_height, std::vector<double>(params.image_width * image_height * 3)};
  int rc = rl_rtiow_render(sc, &cam, samples_already_rendered, c.data.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render: ") + rl_last_error());
  return c;
}
static Canvas render_independent_impl(const Camera &camera, const Hittable &world, const Canvas *checkpoint) {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_rtiow_camera cam = camera.derived();
  const size_t n = (size_t)cam.image_width * cam.image_height * 3;
  if (checkpoint && (checkpoint->width != cam.image_width || checkpoint->height != cam.image_height || checkpoint->data.size() != n))
    throw std::runtime_error("render_independent_from_checkpoint: size mismatch");
  Canvas c{(checkpoint ? checkpoint->samples : 0) + camera.params.samples_per_pixel, cam.image_width, cam.image_height,
           checkpoint ? checkpoint->data : std::vector<double>(n)};
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  int rc = rl_rtiow_render_independent_rows(sc, &cam, checkpoint ? checkpoint->samples : 0, 0, 1, checkpoint ? 1u : 0u, c.data.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_independent_rows: ") + rl_last_error());
  return c;
}
std::vector<double> Camera::render_pixels(const Hittable &world, const uint32_t *xs, const uint32_t *ys, size_t n, uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  std::vector<double> out(n * 3);
  int rc = rl_rtiow_render_pixels(sc, &cam, first_sample, xs, ys, n, out.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_pixels: ") + rl_last_error());
  return out;
}
Camera::Moments Camera::render_moments(const Hittable &world, uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  const size_t n = params.image_width * image_height * 3;
  Moments m{params.samples_per_pixel, std::vector<double>(n), std::vector<double>(n)};
  int rc = rl_rtiow_render_moments_rows(sc, &cam, first_sample, 0, 1, m.sums.data(), m.sq.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_moments_rows: ") + rl_last_error());
  return m;
}
Camera::Moments Camera::render_pixels_moments(const Hittable &world, const uint32_t *xs, const uint32_t *ys, size_t n, uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  Moments m{params.samples_per_pixel, std::vector<double>(n * 3), std::vector<double>(n * 3)};
  int rc = rl_rtiow_render_pixels_moments(sc, &cam, first_sample, xs, ys, n, m.sums.data(), m.sq.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_pixels_moments: ") + rl_last_error());
  return m;
}
Camera::Adaptive Camera::render_adaptive(const Hittable &world, const rl_rtiow_adaptive &rule, uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  const size_t n = params.image_width * image_height;
  Adaptive a{std::vector<double>(n * 3), std::vector<double>(n * 3), std::vector<uint32_t>(n)};
  int rc = rl_rtiow_render_adaptive_rows(sc, &cam, first_sample, 0, 1, &rule, a.sums.data(), a.sq.data(), a.counts.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_adaptive_rows: ") + rl_last_error());
  return a;
}
Camera::Features Camera::render_features(const Hittable &world, uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  const size_t n = params.image_width * image_height;
  Features ft{params.samples_per_pixel, std::vector<double>(n * 3), std::vector<double>(n * 3), std::vector<double>(n), std::vector<uint32_t>(n)};
  const rl_rtiow_features out{ft.albedo_sum.data(), ft.normal_sum.data(), ft.depth_sum.data(), ft.hit_count.data()};
  int rc = rl_rtiow_render_features_rows(sc, &cam, first_sample, 0, 1, &out, nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_features_rows: ") + rl_last_error());
  return ft;
}
Camera::AmbientOcclusion Camera::render_ao(const Hittable &world, uint32_t ao_rays, double radius, uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  const size_t n = params.image_width * image_height;
  AmbientOcclusion ao{ao_rays, std::vector<uint32_t>(n), std::vector<uint32_t>(n)};
  int rc = rl_rtiow_render_ao_rows(sc, &cam, first_sample, 0, 1, ao_rays, radius, ao.open_count.data(), ao.hit_count.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_ao_rows: ") + rl_last_error());
  return ao;
}
Camera::DirectLight Camera::render_direct(const Hittable &world, const std::vector<QuadLight> &lights, uint32_t light_samples, double seg_tmax,
                                          uint64_t first_sample) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  const size_t n = params.image_width * image_height;
  std::vector<double> packed;  // [L][12]: Q, u, v, E
  for (const QuadLight &l : lights)
    for (const Vec3 *v : {&l.q, &l.u, &l.v, &l.emit}) packed.insert(packed.end(), v->e, v->e + 3);
  DirectLight dl{light_samples, std::vector<double>(3 * n), std::vector<double>(3 * n), std::vector<uint32_t>(n)};
  int rc = rl_rtiow_render_direct_rows(sc, &cam, first_sample, 0, 1, (uint32_t)std::min<size_t>(lights.size(), 0xFFFFFFFFu), packed.data(), light_samples, seg_tmax,
                                       dl.direct.data(), dl.unshadowed.data(), dl.hit_count.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_render_direct_rows: ") + rl_last_error());
  return dl;
}
Camera::Moments Camera::render_nee(const Hittable &world, const std::vector<QuadLight> &lights, uint32_t light_samples, double seg_tmax,
                                   uint64_t first_sample) const {
  return nee_moments(world, lights, light_samples, seg_tmax, first_sample, nullptr);
}
Camera::Moments Camera::render_nee_mis(const Hittable &world, const std::vector<QuadLight> &lights, uint32_t light_samples, double seg_tmax,
                                       MisHeuristic heuristic, uint64_t first_sample) const {
  const uint32_t h = (uint32_t)heuristic;
  return nee_moments(world, lights, light_samples, seg_tmax, first_sample, &h);
}
Camera::Moments Camera::render_nee_mis(const Hittable &world, const std::vector<QuadLight> &lights, const std::vector<SphereLight> &sphere_lights,
                                       uint32_t light_samples, double seg_tmax, MisHeuristic heuristic, uint64_t first_sample) const {
  const uint32_t h = (uint32_t)heuristic;
  return nee_moments(world, lights, light_samples, seg_tmax, first_sample, &h, &sphere_lights);
}
// heuristic == null: rl_rtiow_render_nee_rows, else rl_rtiow_render_nee_mis_rows, or with sphere_lights rl_rtiow_render_nee_mis_spheres_rows
Camera::Moments Camera::nee_moments(const Hittable &world, const std::vector<QuadLight> &lights, uint32_t light_samples, double seg_tmax, uint64_t first_sample,
                                    const uint32_t *heuristic, const std::vector<SphereLight> *sphere_lights) const {
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  rl_rtiow_camera cam = derived();
  const size_t n = params.image_width * image_height;
  std::vector<double> packed;  // [L][12]: Q, u, v, E
  for (const QuadLight &l : lights)
    for (const Vec3 *v : {&l.q, &l.u, &l.v, &l.emit}) packed.insert(packed.end(), v->e, v->e + 3);
  Moments m{params.samples_per_pixel, std::vector<double>(3 * n), std::vector<double>(3 * n)};
  const uint32_t n_lights = (uint32_t)std::min<size_t>(lights.size(), 0xFFFFFFFFu);
  std::vector<double> spheres;  // [Ls][7]: C, r, E
  for (size_t j = 0; sphere_lights && j < sphere_lights->size(); j++) {
    const SphereLight &l = (*sphere_lights)[j];
    spheres.insert(spheres.end(), l.center.e, l.center.e + 3);
    spheres.push_back(l.radius);
    spheres.insert(spheres.end(), l.emit.e, l.emit.e + 3);
  }
  const uint32_t n_spheres = sphere_lights ? (uint32_t)std::min<size_t>(sphere_lights->size(), 0xFFFFFFFFu) : 0u;
  const char *call = sphere_lights ? "rl_rtiow_render_nee_mis_spheres_rows: " : heuristic ? "rl_rtiow_render_nee_mis_rows: " : "rl_rtiow_render_nee_rows: ";
  int rc = sphere_lights ? rl_rtiow_render_nee_mis_spheres_rows(sc, &cam, first_sample, 0, 1, n_lights, packed.data(), n_spheres, spheres.data(), light_samples, seg_tmax,
                                                                *heuristic, m.sums.data(), m.sq.data(), nullptr)
           : heuristic ? rl_rtiow_render_nee_mis_rows(sc, &cam, first_sample, 0, 1, n_lights, packed.data(), light_samples, seg_tmax, *heuristic, m.sums.data(),
                                                      m.sq.data(), nullptr)
                       : rl_rtiow_render_nee_rows(sc, &cam, first_sample, 0, 1, n_lights, packed.data(), light_samples, seg_tmax, m.sums.data(), m.sq.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string(call) + rl_last_error());
  return m;
}
Denoised denoise_atrous(size_t width, size_t height, uint32_t iterations, const rl_atrous_params &params, const std::vector<double> &color,
                        const std::vector<double> &variance, const std::vector<double> &guides) {
  const size_t n = width * height;
  if (width > UINT32_MAX || height > UINT32_MAX || color.size() != n * 3 || variance.size() != n * 3 || guides.size() != n * params.n_guides)
    throw std::runtime_error("denoise_atrous: size mismatch");
  Denoised d{std::vector<double>(n * 3), std::vector<double>(n * 3)};
  int rc = rl_denoise_atrous((uint32_t)width, (uint32_t)height, iterations, &params, color.data(), variance.data(), params.n_guides ? guides.data() : nullptr,
                             d.color.data(), d.variance.data());
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_denoise_atrous: ") + rl_last_error());
  return d;
}
static Denoised denoise_render_impl(size_t width, size_t height, const std::vector<double> &sums, const std::vector<double> &sq, const std::vector<uint32_t> *counts,
                                    size_t samples, const Camera::Features &f, uint32_t want, uint32_t iterations, const rl_atrous_params &params) {
  const size_t n = width * height;
  const bool normal = want & RL_GUIDE_NORMAL, depth = want & RL_GUIDE_DEPTH, hits = want & (RL_GUIDE_DEPTH | RL_GUIDE_COVERAGE);
  if (width > UINT32_MAX || height > UINT32_MAX || samples > UINT32_MAX || f.samples > UINT32_MAX || sums.size() != n * 3 || sq.size() != n * 3 ||
      (counts && counts->size() != n) || f.albedo_sum.size() != n * 3 || (normal && f.normal_sum.size() != n * 3) || (depth && f.depth_sum.size() != n) ||
      (hits && f.hit_count.size() != n))
    throw std::runtime_error("denoise_render: size mismatch");
  rl_denoise_inputs in{};
  in.sums = sums.data(), in.sq = sq.data(), in.counts = counts ? counts->data() : nullptr, in.albedo_sum = f.albedo_sum.data();
  in.normal_sum = normal ? f.normal_sum.data() : nullptr, in.depth_sum = depth ? f.depth_sum.data() : nullptr, in.hit_count = hits ? f.hit_count.data() : nullptr;
  in.samples = (uint32_t)samples, in.feature_samples = (uint32_t)f.samples, in.want = want;
  Denoised d{std::vector<double>(n * 3), std::vector<double>(n * 3)};
  int rc = rl_denoise_render((uint32_t)width, (uint32_t)height, &in, iterations, &params, d.color.data(), d.variance.data(), nullptr);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_denoise_render: ") + rl_last_error());
  return d;
}
Denoised denoise_render(size_t width, size_t height, const Camera::Moments &estimate, const Camera::Features &features, uint32_t want, uint32_t iterations,
                        const rl_atrous_params &params) {
  return denoise_render_impl(width, height, estimate.sums, estimate.sq, nullptr, estimate.samples, features, want, iterations, params);
}
Denoised denoise_render(size_t width, size_t height, const Camera::Adaptive &estimate, const Camera::Features &features, uint32_t want, uint32_t iterations,
                        const rl_atrous_params &params) {
  return denoise_render_impl(width, height, estimate.sums, estimate.sq, &estimate.counts, 0, features, want, iterations, params);
}
Canvas Camera::render_independent(const Hittable &world) const { return render_independent_impl(*this, world, nullptr); }
Canvas Camera::render_independent_from_checkpoint(const Hittable &world, const Canvas &checkpoint) const {
  return render_independent_impl(*this, world, &checkpoint);
}
std::vector<rl_rtiow_hit> hit(const Hittable &world, const rl_ray *rays, size_t n, Interval ray_t) {  // hittable/mod.rs:42
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  std::vector<rl_rtiow_hit> out(n);
  int rc = rl_rtiow_hit_rays(sc, rays, n, ray_t.min, ray_t.max, out.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtiow_hit_rays: ") + rl_last_error());
  return out;
}
std::vector<uint8_t> occluded_rays(const Hittable &world, const rl_ray *rays, size_t n, Interval ray_t) {  // hittable/mod.rs:42 .is_some()
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  std::vector<uint8_t> out(n);
  int rc = rl_rtiow_occluded_rays(sc, rays, n, ray_t.min, ray_t.max, out.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtiow_occluded_rays: ") + rl_last_error());
  return out;
}
std::vector<rl_rtiow_hit> hit_rays_seeded(const Hittable &world, const rl_ray *rays, rl_rng_cursor *cursors, size_t n, uint64_t seed,
                                          Interval ray_t) {  // hittable/mod.rs:42 with constant_medium.rs:27-80
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  std::vector<rl_rtiow_hit> out(n);
  int rc = rl_rtiow_hit_rays_seeded(sc, rays, cursors, n, seed, ray_t.min, ray_t.max, out.data(), cursors, nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtiow_hit_rays_seeded: ") + rl_last_error());
  return out;
}
std::vector<double> ray_color_rays(const Hittable &world, const rl_ray *rays, rl_rng_cursor *cursors, size_t n, uint64_t seed, size_t max_depth,
                                   const Color &background, std::vector<uint32_t> *ray_counts) {  // camera.rs:232-260
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  std::vector<double> out(n * 3);
  if (ray_counts) ray_counts->assign(n, 0u);
  const double bg[3] = {background.x(), background.y(), background.z()};
  int rc = rl_rtiow_ray_color_rays(sc, rays, cursors, n, seed, (uint32_t)max_depth, bg, out.data(), cursors, ray_counts ? ray_counts->data() : nullptr, nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtiow_ray_color_rays: ") + rl_last_error());
  return out;
}
std::vector<rl_rtiow_scatter> scatter(const Hittable &world, const rl_ray *rays, const rl_rtiow_hit *hits, rl_rng_cursor *cursors, size_t n,
                                      uint64_t seed) {  // material.rs:11-20
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  std::vector<rl_rtiow_scatter> out(n);
  int rc = rl_rtiow_scatter_rays(sc, rays, hits, cursors, n, seed, out.data(), cursors, nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtiow_scatter_rays: ") + rl_last_error());
  return out;
}
std::vector<double> texture_values(const Hittable &world, const uint32_t *textures, const double *uv, const double *p, size_t n) {  // texture.rs
  Flattened f;
  f.root = world.flatten(f);
  rl_rtiow_scene_desc d = f.desc();
  rl_scene *sc = rl_rtiow_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtiow_scene_create: ") + rl_last_error());
  std::vector<double> out(n * 3);
  int rc = rl_rtiow_texture_values(sc, textures, uv, p, n, out.data());
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_texture_values: ") + rl_last_error());
  return out;
}
std::vector<rl_ray> Camera::get_rays(const uint32_t *px, const uint32_t *py, rl_rng_cursor *cursors, size_t n) const {  // camera.rs:203-216
  rl_rtiow_camera cam = derived();
  std::vector<rl_ray> out(n);
  int rc = rl_rtiow_camera_rays(&cam, n, px, py, cursors, out.data(), cursors);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtiow_camera_rays: ") + rl_last_error());
  return out;
}
Canvas Camera::render(const Hittable &world) const { return render_internal(0, world); }  // camera.rs:122
Canvas Camera::render_from_checkpoint(const Hittable &world, const Canvas &checkpoint) const {  // camera.rs:136-143
  return render_internal(checkpoint.samples, world).merge(checkpoint);
}
}  // namespace rtiow

namespace rtc {
Canvas Camera::render(const World &world, const RenderOpts &opts) const {  // scene/camera.rs:93
  Flattened f;
  world.flatten(f);
  rl_rtc_scene_desc d = f.desc();
  rl_scene *sc = rl_rtc_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtc_scene_create: ") + rl_last_error());
  rl_rtc_camera cam = derived();
  Canvas c{hsize, vsize, std::vector<double>(hsize * vsize * 3)};
  int rc = rl_rtc_render(sc, &cam, (uint32_t)opts.anti_aliasing_samples, c.data.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtc_render: ") + rl_last_error());
  return c;
}
std::vector<double> Camera::render_pixels(const World &world, const RenderOpts &opts, const uint32_t *xs, const uint32_t *ys, size_t n) const {
  Flattened f;
  world.flatten(f);
  rl_rtc_scene_desc d = f.desc();
  rl_scene *sc = rl_rtc_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtc_scene_create: ") + rl_last_error());
  rl_rtc_camera cam = derived();
  std::vector<double> out(n * 3);
  int rc = rl_rtc_render_pixels(sc, &cam, (uint32_t)opts.anti_aliasing_samples, xs, ys, n, out.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtc_render_pixels: ") + rl_last_error());
  return out;
}
std::vector<double> World::color_at(const rl_ray *rays, size_t n) const {  // world.rs:100
  Flattened f;
  flatten(f);
  rl_rtc_scene_desc d = f.desc();
  rl_scene *sc = rl_rtc_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtc_scene_create: ") + rl_last_error());
  std::vector<double> out(n * 3);
  int rc = rl_rtc_color_at_rays(sc, rays, n, out.data(), nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtc_color_at_rays: ") + rl_last_error());
  return out;
}
std::vector<uint32_t> World::intersect(const rl_ray *rays, size_t n, uint32_t k, std::vector<rl_rtc_isect> *isects,
                                       std::vector<uint32_t> *hit_index) const {  // world.rs:46, intersect.rs:159
  Flattened f;
  flatten(f);
  rl_rtc_scene_desc d = f.desc();
  rl_scene *sc = rl_rtc_scene_create(&d);
  if (!sc) throw std::runtime_error(std::string("rl_rtc_scene_create: ") + rl_last_error());
  std::vector<uint32_t> counts(n);
  const bool want = isects && k > 0;
  if (want) isects->assign(n * k, rl_rtc_isect{});
  if (hit_index) hit_index->assign(n, 0u);
  int rc = rl_rtc_intersect_rays(sc, rays, n, want ? k : 0u, want ? isects->data() : nullptr, counts.data(), hit_index ? hit_index->data() : nullptr,
                                 nullptr);
  rl_scene_destroy(sc);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtc_intersect_rays: ") + rl_last_error());
  return counts;
}
namespace {
struct SceneGuard {  // the flattened world on the device for one query
  rl_scene *sc;
  explicit SceneGuard(const World &w) {
    Flattened f;
    w.flatten(f);
    rl_rtc_scene_desc d = f.desc();
    sc = rl_rtc_scene_create(&d);
    if (!sc) throw std::runtime_error(std::string("rl_rtc_scene_create: ") + rl_last_error());
  }
  ~SceneGuard() { rl_scene_destroy(sc); }
  SceneGuard(const SceneGuard &) = delete;
  SceneGuard &operator=(const SceneGuard &) = delete;
};
}  // namespace
std::vector<rl_rtc_comps> World::prepare(const rl_ray *rays, size_t n) const {  // intersect.rs:159-168, :48-115
  SceneGuard g(*this);
  std::vector<rl_rtc_comps> out(n);
  int rc = rl_rtc_prepare_rays(g.sc, rays, n, out.data(), nullptr);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtc_prepare_rays: ") + rl_last_error());
  return out;
}
std::vector<rl_rtc_shade> World::shade(const rl_rtc_comps *comps, size_t n, std::vector<double> *shadow) const {  // world.rs:57-87
  SceneGuard g(*this);
  std::vector<rl_rtc_shade> out(n);
  if (shadow) shadow->assign(n * lights.size(), 0.0);
  int rc = rl_rtc_shade_hits(g.sc, comps, n, out.data(), shadow && !shadow->empty() ? shadow->data() : nullptr, nullptr);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtc_shade_hits: ") + rl_last_error());
  return out;
}
std::vector<double> World::shadow_attenuation(const double *points, const double *light_positions, size_t n) const {  // world.rs:104-126
  SceneGuard g(*this);
  std::vector<double> out(n);
  int rc = rl_rtc_shadow_attenuation(g.sc, points, light_positions, n, out.data(), nullptr);
  if (rc != RL_OK && rc != RL_E_DEGENERATE) throw std::runtime_error(std::string("rl_rtc_shadow_attenuation: ") + rl_last_error());
  return out;
}
std::vector<double> World::lighting(const rl_rtc_comps *comps, const double *light_positions, const double *light_intensities,
                                    const double *shadow_att, size_t n) const {  // material.rs:54-90
  SceneGuard g(*this);
  std::vector<double> out(n * 3);
  int rc = rl_rtc_lighting(g.sc, comps, light_positions, light_intensities, shadow_att, n, out.data());
  if (rc != RL_OK) throw std::runtime_error(std::string("rl_rtc_lighting: ") + rl_last_error());
  return out;
}
}  // namespace rtc
