// Stand-alone host check of the batched queries' 24 entry points and the 14 render entry points with rl_render_status and
// rl_rtiow_render_progress (include/rl_render.h; csrc/rl_query_api.h, csrc/rl_host_api.h) on a machine without a GPU: every form must
// return RL_E_NO_DEVICE before it touches a buffer or opt_stats — with valid buffers, with nothing to do (n = 0; an image whose row_first
// equals its height) and with every pointer NULL.  Meant to be built with the host sanitizers (the library's host code and this file; no
// Python involved):
//   cd rendering-learning_amd/csrc && for f in rl_render.hip rl_multi.hip rl_bvh_build.hip rl_program.cpp rl_fast_bvh.cpp rl_scene_host.cpp; do
//     hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -fPIC -ffp-contract=off -Xarch_host -fsanitize=address,undefined -c -o /tmp/san_${f%.*}.o $f; done
//   clang++ -std=c++17 -g -fsanitize=address,undefined -I../../include -c -o /tmp/san_main.o ../../tools/query_nodevice.cpp
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined -o /tmp/query_nodevice /tmp/san_*.o -ldl && /tmp/query_nodevice
#include <cstdio>
#include <cstring>
#include <vector>

#include "rl_render.h"

#define EXPECT(call, want)                                                  \
  do {                                                                      \
    int rc_ = (call);                                                       \
    calls++;                                                                \
    if (rc_ != (want)) {                                                    \
      std::printf("FAIL %s = %d, expected %d (%s)\n", #call, rc_, (want), rl_last_error()); \
      failures++;                                                           \
    }                                                                       \
  } while (0)

int main() {
  int failures = 0, calls = 0;
  if (rl_init(-1) == RL_OK) {
    std::printf("a device is present: the no-device paths are not reachable, nothing checked\n");
    return 0;
  }
  const uint64_t n = 3;
  const uint32_t k = 2;
  const double inf = 1.0 / 0.0, bg[3] = {0.5, 0.7, 1.0};
  rl_rtiow_camera cam{};
  cam.image_width = 8, cam.image_height = 8, cam.samples_per_pixel = 1, cam.max_depth = 5;
  std::vector<rl_ray> rays(n);
  std::vector<rl_rtiow_hit> hits(n);
  std::vector<rl_rtc_isect> isects(n * k);
  std::vector<rl_rng_cursor> cur(n), cur2(n);
  std::vector<rl_rtiow_scatter> scat(n);
  std::vector<rl_rtc_comps> comps(n);
  std::vector<rl_rtc_shade> shade(n);
  std::vector<uint32_t> u32a(n), u32b(n);
  std::vector<double> v2(n * 2), v3(n * 3), att(n, 1.0), rgb(n * 3), shadow(n);
  rl_stats st;
  for (int with_stats = 0; with_stats < 2; with_stats++) {
    rl_stats *s = with_stats ? &st : nullptr;
    for (uint64_t m : {n, (uint64_t)0}) {  // valid buffers; the empty batch
      // batched ray queries
      EXPECT(rl_rtiow_hit_rays(nullptr, rays.data(), m, 1e-10, inf, hits.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_hit_rays_device(nullptr, rays.data(), m, 1e-10, inf, hits.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_intersect_rays(nullptr, rays.data(), m, k, isects.data(), u32a.data(), u32b.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_intersect_rays(nullptr, rays.data(), m, 0, nullptr, u32a.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_intersect_rays_device(nullptr, rays.data(), m, k, isects.data(), u32a.data(), u32b.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_color_at_rays(nullptr, rays.data(), m, rgb.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_color_at_rays_device(nullptr, rays.data(), m, rgb.data(), nullptr, s), RL_E_NO_DEVICE);
      // seeded path queries
      EXPECT(rl_rtiow_ray_color_rays(nullptr, rays.data(), cur.data(), m, 1, 5, bg, rgb.data(), cur2.data(), u32a.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_ray_color_rays(nullptr, rays.data(), cur.data(), m, 1, 5, bg, rgb.data(), nullptr, nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_ray_color_rays_device(nullptr, rays.data(), cur.data(), m, 1, 5, bg, rgb.data(), cur2.data(), u32a.data(), nullptr, s), RL_E_NO_DEVICE);
      // material queries
      EXPECT(rl_rtiow_scatter_rays(nullptr, rays.data(), hits.data(), cur.data(), m, 1, scat.data(), cur2.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_scatter_rays(nullptr, rays.data(), hits.data(), cur.data(), m, 1, scat.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_scatter_rays_device(nullptr, rays.data(), hits.data(), cur.data(), m, 1, scat.data(), cur2.data(), nullptr, s), RL_E_NO_DEVICE);
      // seeded hit queries
      EXPECT(rl_rtiow_hit_rays_seeded(nullptr, rays.data(), cur.data(), m, 1, 1e-10, inf, hits.data(), cur2.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_hit_rays_seeded(nullptr, rays.data(), cur.data(), m, 1, 1e-10, inf, hits.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtiow_hit_rays_seeded_device(nullptr, rays.data(), cur.data(), m, 1, 1e-10, inf, hits.data(), cur2.data(), nullptr, s), RL_E_NO_DEVICE);
      // RTC shading queries
      EXPECT(rl_rtc_prepare_rays(nullptr, rays.data(), m, comps.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_prepare_rays_device(nullptr, rays.data(), m, comps.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shade_hits(nullptr, comps.data(), m, shade.data(), shadow.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shade_hits(nullptr, comps.data(), m, shade.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shade_hits_device(nullptr, comps.data(), m, shade.data(), shadow.data(), nullptr, s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shadow_attenuation(nullptr, v3.data(), v3.data(), m, att.data(), s), RL_E_NO_DEVICE);
      EXPECT(rl_rtc_shadow_attenuation_device(nullptr, v3.data(), v3.data(), m, att.data(), nullptr, s), RL_E_NO_DEVICE);
    }
  }
  for (uint64_t m : {n, (uint64_t)0}) {  // the forms without opt_stats
    EXPECT(rl_rtiow_camera_rays(&cam, m, u32a.data(), u32b.data(), cur.data(), rays.data(), cur2.data()), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_camera_rays_device(&cam, m, u32a.data(), u32b.data(), cur.data(), rays.data(), cur2.data(), nullptr), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_texture_values(nullptr, u32a.data(), v2.data(), v3.data(), m, rgb.data()), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_texture_values_device(nullptr, u32a.data(), v2.data(), v3.data(), m, rgb.data(), nullptr), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_lighting(nullptr, comps.data(), v3.data(), v3.data(), att.data(), m, rgb.data()), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_lighting_device(nullptr, comps.data(), v3.data(), v3.data(), att.data(), m, rgb.data(), nullptr), RL_E_NO_DEVICE);
  }
  // every pointer NULL, n > 0
  EXPECT(rl_rtiow_hit_rays(nullptr, nullptr, n, 1e-10, inf, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_hit_rays_device(nullptr, nullptr, n, 1e-10, inf, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_intersect_rays(nullptr, nullptr, n, k, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_intersect_rays_device(nullptr, nullptr, n, k, nullptr, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_color_at_rays(nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_color_at_rays_device(nullptr, nullptr, n, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_ray_color_rays(nullptr, nullptr, nullptr, n, 1, 5, nullptr, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_ray_color_rays_device(nullptr, nullptr, nullptr, n, 1, 5, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_camera_rays(nullptr, n, nullptr, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_camera_rays_device(nullptr, n, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_scatter_rays(nullptr, nullptr, nullptr, nullptr, n, 1, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_scatter_rays_device(nullptr, nullptr, nullptr, nullptr, n, 1, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_hit_rays_seeded(nullptr, nullptr, nullptr, n, 1, 1e-10, inf, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_hit_rays_seeded_device(nullptr, nullptr, nullptr, n, 1, 1e-10, inf, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_texture_values(nullptr, nullptr, nullptr, nullptr, n, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtiow_texture_values_device(nullptr, nullptr, nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_prepare_rays(nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_prepare_rays_device(nullptr, nullptr, n, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_shade_hits(nullptr, nullptr, n, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_shade_hits_device(nullptr, nullptr, n, nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_shadow_attenuation(nullptr, nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_shadow_attenuation_device(nullptr, nullptr, nullptr, n, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_lighting(nullptr, nullptr, nullptr, nullptr, nullptr, n, nullptr), RL_E_NO_DEVICE);
  EXPECT(rl_rtc_lighting_device(nullptr, nullptr, nullptr, nullptr, nullptr, n, nullptr, nullptr), RL_E_NO_DEVICE);
  // ---- the render entry points: valid buffers; an image whose row_first equals its height (the forms without row arguments start at
  // row 0: an image without rows); every pointer NULL.  A prefilled opt_stats stays as it was.
  rl_rtc_camera rcam{};
  rcam.hsize = 8, rcam.vsize = 8;
  std::vector<double> frame(8 * 8 * 3, -1.0);
  std::vector<uint8_t> bytes(8 * 8 * 3, 0xAB);
  rl_stats filled, before;
  std::memset(&filled, 0xA5, sizeof filled);
  before = filled;
  uint64_t claimed = 7, total = 7;
  uint32_t phase = 7;
  for (int way = 0; way < 3; way++) {
    rl_rtiow_camera c1 = cam;
    rl_rtc_camera c2 = rcam;
    if (way == 1) c1.image_height = 0, c2.vsize = 0;  // for the forms that always start at row 0
    const rl_rtiow_camera *pc1 = way == 2 ? nullptr : &c1, *pr1 = way == 2 ? nullptr : &cam;  // pr*: the forms with a row_first of their own
    const rl_rtc_camera *pc2 = way == 2 ? nullptr : &c2, *pr2 = way == 2 ? nullptr : &rcam;
    double *f = way == 2 ? nullptr : frame.data();
    uint8_t *b = way == 2 ? nullptr : bytes.data();
    rl_stats *s = way == 2 ? nullptr : &filled;
    const uint32_t row_first = way == 1 ? 8 : 0, row_step = way == 2 ? 0 : 1;
    EXPECT(rl_rtiow_render(nullptr, pc1, 0, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_rows(nullptr, pr1, 0, row_first, row_step, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_device(nullptr, pr1, 0, row_first, row_step, f, nullptr, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_independent_rows(nullptr, pr1, 0, row_first, row_step, 1, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_independent_device(nullptr, pr1, 0, row_first, row_step, 1, f, nullptr, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_multi(nullptr, pc1, 0, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_multi_device(nullptr, pc1, 0, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtiow_render_rgb8(nullptr, pc1, 0, b, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_render(nullptr, pc2, 1, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_render_rows(nullptr, pr2, 1, row_first, row_step, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_render_device(nullptr, pr2, 1, row_first, row_step, f, nullptr, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_render_multi(nullptr, pc2, 1, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_render_multi_device(nullptr, pc2, 1, f, s), RL_E_NO_DEVICE);
    EXPECT(rl_rtc_render_rgb8(nullptr, pc2, 1, b, s), RL_E_NO_DEVICE);
    EXPECT(rl_render_status(nullptr, s), RL_E_NO_DEVICE);
    if (way == 2)
      EXPECT(rl_rtiow_render_progress(nullptr, nullptr, nullptr, nullptr), RL_E_NO_DEVICE);
    else
      EXPECT(rl_rtiow_render_progress(nullptr, &claimed, &total, &phase), RL_E_NO_DEVICE);
  }
  calls++;
  if (std::memcmp(&filled, &before, sizeof filled) != 0 || claimed != 7 || total != 7 || phase != 7) {
    std::printf("FAIL a render entry point wrote opt_stats or a progress output without a device\n");
    failures++;
  }
  for (double v : frame) failures += v != -1.0;
  for (uint8_t v : bytes) failures += v != 0xAB;
  if (failures)
    std::printf("%d of %d checks failed\n", failures, calls);
  else
    std::printf("batched queries and renders, no-device paths: ok (%d checks)\n", calls);
  return failures ? 1 : 0;
}
