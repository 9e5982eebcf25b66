// The host side of the direct-lighting renders (include/rl_render.h "Direct-lighting renders", rl_rtiow_render_direct*; DESIGN.md §3.21;
// kernel: rl_rtiow_direct.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernel is
// instantiated behind every other one), and it uses what rl_ao_api.h uses: rl_query_api.h's query_run, hit_query_params,
// query_tree_params and rl_debug_last_query ids, rl_features_api.h's launch geometry, the render checks and the staging of rl_host_api.h.
// Four entry points over one launch function; the routing and the LDS plan are rtiow_ao_impl's.
#pragma once

namespace {
// rl_debug_last_query ids of the direct-lighting renders (1 .. 8: the ray queries', the feature renders', the occlusion queries', the AO renders')
constexpr int LAST_QUERY_DIRECT_REFERENCE = 9, LAST_QUERY_DIRECT_FAST = 10;

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

struct DirectArgs {
  uint32_t n_lights, light_samples;
  double seg_tmax;
  DirectLight lights[RL_DIRECT_MAX_LIGHTS];
};
}  // namespace

// One launch for the shard rows (d_xs == null: n = nrows * W slots) and for a pixel list; counting / sync_st as rtiow_ao_impl.
static int rtiow_direct_impl(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, const void *d_xs,
                             const void *d_ys, uint64_t n, const DirectArgs &A, void *d_direct, void *d_unshadowed, void *d_hits, hipStream_t stream,
                             bool counting, rl_stats *sync_st) {
  const FastGeneral &QF = scene->hrt->query_tree();
  RtiowParams P = hit_query_params(scene);
  P.cam = *cam;
  chacha_key_from_seed(cam->seed, P.key);
  P.first_sample = first_sample, P.row_first = row_first, P.row_step = row_step;
  DirectQuery Q{};
  Q.n = n, Q.xs = (const uint32_t *)d_xs, Q.ys = (const uint32_t *)d_ys;
  Q.n_lights = A.n_lights, Q.light_samples = A.light_samples, Q.seg_tmax = A.seg_tmax;
  Q.direct = (double *)d_direct, Q.unshadowed = (double *)d_unshadowed, Q.hit_count = (uint32_t *)d_hits;
  for (uint32_t l = 0; l < A.n_lights; l++) Q.lights[l] = A.lights[l];
  const bool fast = !counting && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    size_t lds = (size_t)FEATURES_NT * 16 * sizeof(unsigned long long);  // the ChaCha rings
    void (*kern)(RtiowParams, DirectQuery) =
        counting ? rtiow_direct_kernel<FEATURES_NT, true, false, FEATURES_SD> : rtiow_direct_kernel<FEATURES_NT, false, false, FEATURES_SD>;
    if (fast) {
      kern = rtiow_direct_kernel<FEATURES_NT, false, true, FEATURES_SD>;
      P.fg_nodes = scene->d_fg_nodes, P.fg_items = scene->d_fg_items, P.fg_spheres = scene->d_fg_spheres, P.fg_material = scene->d_fg_material;
      P.fg_seg_roots = scene->d_fg_seg_roots;
      query_tree_params(QF, P);
      // LDS: rings, the per-lane stacks, and the tree's top (breadth first) in what two workgroups per CU leave of it
      const size_t base = lds + (size_t)FEATURES_NT * FEATURES_SD * sizeof(uint32_t);
      const size_t half = g_lds_max / 2;
      const size_t room = half > base ? (half - base) / sizeof(FastNodeQ) : 0;
      P.fg_top = g_sw.fastg_top ? (uint32_t)std::min<size_t>(QF.top_nodes, room) : 0u;
      lds = base + (size_t)P.fg_top * sizeof(FastNodeQ);
    }
    if (ensure_lds_attr((const void *)kern, lds) != 0) return set_err(RL_E_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    const uint64_t want = (n + FEATURES_NT - 1) / FEATURES_NT;
    const uint64_t cap = (uint64_t)std::max(1, g_cus) * (uint64_t)std::max<size_t>(1, std::min<size_t>(g_lds_max / lds, FEATURES_MAX_BLOCKS_PER_CU));
    hipLaunchKernelGGL(kern, dim3((uint32_t)std::min(want, cap)), dim3(FEATURES_NT), lds, stream, P, Q);
    g_last_query_kernel = fast ? LAST_QUERY_DIRECT_FAST : LAST_QUERY_DIRECT_REFERENCE;
    if (!fast) g_last_query_retraced = 0;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch, fast);
}

extern "C" {

int rl_rtiow_render_direct_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_direct, void *d_unshadowed,
                                  void *d_hit_count, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!direct_ok(cam, n_lights, lights, light_samples, seg_tmax, d_direct, d_unshadowed, d_hit_count, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  const uint64_t n = frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double));
  if (n >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");
  return rtiow_direct_impl(scene, cam, first_sample, row_first, row_step, nullptr, nullptr, n, A, d_direct, d_unshadowed, d_hit_count, (hipStream_t)hip_stream,
                           st != nullptr, st);
}

int rl_rtiow_render_direct_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *direct, double *unshadowed,
                                uint32_t *hit_count, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!direct_ok(cam, n_lights, lights, light_samples, seg_tmax, direct, unshadowed, hit_count, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  HostStaging q(scene);
  const size_t bytes = frame_of(cam).rows_bytes(row_first, row_step), pixels = bytes / (3 * sizeof(double));
  void *d_direct = q.out(direct, bytes), *d_unsh = q.out(unshadowed, bytes), *d_hits = q.out(hit_count, pixels * sizeof(uint32_t));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // (always a counting call, as rl_rtiow_render_ao_rows)
  return q.finish(
      rl_rtiow_render_direct_device(scene, cam, first_sample, row_first, row_step, n_lights, lights, light_samples, seg_tmax, d_direct, d_unsh, d_hits, q.stream, &local),
      st, local);
}

int rl_rtiow_render_pixels_direct_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                         uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_direct, void *d_unshadowed,
                                         void *d_hit_count, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!direct_ok(cam, n_lights, lights, light_samples, seg_tmax, d_direct, d_unshadowed, d_hit_count, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (d_xs && d_ys), 0, "empty image", st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return rtiow_direct_impl(scene, cam, first_sample, 0, 1, d_xs, d_ys, n, A, d_direct, d_unshadowed, d_hit_count, (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_render_pixels_direct(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                  uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *direct, double *unshadowed,
                                  uint32_t *hit_count, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!direct_ok(cam, n_lights, lights, light_samples, seg_tmax, direct, unshadowed, hit_count, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (xs && ys), 0, "empty image", st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  void *d_direct = q.out(direct, (size_t)n * 3 * sizeof(double)), *d_unsh = q.out(unshadowed, (size_t)n * 3 * sizeof(double));
  void *d_hits = q.out(hit_count, (size_t)n * sizeof(uint32_t));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast walks where they apply); rays, words and flagged are still collected
  return q.finish(rtiow_direct_impl(scene, cam, first_sample, 0, 1, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, A, d_direct, d_unsh, d_hits, q.stream,
                                    st != nullptr, &local),
                  st, local);
}

}  // extern "C"
