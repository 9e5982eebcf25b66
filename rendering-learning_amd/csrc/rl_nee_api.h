// The host side of the NEE path renders (include/rl_render.h "NEE path renders", rl_rtiow_render_nee*; kernel:
// rl_rtiow_nee.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernel is instantiated
// behind every other one), and it uses what rl_direct_api.h uses and that file's direct_ok, direct_rules and DirectArgs.
// Four entry points over one launch function; the routing and the LDS plan are rtiow_ao_impl's.
// The renders with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance sampling",
// rl_rtiow_render_nee_mis*) are the same four with a heuristic: both families run the four static functions below, which
// take the flavour as `mis`, through nee_ok, direct_rules and rtiow_nee_impl.
#pragma once

namespace {
// rl_debug_last_query ids of the NEE path renders (1 .. 10: the ray queries', the feature, occlusion, AO and direct-lighting renders')
constexpr int LAST_QUERY_NEE_REFERENCE = 11, LAST_QUERY_NEE_FAST = 12, LAST_QUERY_NEE_MIS_REFERENCE = 13, LAST_QUERY_NEE_MIS_FAST = 14;
// `mis` of everything below: -1 the plain NEE renders, else the heuristic of the renders with multiple importance sampling
constexpr int NEE_PLAIN = -1;

// The six instantiations: {plain, MIS} x {counting, counter-free reference order, counter-free fast walks}
template <bool MIS>
auto nee_kernel(bool counting, bool fast) -> void (*)(RtiowParams, NeeQueryOf<MIS>) {
  if (fast) return rtiow_nee_kernel<FEATURES_NT, false, true, FEATURES_SD, MIS>;
  return counting ? rtiow_nee_kernel<FEATURES_NT, true, false, FEATURES_SD, MIS> : rtiow_nee_kernel<FEATURES_NT, false, false, FEATURES_SD, MIS>;
}

// What is particular to these calls and decided before a device is looked at: direct_ok's rules with the two outputs of these calls, and
// a path of at least one vertex.  On success `out` holds the lights as the kernel reads them.
bool nee_ok(int mis, const rl_rtiow_camera *cam, uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, const void *sums, const void *sq,
            DirectLight *out) {
  if (cam && cam->max_depth == 0) return false;
  if (mis != NEE_PLAIN && mis != (int)RL_MIS_BALANCE && mis != (int)RL_MIS_POWER) return false;
  return direct_ok(cam, n_lights, lights, light_samples, seg_tmax, sums, sq, nullptr, out);
}
}  // namespace

// One launch for the shard rows (d_xs == null: n = nrows * W slots) and for a pixel list; counting / sync_st as rtiow_ao_impl.
static int rtiow_nee_impl(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, const void *d_xs,
                          const void *d_ys, uint64_t n, const DirectArgs &A, int mis, void *d_sums, void *d_sq, hipStream_t stream, bool counting, rl_stats *sync_st) {
  const FastGeneral &QF = scene->hrt->query_tree();
  RtiowParams P = hit_query_params(scene);
  P.materials = scene->d_materials, P.textures = scene->d_textures, P.images = scene->d_images, P.image_pool = scene->d_image_pool;
  P.perlins = scene->d_perlins;
  P.cam = *cam;
  chacha_key_from_seed(cam->seed, P.key);
  P.first_sample = first_sample, P.row_first = row_first, P.row_step = row_step;
  NeeQuery Q{};
  Q.n = n, Q.xs = (const uint32_t *)d_xs, Q.ys = (const uint32_t *)d_ys;
  Q.n_lights = A.n_lights, Q.light_samples = A.light_samples, Q.seg_tmax = A.seg_tmax;
  Q.kf = 1.0 / (M_PI * (double)A.light_samples);
  Q.sums = (double *)d_sums, Q.sq = (double *)d_sq;
  for (uint32_t l = 0; l < A.n_lights; l++) Q.lights[l] = A.lights[l];
  const bool fast = !counting && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    size_t lds = (size_t)FEATURES_NT * 16 * sizeof(unsigned long long);  // the ChaCha rings
    const void *kern = mis >= 0 ? (const void *)nee_kernel<true>(counting, fast) : (const void *)nee_kernel<false>(counting, fast);
    if (fast) {
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
    if (ensure_lds_attr(kern, lds) != 0) return set_err(RL_E_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
    const uint64_t want = (n + FEATURES_NT - 1) / FEATURES_NT;
    const uint64_t cap = (uint64_t)std::max(1, g_cus) * (uint64_t)std::max<size_t>(1, std::min<size_t>(g_lds_max / lds, FEATURES_MAX_BLOCKS_PER_CU));
    const dim3 grid((uint32_t)std::min(want, cap)), block(FEATURES_NT);
    if (mis >= 0) {
      NeeMisQuery M{};
      static_cast<NeeQuery &>(M) = Q;
      M.heuristic = (uint32_t)mis;
      hipLaunchKernelGGL(nee_kernel<true>(counting, fast), grid, block, lds, stream, P, M);
    } else {
      hipLaunchKernelGGL(nee_kernel<false>(counting, fast), grid, block, lds, stream, P, Q);
    }
    g_last_query_kernel = mis >= 0 ? (fast ? LAST_QUERY_NEE_MIS_FAST : LAST_QUERY_NEE_MIS_REFERENCE) : (fast ? LAST_QUERY_NEE_FAST : LAST_QUERY_NEE_REFERENCE);
    if (!fast) g_last_query_retraced = 0;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch, fast);
}

static int nee_device(int mis, const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                      const double *lights, uint32_t light_samples, double seg_tmax, void *d_sums, void *d_sq, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!nee_ok(mis, cam, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  const uint64_t n = frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double));
  if (n >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");
  return rtiow_nee_impl(scene, cam, first_sample, row_first, row_step, nullptr, nullptr, n, A, mis, d_sums, d_sq, (hipStream_t)hip_stream, st != nullptr, st);
}

static int nee_rows(int mis, const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                    const double *lights, uint32_t light_samples, double seg_tmax, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!nee_ok(mis, cam, n_lights, lights, light_samples, seg_tmax, sums, sq, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  HostStaging q(scene);
  const size_t bytes = frame_of(cam).rows_bytes(row_first, row_step);
  void *d_sums = q.out(sums, bytes), *d_sq = q.out(sq, bytes);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // (always a counting call, as rl_rtiow_render_direct_rows)
  return q.finish(nee_device(mis, scene, cam, first_sample, row_first, row_step, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, q.stream, &local),
                  st, local);
}

static int nee_pixels_device(int mis, const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                             uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_sums, void *d_sq, void *hip_stream,
                             rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!nee_ok(mis, cam, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (d_xs && d_ys), 0, "empty image", st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return rtiow_nee_impl(scene, cam, first_sample, 0, 1, d_xs, d_ys, n, A, mis, d_sums, d_sq, (hipStream_t)hip_stream, st != nullptr, st);
}

static int nee_pixels(int mis, const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                      uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  if (!nee_ok(mis, cam, n_lights, lights, light_samples, seg_tmax, sums, sq, A.lights)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (xs && ys), 0, "empty image", st, done);
  if (done) return rc;
  if ((rc = direct_rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  void *d_sums = q.out(sums, (size_t)n * 3 * sizeof(double)), *d_sq = q.out(sq, (size_t)n * 3 * sizeof(double));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast walks where they apply); rays, words and flagged are still collected
  return q.finish(
      rtiow_nee_impl(scene, cam, first_sample, 0, 1, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, A, mis, d_sums, d_sq, q.stream, st != nullptr, &local), st, local);
}

// a heuristic beyond the two is kept a value nee_ok refuses (never NEE_PLAIN)
static int mis_of(uint32_t heuristic) { return heuristic <= RL_MIS_POWER ? (int)heuristic : (int)RL_MIS_POWER + 1; }

extern "C" {

int rl_rtiow_render_nee_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                               const double *lights, uint32_t light_samples, double seg_tmax, void *d_sums, void *d_sq, void *hip_stream, rl_stats *st) {
  return nee_device(NEE_PLAIN, scene, cam, first_sample, row_first, row_step, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, hip_stream, st);
}
int rl_rtiow_render_nee_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                             const double *lights, uint32_t light_samples, double seg_tmax, double *sums, double *sq, rl_stats *st) {
  return nee_rows(NEE_PLAIN, scene, cam, first_sample, row_first, row_step, n_lights, lights, light_samples, seg_tmax, sums, sq, st);
}
int rl_rtiow_render_pixels_nee_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                      uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_sums, void *d_sq, void *hip_stream,
                                      rl_stats *st) {
  return nee_pixels_device(NEE_PLAIN, scene, cam, first_sample, d_xs, d_ys, n, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, hip_stream, st);
}
int rl_rtiow_render_pixels_nee(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                               uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *sums, double *sq, rl_stats *st) {
  return nee_pixels(NEE_PLAIN, scene, cam, first_sample, xs, ys, n, n_lights, lights, light_samples, seg_tmax, sums, sq, st);
}

// with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance sampling"): the same four with a heuristic
int rl_rtiow_render_nee_mis_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                   uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, void *d_sums, void *d_sq,
                                   void *hip_stream, rl_stats *st) {
  return nee_device(mis_of(heuristic), scene, cam, first_sample, row_first, row_step, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, hip_stream, st);
}
int rl_rtiow_render_nee_mis_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                                 const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, double *sums, double *sq, rl_stats *st) {
  return nee_rows(mis_of(heuristic), scene, cam, first_sample, row_first, row_step, n_lights, lights, light_samples, seg_tmax, sums, sq, st);
}
int rl_rtiow_render_pixels_nee_mis_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                          uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, void *d_sums,
                                          void *d_sq, void *hip_stream, rl_stats *st) {
  return nee_pixels_device(mis_of(heuristic), scene, cam, first_sample, d_xs, d_ys, n, n_lights, lights, light_samples, seg_tmax, d_sums, d_sq, hip_stream, st);
}
int rl_rtiow_render_pixels_nee_mis(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                   uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, double *sums, double *sq,
                                   rl_stats *st) {
  return nee_pixels(mis_of(heuristic), scene, cam, first_sample, xs, ys, n, n_lights, lights, light_samples, seg_tmax, sums, sq, st);
}

}  // extern "C"
