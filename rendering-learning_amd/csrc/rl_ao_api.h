// The host side of the ambient-occlusion renders (include/rl_render.h "Ambient-occlusion renders", rl_rtiow_render_ao*; DESIGN.md §3.20;
// kernel: rl_rtiow_ao.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernel is
// instantiated behind every other one), and it uses rl_query_api.h's query_run, hit_query_params, query_tree_params and
// rl_debug_last_query ids, rl_features_api.h's launch geometry, and the render checks and the staging of rl_host_api.h.
// Four entry points over one launch function; the routing between the instantiations is rtiow_features_impl's.
#pragma once

namespace {
// rl_debug_last_query ids of the ambient-occlusion renders (1 .. 6: the ray queries', the feature renders', the occlusion queries')
constexpr int LAST_QUERY_AO_REFERENCE = 7, LAST_QUERY_AO_FAST = 8;

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
}  // namespace

// One launch for the shard rows (d_xs == null: n = nrows * W slots) and for a pixel list.  counting: the caller wants the reference's
// counters (reference-order instantiation); sync_st: filled synchronously (the host forms; rays, words and flagged only when !counting);
// null: asynchronous, status ring.
static int rtiow_ao_impl(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, const void *d_xs,
                         const void *d_ys, uint64_t n, uint32_t ao_rays, double radius, void *d_open, void *d_hits, hipStream_t stream, bool counting,
                         rl_stats *sync_st) {
  const FastGeneral &QF = scene->hrt->query_tree();
  RtiowParams P = hit_query_params(scene);
  P.cam = *cam;
  chacha_key_from_seed(cam->seed, P.key);
  P.first_sample = first_sample, P.row_first = row_first, P.row_step = row_step;
  AoQuery Q{};
  Q.n = n, Q.xs = (const uint32_t *)d_xs, Q.ys = (const uint32_t *)d_ys;
  Q.ao_rays = ao_rays, Q.radius = radius, Q.open_count = (uint32_t *)d_open, Q.hit_count = (uint32_t *)d_hits;
  const bool fast = !counting && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    size_t lds = (size_t)FEATURES_NT * 16 * sizeof(unsigned long long);  // the ChaCha rings
    void (*kern)(RtiowParams, AoQuery) =
        counting ? rtiow_ao_kernel<FEATURES_NT, true, false, FEATURES_SD> : rtiow_ao_kernel<FEATURES_NT, false, false, FEATURES_SD>;
    if (fast) {
      kern = rtiow_ao_kernel<FEATURES_NT, false, true, FEATURES_SD>;
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
    g_last_query_kernel = fast ? LAST_QUERY_AO_FAST : LAST_QUERY_AO_REFERENCE;
    if (!fast) g_last_query_retraced = 0;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch, fast);
}

extern "C" {

int rl_rtiow_render_ao_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t ao_rays,
                              double radius, void *d_open_count, void *d_hit_count, void *hip_stream, rl_stats *st) {
  if (!ao_ok(cam, ao_rays, radius, d_open_count, d_hit_count)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  if ((rc = ao_rules(scene)) != RL_OK) return rc;
  const uint64_t n = frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double));
  if (n >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");
  return rtiow_ao_impl(scene, cam, first_sample, row_first, row_step, nullptr, nullptr, n, ao_rays, radius, d_open_count, d_hit_count, (hipStream_t)hip_stream,
                       st != nullptr, st);
}

int rl_rtiow_render_ao_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t ao_rays,
                            double radius, uint32_t *open_count, uint32_t *hit_count, rl_stats *st) {
  if (!ao_ok(cam, ao_rays, radius, open_count, hit_count)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  if ((rc = ao_rules(scene)) != RL_OK) return rc;
  HostStaging q(scene);
  const size_t pixels = frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double));
  void *d_open = q.out(open_count, pixels * sizeof(uint32_t)), *d_hits = q.out(hit_count, pixels * sizeof(uint32_t));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // (always a counting call, as rl_rtiow_render_features_rows)
  return q.finish(rl_rtiow_render_ao_device(scene, cam, first_sample, row_first, row_step, ao_rays, radius, d_open, d_hits, q.stream, &local), st, local);
}

int rl_rtiow_render_pixels_ao_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                     uint32_t ao_rays, double radius, void *d_open_count, void *d_hit_count, void *hip_stream, rl_stats *st) {
  if (!ao_ok(cam, ao_rays, radius, d_open_count, d_hit_count)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (d_xs && d_ys), 0, "empty image", st, done);
  if (done) return rc;
  if ((rc = ao_rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return rtiow_ao_impl(scene, cam, first_sample, 0, 1, d_xs, d_ys, n, ao_rays, radius, d_open_count, d_hit_count, (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_render_pixels_ao(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                              uint32_t ao_rays, double radius, uint32_t *open_count, uint32_t *hit_count, rl_stats *st) {
  if (!ao_ok(cam, ao_rays, radius, open_count, hit_count)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (xs && ys), 0, "empty image", st, done);
  if (done) return rc;
  if ((rc = ao_rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  void *d_open = q.out(open_count, (size_t)n * sizeof(uint32_t)), *d_hits = q.out(hit_count, (size_t)n * sizeof(uint32_t));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast walks where they apply); rays, words and flagged are still collected
  return q.finish(
      rtiow_ao_impl(scene, cam, first_sample, 0, 1, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, ao_rays, radius, d_open, d_hits, q.stream, st != nullptr, &local),
      st, local);
}

}  // extern "C"
