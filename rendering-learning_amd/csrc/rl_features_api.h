// The host side of the feature renders (include/rl_render.h "Feature renders", rl_rtiow_render_features*; kernel:
// rl_rtiow_features.h).  Not a translation unit of its own: rl_render.hip includes it once, behind rl_query_api.h, whose query_run,
// hit_query_params, query_tree_params and rl_debug_last_query ids it uses beside the render checks and the staging of rl_host_api.h.
// Four entry points over one launch function; the routing between the two instantiations of the trace is rtiow_hit_rays_impl's.
#pragma once

namespace {
constexpr int FEATURES_NT = 256;
constexpr int FEATURES_SD = 40;
constexpr int FEATURES_MAX_BLOCKS_PER_CU = 2048 / FEATURES_NT;
// rl_debug_last_query ids of the feature renders (1 / 2 are the ray queries')
constexpr int LAST_QUERY_FEATURES_REFERENCE = 3, LAST_QUERY_FEATURES_FAST = 4;

// NULL, or no output asked for: refused before anything else is looked at
bool features_ok(const rl_rtiow_features *f) { return f && (f->albedo_sum || f->normal_sum || f->depth_sum || f->hit_count); }

// The host forms' device copies of the four optional outputs, `pixels` elements each
rl_rtiow_features stage_features(HostStaging &q, const rl_rtiow_features *out, size_t pixels) {
  rl_rtiow_features d;
  d.albedo_sum = (double *)q.out(out->albedo_sum, pixels * 3 * sizeof(double));
  d.normal_sum = (double *)q.out(out->normal_sum, pixels * 3 * sizeof(double));
  d.depth_sum = (double *)q.out(out->depth_sum, pixels * sizeof(double));
  d.hit_count = (uint32_t *)q.out(out->hit_count, pixels * sizeof(uint32_t));
  return d;
}
}  // namespace

// One launch for the shard rows (d_xs == null: n = nrows * W slots) and for a pixel list.  counting: the caller wants the reference's
// counters (reference-order instantiation); sync_st: filled synchronously (the host forms; rays, words and flagged only when !counting);
// null: asynchronous, status ring.
static int rtiow_features_impl(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, const void *d_xs,
                               const void *d_ys, uint64_t n, const rl_rtiow_features *d_out, hipStream_t stream, bool counting, rl_stats *sync_st) {
  const FastGeneral &QF = scene->hrt->query_tree();
  RtiowParams P = hit_query_params(scene);
  P.materials = scene->d_materials, P.textures = scene->d_textures, P.images = scene->d_images, P.image_pool = scene->d_image_pool;
  P.perlins = scene->d_perlins;
  P.cam = *cam;
  chacha_key_from_seed(cam->seed, P.key);
  P.first_sample = first_sample, P.row_first = row_first, P.row_step = row_step;
  FeaturesQuery Q{};
  Q.n = n, Q.xs = (const uint32_t *)d_xs, Q.ys = (const uint32_t *)d_ys;
  Q.albedo_sum = d_out->albedo_sum, Q.normal_sum = d_out->normal_sum, Q.depth_sum = d_out->depth_sum, Q.hit_count = d_out->hit_count;
  const bool fast = !counting && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    size_t lds = (size_t)FEATURES_NT * 16 * sizeof(unsigned long long);  // the ChaCha rings
    void (*kern)(RtiowParams, FeaturesQuery) =
        counting ? rtiow_features_kernel<FEATURES_NT, true, false, FEATURES_SD> : rtiow_features_kernel<FEATURES_NT, false, false, FEATURES_SD>;
    if (fast) {
      kern = rtiow_features_kernel<FEATURES_NT, false, true, FEATURES_SD>;
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
    g_last_query_kernel = fast ? LAST_QUERY_FEATURES_FAST : LAST_QUERY_FEATURES_REFERENCE;
    if (!fast) g_last_query_retraced = 0;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch, fast);
}

extern "C" {

// the most lanes one feature launch has on the current device: a frame or list beyond it puts several pixels through one lane
unsigned long long rl_debug_features_lanes(void) { return (unsigned long long)std::max(1, g_cus) * FEATURES_MAX_BLOCKS_PER_CU * FEATURES_NT; }

int rl_rtiow_render_features_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                    const rl_rtiow_features *d_out, void *hip_stream, rl_stats *st) {
  if (!features_ok(d_out)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  const uint64_t n = frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double));
  if (n >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");
  return rtiow_features_impl(scene, cam, first_sample, row_first, row_step, nullptr, nullptr, n, d_out, (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_render_features_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                  const rl_rtiow_features *out, rl_stats *st) {
  if (!features_ok(out)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  HostStaging q(scene);
  const rl_rtiow_features d_out = stage_features(q, out, frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double)));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // (always a counting call, as rl_rtiow_render_rows)
  return q.finish(rl_rtiow_render_features_device(scene, cam, first_sample, row_first, row_step, &d_out, q.stream, &local), st, local);
}

int rl_rtiow_render_pixels_features_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                           const rl_rtiow_features *d_out, void *hip_stream, rl_stats *st) {
  if (!features_ok(d_out)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (d_xs && d_ys), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return rtiow_features_impl(scene, cam, first_sample, 0, 1, d_xs, d_ys, n, d_out, (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_render_pixels_features(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                    const rl_rtiow_features *out, rl_stats *st) {
  if (!features_ok(out)) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (xs && ys), 0, "empty image", st, done);
  if (done) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  const rl_rtiow_features d_out = stage_features(q, out, (size_t)n);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast walk where it applies); rays, words and flagged are still collected
  return q.finish(rtiow_features_impl(scene, cam, first_sample, 0, 1, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, &d_out, q.stream, st != nullptr, &local), st, local);
}

}  // extern "C"
