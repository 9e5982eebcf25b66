// What the host side of every pixel render is made of (include/rl_render.h "Feature renders" .. "NEE path renders with multiple
// importance sampling"): the renders that put one pixel of a shard's rows or of a pixel list through one lane and write
// per-pixel outputs — features, ambient occlusion, direct lighting, NEE paths with and without MIS.  Not a translation unit of its own:
// rl_render.hip includes it once, behind rl_query_api.h, whose query_run, hit_query_params, query_tree_params and rl_debug_last_query ids
// it uses beside the render checks and the staging of rl_host_api.h.  No kernel is named here.
//   pixel_render_params  — RtiowParams of a pixel render: the scene's tables, camera, key, first_sample, the row fields
//   pixel_render_launch  — the routing between a family's three instantiations, the LDS plan, the grid, the launch, rl_debug_last_query
//   pixel_rows_device / pixel_rows_host / pixel_list_device / pixel_list_host — the four entry forms, each check sequence once
// A family (rl_features_api.h, rl_ao_api.h, rl_direct_api.h, rl_nee_api.h) is an argument check, a rule, a list of outputs and a callable
// that fills its query struct from a PixelTarget and launches.
#pragma once

namespace {
constexpr int FEATURES_NT = 256;
constexpr int FEATURES_SD = 40;
constexpr int FEATURES_MAX_BLOCKS_PER_CU = 2048 / FEATURES_NT;
constexpr int PIXEL_RENDER_MAX_OUTS = 4;

// One output of a family: the caller's pointer (host or device, null: not asked for) and what a pixel takes of it
struct PixelOut {
  void *p;
  size_t bytes_per_pixel;
};

// What an entry form hands the family's callable: the slots (d_xs == null: the shard's rows, n = nrows * W), the device outputs in the
// order of the family's PixelOut list, and how the call runs.  counting: the caller wants the reference's counters (reference-order
// instantiation); sync_st: filled synchronously (the host forms; rays, words and flagged only when !counting); null: asynchronous,
// status ring.
struct PixelTarget {
  uint32_t row_first, row_step;
  const void *d_xs, *d_ys;
  uint64_t n;
  void *out[PIXEL_RENDER_MAX_OUTS];
  hipStream_t stream;
  bool counting;
  rl_stats *sync_st;
};

// shading: the kernel reads materials and textures (features, NEE); the others leave the tables null
RtiowParams pixel_render_params(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const PixelTarget &T, bool shading) {
  RtiowParams P = hit_query_params(scene);
  if (shading) {
    P.materials = scene->d_materials, P.textures = scene->d_textures, P.images = scene->d_images, P.image_pool = scene->d_image_pool;
    P.perlins = scene->d_perlins;
  }
  P.cam = *cam;
  chacha_key_from_seed(cam->seed, P.key);
  P.first_sample = first_sample, P.row_first = T.row_first, P.row_step = T.row_step;
  return P;
}

// One launch of a family's kernel over T.n slots: `k_counting` for a counting call, `k_fast` where the scene has a query tree without
// media and the fast traversal is on, else `k_reference` (counter-free, reference order).  Q: the family's query struct, or one derived
// from it (NeeMisQuery).
template <class Query>
int pixel_render_launch(const rl_scene *scene, RtiowParams P, const Query &Q, void (*k_counting)(RtiowParams, Query), void (*k_reference)(RtiowParams, Query),
                        void (*k_fast)(RtiowParams, Query), int id_reference, int id_fast, const PixelTarget &T) {
  const FastGeneral &QF = scene->hrt->query_tree();
  const bool fast = !T.counting && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    size_t lds = (size_t)FEATURES_NT * 16 * sizeof(unsigned long long);  // the ChaCha rings
    void (*kern)(RtiowParams, Query) = T.counting ? k_counting : k_reference;
    if (fast) {
      kern = k_fast;
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
    const uint64_t want = (T.n + FEATURES_NT - 1) / FEATURES_NT;
    const uint64_t cap = (uint64_t)std::max(1, g_cus) * (uint64_t)std::max<size_t>(1, std::min<size_t>(g_lds_max / lds, FEATURES_MAX_BLOCKS_PER_CU));
    hipLaunchKernelGGL(kern, dim3((uint32_t)std::min(want, cap)), dim3(FEATURES_NT), lds, T.stream, P, Q);
    g_last_query_kernel = fast ? id_fast : id_reference;
    if (!fast) g_last_query_retraced = 0;
    return RL_OK;
  };
  return query_run(scene, T.stream, T.sync_st, launch, fast);
}

// The family's side of an entry form.  ok: the family's argument check, made before anything else is looked at; rules: what the family
// adds to render_check (-> RL_*, with its own text; null: nothing); outs: the outputs in the order they are staged and handed on.
struct PixelFamily {
  bool ok;
  int (*rules)(const rl_scene *);
  PixelOut outs[PIXEL_RENDER_MAX_OUTS];
};

// the host forms' family: device copies in the outputs' places, `pixels` elements each
PixelFamily stage_pixel_outs(HostStaging &q, PixelFamily f, size_t pixels) {
  for (PixelOut &o : f.outs)
    if (o.bytes_per_pixel) o.p = q.out(o.p, pixels * o.bytes_per_pixel);
  return f;
}

// the family's callable on T with the family's (device) output pointers put in
template <class Run>
int pixel_render_run(const PixelFamily &f, PixelTarget T, Run run) {
  for (int k = 0; k < PIXEL_RENDER_MAX_OUTS; k++) T.out[k] = f.outs[k].p;
  return run(T);
}

// rl_rtiow_render_<family>_device: rows row_first, row_first + row_step, ... of the frame into device buffers
template <class Run>
int pixel_rows_device(const PixelFamily &f, const rl_scene *scene, const rl_rtiow_camera *cam, uint32_t row_first, uint32_t row_step, void *hip_stream,
                      rl_stats *st, Run run) {
  if (!f.ok) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, "empty image", st, done);
  if (done) return rc;
  if (f.rules && (rc = f.rules(scene)) != RL_OK) return rc;
  const uint64_t n = frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double));
  if (n >= PIXEL_LIST_MAX_N) return set_err(RL_E_INVALID, "image too large");
  return pixel_render_run(f, PixelTarget{row_first, row_step, nullptr, nullptr, n, {}, (hipStream_t)hip_stream, st != nullptr, st}, run);
}

// rl_rtiow_render_<family>_rows: the same into host arrays, through the device form (always a counting call, as rl_rtiow_render_rows)
template <class Run>
int pixel_rows_host(const PixelFamily &f, const rl_scene *scene, const rl_rtiow_camera *cam, uint32_t row_first, uint32_t row_step, rl_stats *st, Run run) {
  if (!f.ok) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), row_step != 0, row_first, nullptr, st, done);
  if (done) return rc;
  if (f.rules && (rc = f.rules(scene)) != RL_OK) return rc;
  HostStaging q(scene);
  const PixelFamily d = stage_pixel_outs(q, f, frame_of(cam).rows_bytes(row_first, row_step) / (3 * sizeof(double)));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(pixel_rows_device(d, scene, cam, row_first, row_step, q.stream, &local, run), st, local);
}

// rl_rtiow_render_pixels_<family>_device: the pixels (d_xs[i], d_ys[i]) into device buffers
template <class Run>
int pixel_list_device(const PixelFamily &f, const rl_scene *scene, const rl_rtiow_camera *cam, const void *d_xs, const void *d_ys, uint64_t n, void *hip_stream,
                      rl_stats *st, Run run) {
  if (!f.ok) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (d_xs && d_ys), 0, "empty image", st, done);
  if (done) return rc;
  if (f.rules && (rc = f.rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  return pixel_render_run(f, PixelTarget{0, 1, d_xs, d_ys, n, {}, (hipStream_t)hip_stream, st != nullptr, st}, run);
}

// rl_rtiow_render_pixels_<family>: host lists into host arrays, straight to the launch
template <class Run>
int pixel_list_host(const PixelFamily &f, const rl_scene *scene, const rl_rtiow_camera *cam, const uint32_t *xs, const uint32_t *ys, uint64_t n, rl_stats *st,
                    Run run) {
  if (!f.ok) return set_err(RL_E_INVALID, "bad argument");
  bool done;
  int rc = render_check(scene, 1, frame_of(cam), n == 0 || (xs && ys), 0, "empty image", st, done);
  if (done) return rc;
  if (f.rules && (rc = f.rules(scene)) != RL_OK) return rc;
  rc = list_length_check(n, st, done);
  if (done) return rc;
  if ((rc = pixel_list_check(frame_of(cam), xs, ys, n)) != RL_OK) return rc;
  HostStaging q(scene);
  const unsigned char *d_xy = (const unsigned char *)q.in({{xs, (size_t)n * sizeof(uint32_t)}, {ys, (size_t)n * sizeof(uint32_t)}});
  const PixelFamily d = stage_pixel_outs(q, f, (size_t)n);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast walks where they apply); rays, words and flagged are still collected
  return q.finish(pixel_render_run(d, PixelTarget{0, 1, d_xy, d_xy + (size_t)n * sizeof(uint32_t), n, {}, q.stream, st != nullptr, &local}, run), st, local);
}
}  // namespace
