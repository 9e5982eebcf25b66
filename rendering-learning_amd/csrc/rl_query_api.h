// The host side of the batched queries (include/rl_render.h rl_*_rays*, rl_rtiow_texture_values*, rl_rtc_lighting*; DESIGN.md §3.8 - §3.12;
// kernels: rl_ray_query.h, rl_material_query.h, rl_rtc_shade_query.h and the *_rays_kernel forms of the render kernels): 12 queries, each in a
// host-buffer and a _device form.  Not a translation unit of its own: rl_render.hip includes it once, at its end, and it uses that file's
// statics (g_sw, g_cus, g_lds_max, ensure_lds_attr, fill_rtiow_params, chacha_key_from_seed) and the launch half of rl_rtiow_launch.h.
//
// Every entry point is made of three moves, each of which exists once:
//   query_check   — library ready, scene family, the empty batch, null buffers, the batch bound; what is particular to a call follows it
//   query_run     — the scene's lock around query_begin, the call's launches and query_end
//   HostStaging   — the host forms' device copies of the caller's arrays, and the copy back (rl_host_api.h: the render forms' too)
// A new query is a check line, a run callable and a staging list.
#pragma once
#include <atomic>
#include <utility>

namespace {
constexpr int QNT = 256;
constexpr uint64_t QUERY_MAX_N = (uint64_t)1 << 40;  // elements per call
// the grid of a query kernel: what is resident at once (occupancy API, cached per kernel and device), at most one lane per ray
uint32_t query_grid(const rl_scene *scene, const void *kern, uint64_t n) {
  static std::mutex mu;
  static std::map<std::pair<const void *, int>, int> cache;
  int per_cu;
  {
    std::lock_guard<std::mutex> lk(mu);
    auto key = std::make_pair(kern, scene->device);
    auto it = cache.find(key);
    if (it == cache.end()) {
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kern, QNT, 0) != hipSuccess || nb < 1) nb = 2;
      it = cache.emplace(key, nb).first;
    }
    per_cu = it->second;
  }
  uint64_t want = (n + QNT - 1) / QNT, cap = (uint64_t)g_cus * (uint64_t)per_cu;
  return (uint32_t)(want < cap ? want : cap);
}
int query_begin(const rl_scene *scene, hipStream_t stream, bool want_stats) {
  int rco = rl::order_after_previous(scene, stream);
  if (rco != RL_OK) return rco;
  HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 512, stream));
  if (want_stats) HIP_TRY(hipEventRecord(scene->ev0, stream));
  return RL_OK;
}
int query_end(const rl_scene *scene, hipStream_t stream, rl_stats *st) {
  HIP_TRY(hipGetLastError());
  if (st) HIP_TRY(hipEventRecord(scene->ev1, stream));
  return st ? rl::collect_stats(scene, stream, st) : post_status(scene, stream);
}
RtcFullParams rtc_query_params(const rl_scene *scene) {
  const RtcProgram &rc_ = scene->rc();
  RtcFullParams F{};
  RtcParams &P = F.R;
  P.ops = scene->d_ops, P.tris = scene->d_tris, P.xforms = scene->d_xforms, P.materials = scene->d_rmaterials, P.lights = scene->d_lights;
  P.n_ops = (uint32_t)rc_.ops.size(), P.n_tris = (uint32_t)rc_.tris.size();
  const uint32_t n_guards = (uint32_t)scene->hrc->guards.size();  // reject-only box trees over the triangle ranges, as the renders use them
  P.guards = n_guards ? scene->d_guards : nullptr, P.n_guards = n_guards;
  P.n_xforms = (uint32_t)rc_.xforms.size(), P.n_lights = (uint32_t)rc_.lights.size();
  P.aa = 1, P.row_step = 1;
  std::memcpy(P.void_color, rc_.void_color, 24);
  P.stats = (unsigned long long *)(scene->d_scratch + 64);
  F.shapes = scene->d_shapes, F.csgs = scene->d_csgs, F.patterns = scene->d_patterns;
  F.n_tris = P.n_tris, F.max_reflection_depth = rc_.max_reflection_depth;
  return F;
}
// what the fast walk takes from the queries' tree (HostRtiow::query_tree) beside the device tables
void query_tree_params(const FastGeneral &QF, RtiowParams &P) {
  P.fg_root = QF.qroot, P.fg_rsafe2 = QF.r_safe * QF.r_safe * 0.9999f, P.fg_n_seg = (uint32_t)QF.stage_roots.size();
  P.fg_center[0] = QF.center[0], P.fg_center[1] = QF.center[1], P.fg_center[2] = QF.center[2];
  P.fg_radius = QF.radius, P.fg_pad_k = QF.pad_k;
}

// The argument rules every query shares.  kind: the scene family the call takes (1 RTIOW, 2 RTC), `subject` its rl_scene; 0: the call
// has no scene, and `subject` is the one argument it cannot do without (rl_rtiow_camera_rays*: the camera).  done: the call ends here
// with the returned code — an error, or the empty batch, which touches no buffer and zeroes `st` when given.
int query_check(const void *subject, int kind, uint64_t n, bool buffers_ok, rl_stats *st, bool &done) {
  done = true;
  if (!g_ready) return set_err(RL_E_NO_DEVICE, "rl_init has not succeeded");
  if (!subject) return set_err(RL_E_INVALID, kind == 0 ? "bad argument" : kind == 1 ? "not an RTIOW scene" : "not an RTC scene");
  if (kind != 0 && ((const rl_scene *)subject)->kind != kind) return set_err(RL_E_INVALID, kind == 1 ? "not an RTIOW scene" : "not an RTC scene");
  if (n == 0) {
    if (st) std::memset(st, 0, sizeof *st);
    return RL_OK;
  }
  if (!buffers_ok) return set_err(RL_E_INVALID, "null input / output buffer");
  if (n > QUERY_MAX_N) return set_err(RL_E_INVALID, "batch too large");
  done = false;
  return RL_OK;
}

// rl_debug_last_query: which kernel served the process's most recent query or pixel render.  Every family's pair, in one place.
enum LastQuery : int {
  LAST_QUERY_REFERENCE = 1,  // rl_rtiow_hit_rays*, rl_rtiow_hit_rays_seeded*, rl_rtiow_ray_color_rays*
  LAST_QUERY_FAST = 2,
  LAST_QUERY_FEATURES_REFERENCE = 3,  // the feature renders (rl_features_api.h)
  LAST_QUERY_FEATURES_FAST = 4,
  LAST_QUERY_OCCLUSION_REFERENCE = 5,  // the occlusion queries (rl_occlusion_api.h)
  LAST_QUERY_OCCLUSION_FAST = 6,
  LAST_QUERY_AO_REFERENCE = 7,  // the ambient-occlusion renders (rl_ao_api.h)
  LAST_QUERY_AO_FAST = 8,
  LAST_QUERY_DIRECT_REFERENCE = 9,  // the direct-lighting renders (rl_direct_api.h)
  LAST_QUERY_DIRECT_FAST = 10,
  LAST_QUERY_NEE_REFERENCE = 11,  // the NEE path renders (rl_nee_api.h)
  LAST_QUERY_NEE_FAST = 12,
  LAST_QUERY_NEE_MIS_REFERENCE = 13,  // ... with multiple importance sampling
  LAST_QUERY_NEE_MIS_FAST = 14,
  LAST_QUERY_NEE_SPHERES_REFERENCE = 15,  // ... and sphere lights (at least one)
  LAST_QUERY_NEE_SPHERES_FAST = 16,
};
// Atomic: queries of two scenes run under two locks.
std::atomic<int> g_last_query_kernel{0};                  // a LastQuery
std::atomic<unsigned long long> g_last_query_retraced{0};  // the rays the fast kernel re-traced (synchronous calls)

// One query of `scene` on `stream`: ordered behind the scene's previous work, then what `launch` enqueues (-> RL_*), then the status.
// sync_st: filled synchronously; null: asynchronous, status ring.  The scene's lock is held throughout (queries and renders of one scene:
// see rl_scene::mu) — also over the read of the fast walk's re-traced count (fast_walk: the calls rl_debug_last_query reports), for which
// the stream is idle and the scene still ours.
template <class Launch>
int query_run(const rl_scene *scene, hipStream_t stream, rl_stats *sync_st, Launch launch, bool fast_walk = false) {
  std::lock_guard<std::mutex> lk(scene->mu);
  int rc = query_begin(scene, stream, sync_st != nullptr);
  if (rc == RL_OK) rc = launch();
  if (rc != RL_OK) return rc;
  rc = query_end(scene, stream, sync_st);
  if (fast_walk && sync_st && outputs_written(rc)) {
    unsigned long long slow = 0;
    if (hipMemcpy(&slow, scene->d_scratch + 64 + 56, 8, hipMemcpyDeviceToHost) == hipSuccess) g_last_query_retraced = slow;
  }
  return rc;
}

}  // namespace

// what the reference-order fold (general_trace) reads of an RTIOW scene: rl_rtiow_hit_rays* and rl_rtiow_hit_rays_seeded*
static RtiowParams hit_query_params(const rl_scene *scene) {
  const RtiowProgram &rt = scene->rt();
  RtiowParams P = RtiowParams{};
  P.ops = scene->d_ops, P.spheres = scene->d_spheres, P.sphere_material = scene->d_sphere_material;
  P.planars = scene->d_planars, P.translates = scene->d_translates, P.transforms = scene->d_transforms, P.media = scene->d_media;
  P.n_ops = (uint32_t)rt.ops.size(), P.n_spheres = (uint32_t)rt.spheres.size();
  P.stats = (unsigned long long *)(scene->d_scratch + 64);
  return P;
}

extern "C" {

// ---- batched ray queries (include/rl_render.h): Hittable::hit, World::intersect and World::color_at for ray buffers
// counting: the caller wants the reference's counters (reference-order kernel).  Otherwise the fast kernel serves the call where the
// scene has a fast tree and tmin is the interval its filters are derived for (camera.rs:242-245).  sync_st: filled synchronously (the
// host forms; rays and flagged only when !counting); null: asynchronous, status ring.
// pass_from / pass_to (rl_rtiow_hit_rays_seeded* on a scene without media): n rl_rng_cursor copied device to device ahead of the kernel, as
// one of this query's enqueues (under the scene's lock, behind the scene's previous work, reported with the query).
static int rtiow_hit_rays_impl(const rl_scene *scene, const void *d_rays, uint64_t n, double tmin, double tmax, void *d_out, hipStream_t stream,
                               bool counting, rl_stats *sync_st, const void *pass_from = nullptr, void *pass_to = nullptr) {
  const FastGeneral &QF = scene->hrt->query_tree();
  RtiowParams P = hit_query_params(scene);
  RayQuery Q{};
  Q.rays = (const rl_ray *)d_rays, Q.n = n, Q.tmin = tmin, Q.tmax = tmax, Q.hits = (rl_rtiow_hit *)d_out;
  const bool fast = !counting && tmin == 1e-10 && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    if (pass_to) HIP_TRY(hipMemcpyAsync(pass_to, pass_from, (size_t)n * sizeof(rl_rng_cursor), hipMemcpyDeviceToDevice, stream));
    if (fast) {
      constexpr int SD = 40;
      P.fg_nodes = scene->d_fg_nodes, P.fg_items = scene->d_fg_items, P.fg_spheres = scene->d_fg_spheres, P.fg_material = scene->d_fg_material;
      P.fg_seg_roots = scene->d_fg_seg_roots;
      query_tree_params(QF, P);
      // LDS: the per-lane stacks, and the tree's top (breadth first) in what is left — no RNG rings here, so more of it than a render has
      const size_t base = (size_t)QNT * SD * sizeof(uint32_t);
      const size_t room = g_lds_max > base ? (g_lds_max - base) / sizeof(FastNodeQ) : 0;
      P.fg_top = g_sw.fastg_top ? (uint32_t)std::min<size_t>(QF.top_nodes, room) : 0u;
      const size_t lds = base + (size_t)P.fg_top * sizeof(FastNodeQ);
      const void *kern = (const void *)rtiow_hit_rays_fast_kernel<QNT, SD>;
      if (ensure_lds_attr(kern, lds) != 0) return set_err(RL_E_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      uint64_t want = (n + QNT - 1) / QNT, cap = (uint64_t)g_cus * (uint64_t)std::max<size_t>(1, std::min<size_t>(g_lds_max / lds, 2048 / QNT));
      hipLaunchKernelGGL((rtiow_hit_rays_fast_kernel<QNT, SD>), dim3((uint32_t)std::min(want, cap)), dim3(QNT), lds, stream, P, Q);
    } else if (counting)
      hipLaunchKernelGGL((rtiow_hit_rays_kernel<QNT, true>), dim3(query_grid(scene, (const void *)rtiow_hit_rays_kernel<QNT, true>, n)), dim3(QNT), 0, stream, P, Q);
    else
      hipLaunchKernelGGL((rtiow_hit_rays_kernel<QNT, false>), dim3(query_grid(scene, (const void *)rtiow_hit_rays_kernel<QNT, false>, n)), dim3(QNT), 0, stream, P, Q);
    g_last_query_kernel = fast ? LAST_QUERY_FAST : LAST_QUERY_REFERENCE;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch, true);
}

// what rl_rtiow_hit_rays* adds to query_check
static int rtiow_hit_rays_rules(const rl_scene *scene, double tmin, double tmax) {
  if (std::isnan(tmin) || std::isnan(tmax)) return set_err(RL_E_INVALID, "NaN interval bound");
  if (scene->rt().has_media)
    return set_err(RL_E_UNSUPPORTED, "ConstantMedium::hit draws from the pixel's RNG stream (constant_medium.rs:55); a bare ray has none");
  return RL_OK;
}

int rl_rtiow_hit_rays_device(const rl_scene *scene, const void *d_rays, uint64_t n, double tmin, double tmax, void *d_out, void *hip_stream,
                             rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, d_rays && d_out, st, done);
  if (done) return rc;
  if ((rc = rtiow_hit_rays_rules(scene, tmin, tmax)) != RL_OK) return rc;
  return rtiow_hit_rays_impl(scene, d_rays, n, tmin, tmax, d_out, (hipStream_t)hip_stream, st != nullptr, st);
}

// which kernel served the most recent rl_rtiow_hit_rays* / rl_rtiow_ray_color_rays* call of this process (1: reference order, 2: fast walk), and how many rays of
// the most recent SYNCHRONOUS one the fast walk re-traced in the reference's order (asynchronous calls: rl_render_status + rl_debug_slow_traces).
// The occlusion queries and the pixel renders report here too, under ids of their own: enum LastQuery above.
int rl_debug_last_query(unsigned long long *out2) {
  if (!out2) return set_err(RL_E_INVALID, "bad argument");
  out2[0] = (unsigned long long)g_last_query_kernel, out2[1] = g_last_query_retraced;
  return RL_OK;
}

int rl_rtc_intersect_rays_device(const rl_scene *scene, const void *d_rays, uint64_t n, uint32_t k, void *d_isects, void *d_counts, void *d_hit_index,
                                 void *hip_stream, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, d_rays && d_counts, st, done);
  if (done) return rc;
  if ((k != 0) != (d_isects != nullptr)) return set_err(RL_E_INVALID, "null buffer (out_isects goes with k > 0)");
  if (n * (uint64_t)(k ? k : 1) / (uint64_t)(k ? k : 1) != n) return set_err(RL_E_INVALID, "n * k overflows");
  hipStream_t stream = (hipStream_t)hip_stream;
  RtcFullParams F = rtc_query_params(scene);
  RayQuery Q{};
  Q.rays = (const rl_ray *)d_rays, Q.n = n, Q.k = k, Q.isects = (rl_rtc_isect *)d_isects, Q.counts = (uint32_t *)d_counts, Q.hit_index = (uint32_t *)d_hit_index;
  return query_run(scene, stream, st, [&]() -> int {
    hipLaunchKernelGGL((rtc_intersect_rays_kernel<QNT, 512>), dim3(query_grid(scene, (const void *)rtc_intersect_rays_kernel<QNT, 512>, n)), dim3(QNT), 0, stream, F, Q);
    return RL_OK;
  });
}

int rl_rtc_color_at_rays_device(const rl_scene *scene, const void *d_rays, uint64_t n, void *d_rgb, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, d_rays && d_rgb, st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  RtcFullParams F = rtc_query_params(scene);
  RayQuery Q{};
  Q.rays = (const rl_ray *)d_rays, Q.n = n, Q.rgb = (double *)d_rgb;
  return query_run(scene, stream, st, [&]() -> int {
    // the register budget rtc_full_kernel runs at (three waves per SIMD): the same per-ray body
    hipLaunchKernelGGL((rtc_color_at_rays_kernel<QNT, 768>), dim3(query_grid(scene, (const void *)rtc_color_at_rays_kernel<QNT, 768>, n)), dim3(QNT), 0, stream, F, Q);
    return RL_OK;
  });
}

int rl_rtiow_hit_rays(const rl_scene *scene, const rl_ray *rays, uint64_t n, double tmin, double tmax, rl_rtiow_hit *out, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, rays && out, st, done);
  if (done) return rc;
  if ((rc = rtiow_hit_rays_rules(scene, tmin, tmax)) != RL_OK) return rc;
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_out = q.out(out, n * sizeof(rl_rtiow_hit));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast kernel where it applies); rays and flagged are still collected
  return q.finish(rtiow_hit_rays_impl(scene, d_rays, n, tmin, tmax, d_out, q.stream, st != nullptr, &local), st, local);
}

int rl_rtc_intersect_rays(const rl_scene *scene, const rl_ray *rays, uint64_t n, uint32_t k, rl_rtc_isect *out_isects, uint32_t *out_counts,
                          uint32_t *out_hit_index, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, rays && out_counts, st, done);
  if (done) return rc;
  if ((k != 0) != (out_isects != nullptr)) return set_err(RL_E_INVALID, "null buffer (out_isects goes with k > 0)");
  if (k && n > ((uint64_t)1 << 44) / k) return set_err(RL_E_INVALID, "n * k too large");
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray));
  void *d_isects = q.inout(out_isects, (size_t)n * k * sizeof(rl_rtc_isect));  // uploaded: entries beyond a ray's count stay the caller's
  void *d_counts = q.out(out_counts, n * 4), *d_hit_index = q.out(out_hit_index, n * 4);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_intersect_rays_device(scene, d_rays, n, k, d_isects, d_counts, d_hit_index, q.stream, &local), st, local);
}

int rl_rtc_color_at_rays(const rl_scene *scene, const rl_ray *rays, uint64_t n, double *out_rgb, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, rays && out_rgb, st, done);
  if (done) return rc;
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_rgb = q.out(out_rgb, n * 24);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_color_at_rays_device(scene, d_rays, n, d_rgb, q.stream, &local), st, local);
}

// ---- seeded path queries (include/rl_render.h): Camera::get_ray and Camera::ray_color for ray buffers
static uint64_t g_query_pass_cap = 0;  // rl_debug_set_query_pass_cap: rays per pass of rl_rtiow_ray_color_rays* (0: what the work counter allows)
void rl_debug_set_query_pass_cap(unsigned long long rays) { g_query_pass_cap = rays; }

static int cursors_check(const rl_rng_cursor *cursors, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (cursors[i].word_pos >= (uint64_t)1 << 31) return set_err(RL_E_INVALID, "cursor word_pos >= 2^31 (the kernels keep the position in 32 bits)");
  return RL_OK;
}

// The kernel families of rtiow_render_indep_launch without the LDS sphere kernels: the counter-free general fast kernel wherever the
// scene has a world-space SAH tree (sphere-only scenes: the queries' own, HostRtiow::qfg), the reference-order wave-scheduled kernel for
// counting calls, scenes without one and RL_FAST=0.  sync_st as in rtiow_hit_rays_impl.
static int rtiow_ray_color_impl(const rl_scene *scene, const void *d_rays, const void *d_cursors, uint64_t n, uint64_t seed, uint32_t max_depth,
                                const double background[3], void *d_rgb, void *d_out_cursors, void *d_counts, hipStream_t stream, bool counting,
                                rl_stats *sync_st) {
  const RtiowProgram &rt = scene->rt();
  const FastGeneral &QF = scene->hrt->query_tree();
  rl_rtiow_camera qcam{};  // what a render takes from its camera and a query from the call
  qcam.image_width = 8, qcam.image_height = 8, qcam.samples_per_pixel = 1, qcam.max_depth = max_depth, qcam.seed = seed;
  qcam.background[0] = background[0], qcam.background[1] = background[1], qcam.background[2] = background[2];
  RtiowParams P;
  uint64_t unused_slots = 0;
  {
    int rcp = fill_rtiow_params(scene, &qcam, 0, 0, 1, 8, nullptr, false, P, unused_slots);
    if (rcp != RL_OK) return rcp;
  }
  query_tree_params(QF, P);
  P.q_rays = (const rl_ray *)d_rays, P.q_cursors = (const rl_rng_cursor *)d_cursors, P.q_rgb = (double *)d_rgb;
  P.q_out_cursors = (rl_rng_cursor *)d_out_cursors, P.q_ray_counts = (uint32_t *)d_counts;
  const bool fast = !counting && QF.ok && g_sw.fast_traversal;
  const bool trans = rt.has_noise || rt.has_sphere_uv;
  ValueKernel kern = nullptr;       // reference order: parameter block by value
  PointerKernel kern_ptr = nullptr;  // fast: by pointer, each pass its own stream-ordered copy
  int nt = 512;
  size_t lds = 0;
  if (fast) {  // never the one-wave-per-SIMD form: the rays flavour has none
    const bool media = QF.stage_roots.size() > 1;
    const FastgLayout lay = fastg_prepare(QF, trans, media, false, P);
    kern_ptr = fast_general_kernel(Mode::RAYS, trans, media, false), nt = lay.nt, lds = lay.lds;
  } else {
    kern = wave_general_kernel(Mode::RAYS, trans, counting, rt.has_media), lds = wave_general_lds(rt.has_media);
  }
  auto launch_pass = [&]() -> int {
    return kern_ptr ? launch_persistent(kern_ptr, nt, lds, P.n_slots, P, scene, stream) : launch_persistent(kern, nt, lds, P.n_slots, P, scene, stream);
  };
  // rays per pass: below the u32 work counter's end, with room for every resident lane's last claim (which overshoots)
  uint64_t per_pass = 0xFF000000ull;
  if (g_query_pass_cap && g_query_pass_cap < per_pass) per_pass = g_query_pass_cap;
  auto passes = [&]() -> int {
    for (uint64_t b = 0; b < n; b += per_pass) {
      P.q_first = b, P.n_slots = (uint32_t)std::min<uint64_t>(per_pass, n - b);
      if (b != 0) HIP_TRY(hipMemsetAsync(scene->d_scratch, 0, 4, stream));  // work counter only; stats keep accumulating
      int rcl = launch_pass();
      if (rcl != RL_OK) return rcl;
    }
    g_last_query_kernel = fast ? LAST_QUERY_FAST : LAST_QUERY_REFERENCE;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, passes, true);
}

int rl_rtiow_ray_color_rays_device(const rl_scene *scene, const void *d_rays, const void *d_cursors, uint64_t n, uint64_t seed, uint32_t max_depth,
                                   const double background[3], void *d_out_rgb, void *d_opt_out_cursors, void *d_opt_out_ray_counts, void *hip_stream,
                                   rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, d_rays && d_cursors && d_out_rgb && background, st, done);
  if (done) return rc;
  return rtiow_ray_color_impl(scene, d_rays, d_cursors, n, seed, max_depth, background, d_out_rgb, d_opt_out_cursors, d_opt_out_ray_counts,
                              (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_ray_color_rays(const rl_scene *scene, const rl_ray *rays, const rl_rng_cursor *cursors, uint64_t n, uint64_t seed, uint32_t max_depth,
                            const double background[3], double *out_rgb, rl_rng_cursor *opt_out_cursors, uint32_t *opt_out_ray_counts, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, rays && cursors && out_rgb && background, st, done);
  if (done) return rc;
  if ((rc = cursors_check(cursors, n)) != RL_OK) return rc;
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_cursors = q.in(cursors, n * sizeof(rl_rng_cursor)), *d_rgb = q.out(out_rgb, n * 24);
  void *d_out_cursors = q.back(opt_out_cursors, d_cursors, n * sizeof(rl_rng_cursor));  // the staged copy: the caller's cursors are never written
  void *d_counts = q.out(opt_out_ray_counts, n * 4);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the fast kernel where it applies); rays and flagged are still collected
  return q.finish(rtiow_ray_color_impl(scene, d_rays, d_cursors, n, seed, max_depth, background, d_rgb, d_out_cursors, d_counts, q.stream, st != nullptr, &local),
                  st, local);
}

static int camera_rays_launch(const rl_rtiow_camera *cam, uint64_t n, const void *d_px, const void *d_py, const void *d_cursors, void *d_rays,
                              void *d_out_cursors, hipStream_t stream) {
  CameraRaysQuery Q{};
  Q.cam = *cam;
  chacha_key_from_seed(cam->seed, Q.key);
  Q.px = (const uint32_t *)d_px, Q.py = (const uint32_t *)d_py, Q.cursors = (const rl_rng_cursor *)d_cursors;
  Q.rays = (rl_ray *)d_rays, Q.out_cursors = (rl_rng_cursor *)d_out_cursors, Q.n = n;
  const uint64_t want = (n + QNT - 1) / QNT, cap = (uint64_t)std::max(1, g_cus) * 8u;
  hipLaunchKernelGGL((rtiow_camera_rays_kernel<QNT>), dim3((uint32_t)std::min(want, cap)), dim3(QNT), 0, stream, Q);
  HIP_TRY(hipGetLastError());
  return RL_OK;
}

// (no scene and no stats: the camera is the call's subject, and a missing one is refused for the empty batch too)
int rl_rtiow_camera_rays_device(const rl_rtiow_camera *cam, uint64_t n, const void *d_px, const void *d_py, const void *d_cursors, void *d_out_rays,
                                void *d_out_cursors, void *hip_stream) {
  bool done;
  int rc = query_check(cam, 0, n, d_px && d_py && d_cursors && d_out_rays && d_out_cursors, nullptr, done);
  if (done) return rc;
  return camera_rays_launch(cam, n, d_px, d_py, d_cursors, d_out_rays, d_out_cursors, (hipStream_t)hip_stream);
}

int rl_rtiow_camera_rays(const rl_rtiow_camera *cam, uint64_t n, const uint32_t *px, const uint32_t *py, const rl_rng_cursor *cursors, rl_ray *out_rays,
                         rl_rng_cursor *out_cursors) {
  bool done;
  int rc = query_check(cam, 0, n, px && py && cursors && out_rays && out_cursors, nullptr, done);
  if (done) return rc;
  for (uint64_t i = 0; i < n; i++)
    if (px[i] >= cam->image_width || py[i] >= cam->image_height) return set_err(RL_E_INVALID, "pixel outside the image");
  if ((rc = cursors_check(cursors, n)) != RL_OK) return rc;
  HostStaging q(nullptr);
  unsigned char *d_xy = (unsigned char *)q.in({{px, n * 4}, {py, n * 4}});
  void *d_cursors = q.in(cursors, n * sizeof(rl_rng_cursor)), *d_rays = q.out(out_rays, n * sizeof(rl_ray));
  q.back(out_cursors, d_cursors, n * sizeof(rl_rng_cursor));
  if (q.rc != RL_OK) return q.rc;
  if ((rc = camera_rays_launch(cam, n, d_xy, d_xy + n * 4, d_cursors, d_rays, d_cursors, q.stream)) != RL_OK) return rc;
  HIP_TRY(hipStreamSynchronize(q.stream));
  return q.finish(RL_OK);
}

// ---- seeded hit queries (include/rl_render.h): Hittable::hit for rays that carry an RNG cursor, media scenes included
// A scene without media draws nothing: the bare-ray kernels serve it (rtiow_hit_rays_impl: fast / reference-order selection,
// rl_debug_last_query) and the cursors pass through.  A scene with media: the reference-order fold with MEDIA = true, counting or not.
// sync_st as in rtiow_hit_rays_impl.
static int rtiow_hit_rays_seeded_impl(const rl_scene *scene, const void *d_rays, const void *d_cursors, uint64_t n, uint64_t seed, double tmin, double tmax,
                                      void *d_out, void *d_out_cursors, hipStream_t stream, bool counting, rl_stats *sync_st) {
  if (!scene->rt().has_media)
    return rtiow_hit_rays_impl(scene, d_rays, n, tmin, tmax, d_out, stream, counting, sync_st, d_cursors, d_out_cursors != d_cursors ? d_out_cursors : nullptr);
  RtiowParams P = hit_query_params(scene);
  chacha_key_from_seed(seed, P.key);
  SeededHitQuery Q{};
  Q.rays = (const rl_ray *)d_rays, Q.cursors = (const rl_rng_cursor *)d_cursors, Q.n = n, Q.tmin = tmin, Q.tmax = tmax;
  Q.hits = (rl_rtiow_hit *)d_out, Q.out_cursors = (rl_rng_cursor *)d_out_cursors;
  auto launch = [&]() -> int {
    if (counting)
      hipLaunchKernelGGL((rtiow_hit_rays_seeded_kernel<QNT, true>), dim3(query_grid(scene, (const void *)rtiow_hit_rays_seeded_kernel<QNT, true>, n)), dim3(QNT), 0,
                         stream, P, Q);
    else
      hipLaunchKernelGGL((rtiow_hit_rays_seeded_kernel<QNT, false>), dim3(query_grid(scene, (const void *)rtiow_hit_rays_seeded_kernel<QNT, false>, n)), dim3(QNT), 0,
                         stream, P, Q);
    g_last_query_kernel = LAST_QUERY_REFERENCE, g_last_query_retraced = 0;  // (no fast walk, nothing re-traced: nothing to read back after the call)
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch);
}

// what rl_rtiow_hit_rays_seeded* adds to query_check; cursors: the host form's (null: the device form, where word_pos >= 2^31 is undefined)
static int rtiow_hit_rays_seeded_rules(double tmin, double tmax, const rl_rng_cursor *cursors, uint64_t n) {
  if (std::isnan(tmin) || std::isnan(tmax)) return set_err(RL_E_INVALID, "NaN interval bound");
  return cursors ? cursors_check(cursors, n) : RL_OK;
}

int rl_rtiow_hit_rays_seeded_device(const rl_scene *scene, const void *d_rays, const void *d_cursors, uint64_t n, uint64_t seed, double tmin, double tmax,
                                    void *d_out_hits, void *d_opt_out_cursors, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, d_rays && d_cursors && d_out_hits, st, done);
  if (done) return rc;
  if ((rc = rtiow_hit_rays_seeded_rules(tmin, tmax, nullptr, n)) != RL_OK) return rc;
  return rtiow_hit_rays_seeded_impl(scene, d_rays, d_cursors, n, seed, tmin, tmax, d_out_hits, d_opt_out_cursors, (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_hit_rays_seeded(const rl_scene *scene, const rl_ray *rays, const rl_rng_cursor *cursors, uint64_t n, uint64_t seed, double tmin, double tmax,
                             rl_rtiow_hit *out_hits, rl_rng_cursor *opt_out_cursors, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, rays && cursors && out_hits, st, done);
  if (done) return rc;
  if ((rc = rtiow_hit_rays_seeded_rules(tmin, tmax, cursors, n)) != RL_OK) return rc;
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_cursors = q.in(cursors, n * sizeof(rl_rng_cursor)), *d_out = q.out(out_hits, n * sizeof(rl_rtiow_hit));
  void *d_out_cursors = q.back(opt_out_cursors, d_cursors, n * sizeof(rl_rng_cursor));  // the staged copy: the caller's cursors are never written
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free; rays, words and flagged are still collected
  return q.finish(rtiow_hit_rays_seeded_impl(scene, d_rays, d_cursors, n, seed, tmin, tmax, d_out, d_out_cursors, q.stream, st != nullptr, &local), st, local);
}

// ---- material queries (include/rl_render.h): Material::scatter / emitted and Texture::value for buffers
static void material_query_params(const rl_scene *scene, uint64_t n, RtiowParams &P, MaterialQuery &Q, uint32_t &blocks) {
  const RtiowProgram &rt = scene->rt();
  P = RtiowParams{};
  P.materials = scene->d_materials, P.textures = scene->d_textures, P.images = scene->d_images, P.image_pool = scene->d_image_pool;
  P.perlins = scene->d_perlins;
  P.stats = (unsigned long long *)(scene->d_scratch + 64);
  Q = MaterialQuery{};
  Q.n = n, Q.n_materials = (uint32_t)rt.materials.size(), Q.n_textures = (uint32_t)rt.textures.size();
  const uint64_t want = (n + MATERIAL_QUERY_NT - 1) / MATERIAL_QUERY_NT, cap = (uint64_t)std::max(1, g_cus) * MATERIAL_QUERY_MAX_BLOCKS_PER_CU;
  blocks = (uint32_t)std::min(want, cap);
}

// the most lanes one material-query launch has on the current device: a larger batch puts several elements through one lane
unsigned long long rl_debug_material_query_lanes(void) {
  return (unsigned long long)std::max(1, g_cus) * MATERIAL_QUERY_MAX_BLOCKS_PER_CU * MATERIAL_QUERY_NT;
}

// sync_st: filled synchronously (the host form, and the device form with opt_stats); null: asynchronous, status ring
static int rtiow_scatter_impl(const rl_scene *scene, const void *d_rays, const void *d_hits, const void *d_cursors, uint64_t n, uint64_t seed, void *d_out,
                              void *d_out_cursors, hipStream_t stream, rl_stats *sync_st) {
  RtiowParams P;
  MaterialQuery Q;
  uint32_t blocks = 0;
  material_query_params(scene, n, P, Q, blocks);
  chacha_key_from_seed(seed, P.key);
  Q.rays = (const rl_ray *)d_rays, Q.hits = (const rl_rtiow_hit *)d_hits, Q.cursors = (const rl_rng_cursor *)d_cursors;
  Q.out = (rl_rtiow_scatter *)d_out, Q.out_cursors = (rl_rng_cursor *)d_out_cursors;
  return query_run(scene, stream, sync_st, [&]() -> int {
    hipLaunchKernelGGL((rtiow_scatter_rays_kernel<MATERIAL_QUERY_NT>), dim3(blocks), dim3(MATERIAL_QUERY_NT), 0, stream, P, Q);
    return RL_OK;
  });
}

int rl_rtiow_scatter_rays_device(const rl_scene *scene, const void *d_rays, const void *d_hits, const void *d_cursors, uint64_t n, uint64_t seed,
                                 void *d_out, void *d_opt_out_cursors, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, d_rays && d_hits && d_cursors && d_out, st, done);
  if (done) return rc;
  return rtiow_scatter_impl(scene, d_rays, d_hits, d_cursors, n, seed, d_out, d_opt_out_cursors, (hipStream_t)hip_stream, st);
}

int rl_rtiow_scatter_rays(const rl_scene *scene, const rl_ray *rays, const rl_rtiow_hit *hits, const rl_rng_cursor *cursors, uint64_t n, uint64_t seed,
                          rl_rtiow_scatter *out, rl_rng_cursor *opt_out_cursors, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, rays && hits && cursors && out, st, done);
  if (done) return rc;
  if ((rc = cursors_check(cursors, n)) != RL_OK) return rc;
  const uint32_t n_materials = (uint32_t)scene->rt().materials.size();
  for (uint64_t i = 0; i < n; i++)
    if (hits[i].hit != 0u && hits[i].material >= n_materials) return set_err(RL_E_INVALID, "hit record's material index outside the scene's table");
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_hits = q.in(hits, n * sizeof(rl_rtiow_hit)), *d_cursors = q.in(cursors, n * sizeof(rl_rng_cursor));
  void *d_out = q.out(out, n * sizeof(rl_rtiow_scatter));
  void *d_out_cursors = q.back(opt_out_cursors, d_cursors, n * sizeof(rl_rng_cursor));  // the staged copy: the caller's cursors are never written
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rtiow_scatter_impl(scene, d_rays, d_hits, d_cursors, n, seed, d_out, d_out_cursors, q.stream, &local), st, local);
}

static int rtiow_texture_values_impl(const rl_scene *scene, const void *d_textures, const void *d_uv, const void *d_p, uint64_t n, void *d_out,
                                     hipStream_t stream, rl_stats *sync_st) {
  RtiowParams P;
  MaterialQuery Q;
  uint32_t blocks = 0;
  material_query_params(scene, n, P, Q, blocks);
  Q.tex_ids = (const uint32_t *)d_textures, Q.uv = (const double *)d_uv, Q.p = (const double *)d_p, Q.rgb = (double *)d_out;
  return query_run(scene, stream, sync_st, [&]() -> int {
    hipLaunchKernelGGL((rtiow_texture_values_kernel<MATERIAL_QUERY_NT>), dim3(blocks), dim3(MATERIAL_QUERY_NT), 0, stream, P, Q);
    return RL_OK;
  });
}

int rl_rtiow_texture_values_device(const rl_scene *scene, const void *d_textures, const void *d_uv, const void *d_p, uint64_t n, void *d_out_rgb,
                                   void *hip_stream) {
  bool done;
  int rc = query_check(scene, 1, n, d_textures && d_uv && d_p && d_out_rgb, nullptr, done);
  if (done) return rc;
  return rtiow_texture_values_impl(scene, d_textures, d_uv, d_p, n, d_out_rgb, (hipStream_t)hip_stream, nullptr);
}

int rl_rtiow_texture_values(const rl_scene *scene, const uint32_t *textures, const double *uv, const double *p, uint64_t n, double *out_rgb) {
  bool done;
  int rc = query_check(scene, 1, n, textures && uv && p && out_rgb, nullptr, done);
  if (done) return rc;
  const uint32_t n_textures = (uint32_t)scene->rt().textures.size();
  for (uint64_t i = 0; i < n; i++)
    if (textures[i] >= n_textures) return set_err(RL_E_INVALID, "texture id outside the scene's table");
  HostStaging q(scene);
  void *d_textures = q.in(textures, n * 4), *d_uv = q.in(uv, n * 16), *d_p = q.in(p, n * 24), *d_rgb = q.out(out_rgb, n * 24);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // (waits for the kernel; the call has no opt_stats and copies back on RL_OK only)
  return q.finish(rtiow_texture_values_impl(scene, d_textures, d_uv, d_p, n, d_rgb, q.stream, &local));
}

// ---- RTC shading queries (include/rl_render.h): prepare_computations, shade_hit, shadow_attenuation, lighting for buffers
// the host forms' rule for comps[i].material (the device forms give such an element zeros)
static int rtc_comps_check(const rl_scene *scene, const rl_rtc_comps *comps, uint64_t n) {
  const uint32_t n_materials = (uint32_t)scene->rc().materials.size();
  for (uint64_t i = 0; i < n; i++)
    if (comps[i].hit != 0u && comps[i].material >= n_materials) return set_err(RL_E_INVALID, "comps record's material index outside the scene's table");
  return RL_OK;
}

static RtcShadeQuery rtc_shade_query(const rl_scene *scene, uint64_t n) {
  RtcShadeQuery Q{};
  Q.n = n, Q.n_materials = (uint32_t)scene->rc().materials.size();
  return Q;
}

int rl_rtc_prepare_rays_device(const rl_scene *scene, const void *d_rays, uint64_t n, void *d_out_comps, void *hip_stream, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, d_rays && d_out_comps, st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  RtcFullParams F = rtc_query_params(scene);
  RtcShadeQuery Q = rtc_shade_query(scene, n);
  Q.rays = (const rl_ray *)d_rays, Q.out_comps = (rl_rtc_comps *)d_out_comps;
  return query_run(scene, stream, st, [&]() -> int {
    hipLaunchKernelGGL((rtc_prepare_rays_kernel<QNT, 512>), dim3(query_grid(scene, (const void *)rtc_prepare_rays_kernel<QNT, 512>, n)), dim3(QNT), 0, stream, F, Q);
    return RL_OK;
  });
}

int rl_rtc_shade_hits_device(const rl_scene *scene, const void *d_comps, uint64_t n, void *d_out, void *d_opt_out_shadow, void *hip_stream,
                             rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, d_comps && d_out, st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  RtcFullParams F = rtc_query_params(scene);
  RtcShadeQuery Q = rtc_shade_query(scene, n);
  Q.comps = (const rl_rtc_comps *)d_comps, Q.out = (rl_rtc_shade *)d_out, Q.out_shadow = (double *)d_opt_out_shadow;
  return query_run(scene, stream, st, [&]() -> int {
    hipLaunchKernelGGL((rtc_shade_hits_kernel<QNT, 512>), dim3(query_grid(scene, (const void *)rtc_shade_hits_kernel<QNT, 512>, n)), dim3(QNT), 0, stream, F, Q);
    return RL_OK;
  });
}

int rl_rtc_shadow_attenuation_device(const rl_scene *scene, const void *d_points, const void *d_light_positions, uint64_t n, void *d_out_att,
                                     void *hip_stream, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, d_points && d_light_positions && d_out_att, st, done);
  if (done) return rc;
  hipStream_t stream = (hipStream_t)hip_stream;
  RtcFullParams F = rtc_query_params(scene);
  RtcShadeQuery Q = rtc_shade_query(scene, n);
  Q.points = (const double *)d_points, Q.light_pos = (const double *)d_light_positions, Q.out_att = (double *)d_out_att;
  return query_run(scene, stream, st, [&]() -> int {
    hipLaunchKernelGGL((rtc_shadow_attenuation_kernel<QNT, 512>), dim3(query_grid(scene, (const void *)rtc_shadow_attenuation_kernel<QNT, 512>, n)), dim3(QNT), 0,
                       stream, F, Q);
    return RL_OK;
  });
}

// sync_st: the host form waits for the kernel through it; null: asynchronous, status ring
static int rtc_lighting_impl(const rl_scene *scene, const void *d_comps, const void *d_light_positions, const void *d_light_intensities,
                             const void *d_shadow_att, uint64_t n, void *d_out_rgb, hipStream_t stream, rl_stats *sync_st) {
  RtcShadeQuery Q = rtc_shade_query(scene, n);
  Q.comps = (const rl_rtc_comps *)d_comps, Q.light_pos = (const double *)d_light_positions, Q.light_int = (const double *)d_light_intensities;
  Q.shadow_att = (const double *)d_shadow_att, Q.out_rgb = (double *)d_out_rgb;
  const rl_rtc_material *materials = scene->d_rmaterials;
  return query_run(scene, stream, sync_st, [&]() -> int {
    hipLaunchKernelGGL((rtc_lighting_kernel<QNT>), dim3(query_grid(scene, (const void *)rtc_lighting_kernel<QNT>, n)), dim3(QNT), 0, stream, materials, Q);
    return RL_OK;
  });
}

int rl_rtc_lighting_device(const rl_scene *scene, const void *d_comps, const void *d_light_positions, const void *d_light_intensities,
                           const void *d_shadow_att, uint64_t n, void *d_out_rgb, void *hip_stream) {
  bool done;
  int rc = query_check(scene, 2, n, d_comps && d_light_positions && d_light_intensities && d_shadow_att && d_out_rgb, nullptr, done);
  if (done) return rc;
  return rtc_lighting_impl(scene, d_comps, d_light_positions, d_light_intensities, d_shadow_att, n, d_out_rgb, (hipStream_t)hip_stream, nullptr);
}

int rl_rtc_prepare_rays(const rl_scene *scene, const rl_ray *rays, uint64_t n, rl_rtc_comps *out_comps, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, rays && out_comps, st, done);
  if (done) return rc;
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_comps = q.out(out_comps, n * sizeof(rl_rtc_comps));
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_prepare_rays_device(scene, d_rays, n, d_comps, q.stream, &local), st, local);
}

int rl_rtc_shade_hits(const rl_scene *scene, const rl_rtc_comps *comps, uint64_t n, rl_rtc_shade *out, double *opt_out_shadow, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, comps && out, st, done);
  if (done) return rc;
  if ((rc = rtc_comps_check(scene, comps, n)) != RL_OK) return rc;
  HostStaging q(scene);
  void *d_comps = q.in(comps, n * sizeof(rl_rtc_comps)), *d_out = q.out(out, n * sizeof(rl_rtc_shade));
  void *d_shadow = q.out(opt_out_shadow, (size_t)n * scene->rc().lights.size() * sizeof(double));  // [n][the scene's lights]
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_shade_hits_device(scene, d_comps, n, d_out, d_shadow, q.stream, &local), st, local);
}

int rl_rtc_shadow_attenuation(const rl_scene *scene, const double *points, const double *light_positions, uint64_t n, double *out_att,
                              rl_stats *st) {
  bool done;
  int rc = query_check(scene, 2, n, points && light_positions && out_att, st, done);
  if (done) return rc;
  HostStaging q(scene);
  void *d_points = q.in(points, n * 24), *d_light_positions = q.in(light_positions, n * 24), *d_att = q.out(out_att, n * 8);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;
  return q.finish(rl_rtc_shadow_attenuation_device(scene, d_points, d_light_positions, n, d_att, q.stream, &local), st, local);
}

int rl_rtc_lighting(const rl_scene *scene, const rl_rtc_comps *comps, const double *light_positions, const double *light_intensities,
                    const double *shadow_att, uint64_t n, double *out_rgb) {
  bool done;
  int rc = query_check(scene, 2, n, comps && light_positions && light_intensities && shadow_att && out_rgb, nullptr, done);
  if (done) return rc;
  if ((rc = rtc_comps_check(scene, comps, n)) != RL_OK) return rc;
  HostStaging q(scene);
  void *d_comps = q.in(comps, n * sizeof(rl_rtc_comps)), *d_rgb = q.out(out_rgb, n * 24);
  // one allocation for the three light inputs: positions, intensities, attenuations
  unsigned char *d_in = (unsigned char *)q.in({{light_positions, n * 24}, {light_intensities, n * 24}, {shadow_att, n * 8}});
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // (waits for the kernel; the call has no opt_stats and copies back on RL_OK only)
  return q.finish(rtc_lighting_impl(scene, d_comps, d_in, d_in + n * 24, d_in + n * 48, n, d_rgb, q.stream, &local));
}

}  // extern "C"
