// The host side of the occlusion queries (include/rl_render.h "RTIOW occlusion queries", rl_rtiow_occluded_rays*; kernels:
// rl_occlusion_query.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernels are
// instantiated behind every other one), and it uses rl_query_api.h's query_check, query_run, hit_query_params, query_tree_params,
// rtiow_hit_rays_rules and rl_debug_last_query ids beside the staging of rl_host_api.h.  Two entry points over one launch function; the
// routing between the two kernels is rtiow_hit_rays_impl's.
#pragma once

namespace {
constexpr int OCCLUSION_SD = 40;
}  // namespace

// counting: the caller wants the reference's counters (reference-order kernel).  Otherwise the any-hit walk serves the call where the
// scene has a fast tree and tmin is the interval its filters are derived for.  sync_st: filled synchronously (the host form; rays and
// flagged only when !counting); null: asynchronous, status ring.
static int rtiow_occluded_rays_impl(const rl_scene *scene, const void *d_rays, uint64_t n, double tmin, double tmax, void *d_out, hipStream_t stream,
                                    bool counting, rl_stats *sync_st) {
  const FastGeneral &QF = scene->hrt->query_tree();
  RtiowParams P = hit_query_params(scene);
  OcclusionQuery Q{};
  Q.rays = (const rl_ray *)d_rays, Q.n = n, Q.tmin = tmin, Q.tmax = tmax, Q.occluded = (uint8_t *)d_out;
  const bool fast = !counting && tmin == 1e-10 && QF.ok && QF.media.empty() && g_sw.fast_traversal;
  auto launch = [&]() -> int {
    if (fast) {
      constexpr int SD = OCCLUSION_SD;
      P.fg_nodes = scene->d_fg_nodes, P.fg_items = scene->d_fg_items, P.fg_spheres = scene->d_fg_spheres, P.fg_material = scene->d_fg_material;
      P.fg_seg_roots = scene->d_fg_seg_roots;
      query_tree_params(QF, P);
      // LDS and grid: those of the fast hit kernel (the per-lane stacks, and the tree's top in what is left)
      const size_t base = (size_t)QNT * SD * sizeof(uint32_t);
      const size_t room = g_lds_max > base ? (g_lds_max - base) / sizeof(FastNodeQ) : 0;
      P.fg_top = g_sw.fastg_top ? (uint32_t)std::min<size_t>(QF.top_nodes, room) : 0u;
      const size_t lds = base + (size_t)P.fg_top * sizeof(FastNodeQ);
      const void *kern = (const void *)rtiow_occluded_rays_fast_kernel<QNT, SD>;
      if (ensure_lds_attr(kern, lds) != 0) return set_err(RL_E_DEVICE, "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed");
      uint64_t want = (n + QNT - 1) / QNT, cap = (uint64_t)g_cus * (uint64_t)std::max<size_t>(1, std::min<size_t>(g_lds_max / lds, 2048 / QNT));
      hipLaunchKernelGGL((rtiow_occluded_rays_fast_kernel<QNT, SD>), dim3((uint32_t)std::min(want, cap)), dim3(QNT), lds, stream, P, Q);
    } else if (counting)
      hipLaunchKernelGGL((rtiow_occluded_rays_kernel<QNT, true>), dim3(query_grid(scene, (const void *)rtiow_occluded_rays_kernel<QNT, true>, n)), dim3(QNT), 0, stream,
                         P, Q);
    else
      hipLaunchKernelGGL((rtiow_occluded_rays_kernel<QNT, false>), dim3(query_grid(scene, (const void *)rtiow_occluded_rays_kernel<QNT, false>, n)), dim3(QNT), 0,
                         stream, P, Q);
    g_last_query_kernel = fast ? LAST_QUERY_OCCLUSION_FAST : LAST_QUERY_OCCLUSION_REFERENCE;
    if (!fast) g_last_query_retraced = 0;
    return RL_OK;
  };
  return query_run(scene, stream, sync_st, launch, fast);
}

extern "C" {

int rl_rtiow_occluded_rays_device(const rl_scene *scene, const void *d_rays, uint64_t n, double tmin, double tmax, void *d_out_occluded, void *hip_stream,
                                  rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, d_rays && d_out_occluded, st, done);
  if (done) return rc;
  if ((rc = rtiow_hit_rays_rules(scene, tmin, tmax)) != RL_OK) return rc;
  return rtiow_occluded_rays_impl(scene, d_rays, n, tmin, tmax, d_out_occluded, (hipStream_t)hip_stream, st != nullptr, st);
}

int rl_rtiow_occluded_rays(const rl_scene *scene, const rl_ray *rays, uint64_t n, double tmin, double tmax, uint8_t *out_occluded, rl_stats *st) {
  bool done;
  int rc = query_check(scene, 1, n, rays && out_occluded, st, done);
  if (done) return rc;
  if ((rc = rtiow_hit_rays_rules(scene, tmin, tmax)) != RL_OK) return rc;
  HostStaging q(scene);
  void *d_rays = q.in(rays, n * sizeof(rl_ray)), *d_out = q.out(out_occluded, n);
  if (q.rc != RL_OK) return q.rc;
  rl_stats local;  // without opt_stats the call is counter-free (the any-hit walk where it applies); rays and flagged are still collected
  return q.finish(rtiow_occluded_rays_impl(scene, d_rays, n, tmin, tmax, d_out, q.stream, st != nullptr, &local), st, local);
}

}  // extern "C"
