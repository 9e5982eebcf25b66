// The host side of the NEE path renders (include/rl_render.h "NEE path renders", rl_rtiow_render_nee*; kernel:
// rl_rtiow_nee.h).  Not a translation unit of its own: rl_render.hip includes it once, as its last line (so the kernel is instantiated
// behind every other one).  The four entry forms, the launch and the launch geometry are rl_pixel_render_api.h's; here: what is
// particular to the family, with rl_direct_api.h's direct_ok, direct_rules and DirectArgs.
// The renders with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance sampling",
// rl_rtiow_render_nee_mis*) are the same four with a heuristic: both families go through nee_family and nee_run, which
// take the flavour as `mis`.
// The renders with sphere lights (include/rl_render.h "NEE path renders with sphere lights", rl_rtiow_render_nee_mis_spheres*; DESIGN.md
// §3.25) are the MIS four with a second light array; with no sphere in it a call is the MIS call, launch and all.
#pragma once

namespace {
// `mis` of everything below: -1 the plain NEE renders, else the heuristic of the renders with multiple importance sampling
constexpr int NEE_PLAIN = -1;

// The nine instantiations: {plain, MIS, MIS with sphere lights} x {counting, counter-free reference order, counter-free fast walks}
template <bool MIS, bool SPH = false>
auto nee_kernel(bool counting, bool fast) -> void (*)(RtiowParams, NeeQueryOf<MIS, SPH>) {
  if (fast) return rtiow_nee_kernel<FEATURES_NT, false, true, FEATURES_SD, MIS, SPH>;
  return counting ? rtiow_nee_kernel<FEATURES_NT, true, false, FEATURES_SD, MIS, SPH> : rtiow_nee_kernel<FEATURES_NT, false, false, FEATURES_SD, MIS, SPH>;
}

// what an entry point with sphere lights gives nee_ok beside DirectArgs (given = false: an entry point without them)
struct SphereArgs {
  bool given = false;
  uint32_t n = 0;
  const double *spheres = nullptr;  // [n][7]: C[3], r, E[3]
};

// What is particular to these calls and decided before a device is looked at: direct_ok's rules with the two outputs of these calls, and
// a path of at least one vertex.  On success `out` holds the lights as the kernel reads them: the quads, then the spheres.
// With sphere lights the two kinds share the slots and n_lights may be 0: the rules of the counts are stated for the total here, and the
// quads (if any) go through direct_ok for theirs.
bool nee_ok(int mis, const rl_rtiow_camera *cam, uint32_t n_lights, const double *lights, const SphereArgs &Sp, uint32_t light_samples, double seg_tmax,
            const void *sums, const void *sq, DirectLight *out) {
  if (cam && cam->max_depth == 0) return false;
  if (mis != NEE_PLAIN && mis != (int)RL_MIS_BALANCE && mis != (int)RL_MIS_POWER) return false;
  if (!Sp.given) return direct_ok(cam, n_lights, lights, light_samples, seg_tmax, sums, sq, nullptr, out);
  const uint64_t total = (uint64_t)n_lights + (uint64_t)Sp.n;
  if (mis == NEE_PLAIN || total == 0 || total > RL_DIRECT_MAX_LIGHTS || (n_lights && !lights) || (Sp.n && !Sp.spheres) || light_samples == 0) return false;
  if (!(seg_tmax > 1e-10) || !(seg_tmax <= 1.0) || (!sums && !sq)) return false;
  if (cam && (uint64_t)cam->samples_per_pixel * (total * (uint64_t)light_samples) >= ((uint64_t)1 << 32)) return false;  // S (L + Ls) K, as direct_ok
  if (n_lights && !direct_ok(cam, n_lights, lights, light_samples, seg_tmax, sums, sq, nullptr, out)) return false;
  for (uint32_t j = 0; j < Sp.n; j++) {
    const double *p = Sp.spheres + (size_t)j * 7;
    for (int i = 0; i < 7; i++)
      if (!std::isfinite(p[i])) return false;
    if (!(p[3] > 0.0)) return false;
    DirectLight &d = out[n_lights + j];
    d = DirectLight{};
    for (int i = 0; i < 3; i++) d.Q[i] = p[i], d.E[i] = p[4 + i];
    sphere_r(d) = p[3];
    sphere_A(d) = (4.0 * M_PI) * (p[3] * p[3]);
    if (!std::isfinite(sphere_A(d))) return false;
  }
  return true;
}

// (A.lights is filled here; the callable reads A when it runs, behind every check)
PixelFamily nee_family(int mis, const rl_rtiow_camera *cam, const double *lights, void *sums, void *sq, DirectArgs &A, SphereArgs Sp = {}) {
  return {nee_ok(mis, cam, A.n_lights, lights, Sp, A.light_samples, A.seg_tmax, sums, sq, A.lights), direct_rules,
          {{sums, 3 * sizeof(double)}, {sq, 3 * sizeof(double)}}};
}

template <bool MIS, bool SPH = false>
int nee_launch(const rl_scene *scene, const RtiowParams &P, const NeeQueryOf<MIS, SPH> &Q, const PixelTarget &T) {
  return pixel_render_launch(scene, P, Q, nee_kernel<MIS, SPH>(true, false), nee_kernel<MIS, SPH>(false, false), nee_kernel<MIS, SPH>(false, true),
                             SPH   ? LAST_QUERY_NEE_SPHERES_REFERENCE
                             : MIS ? LAST_QUERY_NEE_MIS_REFERENCE
                                   : LAST_QUERY_NEE_REFERENCE,
                             SPH   ? LAST_QUERY_NEE_SPHERES_FAST
                             : MIS ? LAST_QUERY_NEE_MIS_FAST
                                   : LAST_QUERY_NEE_FAST,
                             T);
}

// the family's query struct filled from the entry form's target, and the launch: the MIS flavour's is the plain one and the heuristic,
// the sphere flavour's is that and the number of spheres (none: the MIS flavour's own launch)
auto nee_run(int mis, const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const DirectArgs &A, SphereArgs Sp = {}) {
  return [=, &A](const PixelTarget &T) -> int {
    const uint32_t n_spheres = Sp.given ? Sp.n : 0u;
    NeeSpheresQuery M{};
    NeeQuery &Q = M;
    Q.n = T.n, Q.xs = (const uint32_t *)T.d_xs, Q.ys = (const uint32_t *)T.d_ys;
    Q.n_lights = A.n_lights, Q.light_samples = A.light_samples, Q.seg_tmax = A.seg_tmax;
    Q.kf = 1.0 / (M_PI * (double)A.light_samples);
    Q.sums = (double *)T.out[0], Q.sq = (double *)T.out[1];
    for (uint32_t l = 0; l < A.n_lights + n_spheres; l++) Q.lights[l] = A.lights[l];
    const RtiowParams P = pixel_render_params(scene, cam, first_sample, T, true);
    M.heuristic = (uint32_t)mis, M.n_sphere_lights = n_spheres;
    if (n_spheres) return nee_launch<true, true>(scene, P, M, T);
    return mis >= 0 ? nee_launch<true>(scene, P, M, T) : nee_launch<false>(scene, P, Q, T);
  };
}
}  // namespace

// a heuristic beyond the two is kept a value nee_ok refuses (never NEE_PLAIN)
static int mis_of(uint32_t heuristic) { return heuristic <= RL_MIS_POWER ? (int)heuristic : (int)RL_MIS_POWER + 1; }

extern "C" {

int rl_rtiow_render_nee_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                               const double *lights, uint32_t light_samples, double seg_tmax, void *d_sums, void *d_sq, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_rows_device(nee_family(NEE_PLAIN, cam, lights, d_sums, d_sq, A), scene, cam, row_first, row_step, hip_stream, st, nee_run(NEE_PLAIN, scene, cam, first_sample, A));
}
int rl_rtiow_render_nee_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                             const double *lights, uint32_t light_samples, double seg_tmax, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_rows_host(nee_family(NEE_PLAIN, cam, lights, sums, sq, A), scene, cam, row_first, row_step, st, nee_run(NEE_PLAIN, scene, cam, first_sample, A));
}
int rl_rtiow_render_pixels_nee_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                      uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, void *d_sums, void *d_sq, void *hip_stream,
                                      rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_list_device(nee_family(NEE_PLAIN, cam, lights, d_sums, d_sq, A), scene, cam, d_xs, d_ys, n, hip_stream, st, nee_run(NEE_PLAIN, scene, cam, first_sample, A));
}
int rl_rtiow_render_pixels_nee(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                               uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_list_host(nee_family(NEE_PLAIN, cam, lights, sums, sq, A), scene, cam, xs, ys, n, st, nee_run(NEE_PLAIN, scene, cam, first_sample, A));
}

// with multiple importance sampling (include/rl_render.h "NEE path renders with multiple importance sampling"): the same four with a heuristic
int rl_rtiow_render_nee_mis_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                   uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, void *d_sums, void *d_sq,
                                   void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_rows_device(nee_family(mis_of(heuristic), cam, lights, d_sums, d_sq, A), scene, cam, row_first, row_step, hip_stream, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A));
}
int rl_rtiow_render_nee_mis_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step, uint32_t n_lights,
                                 const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_rows_host(nee_family(mis_of(heuristic), cam, lights, sums, sq, A), scene, cam, row_first, row_step, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A));
}
int rl_rtiow_render_pixels_nee_mis_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys, uint64_t n,
                                          uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, void *d_sums,
                                          void *d_sq, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_list_device(nee_family(mis_of(heuristic), cam, lights, d_sums, d_sq, A), scene, cam, d_xs, d_ys, n, hip_stream, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A));
}
int rl_rtiow_render_pixels_nee_mis(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                   uint32_t n_lights, const double *lights, uint32_t light_samples, double seg_tmax, uint32_t heuristic, double *sums, double *sq,
                                   rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  return pixel_list_host(nee_family(mis_of(heuristic), cam, lights, sums, sq, A), scene, cam, xs, ys, n, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A));
}

// with sphere lights (include/rl_render.h "NEE path renders with sphere lights"): the MIS four with a second light array
int rl_rtiow_render_nee_mis_spheres_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                           uint32_t n_lights, const double *lights, uint32_t n_sphere_lights, const double *sphere_lights, uint32_t light_samples,
                                           double seg_tmax, uint32_t heuristic, void *d_sums, void *d_sq, void *hip_stream, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  const SphereArgs Sp{true, n_sphere_lights, sphere_lights};
  return pixel_rows_device(nee_family(mis_of(heuristic), cam, lights, d_sums, d_sq, A, Sp), scene, cam, row_first, row_step, hip_stream, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A, Sp));
}
int rl_rtiow_render_nee_mis_spheres_rows(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, uint32_t row_first, uint32_t row_step,
                                         uint32_t n_lights, const double *lights, uint32_t n_sphere_lights, const double *sphere_lights, uint32_t light_samples,
                                         double seg_tmax, uint32_t heuristic, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  const SphereArgs Sp{true, n_sphere_lights, sphere_lights};
  return pixel_rows_host(nee_family(mis_of(heuristic), cam, lights, sums, sq, A, Sp), scene, cam, row_first, row_step, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A, Sp));
}
int rl_rtiow_render_pixels_nee_mis_spheres_device(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const void *d_xs, const void *d_ys,
                                                  uint64_t n, uint32_t n_lights, const double *lights, uint32_t n_sphere_lights, const double *sphere_lights,
                                                  uint32_t light_samples, double seg_tmax, uint32_t heuristic, void *d_sums, void *d_sq, void *hip_stream,
                                                  rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  const SphereArgs Sp{true, n_sphere_lights, sphere_lights};
  return pixel_list_device(nee_family(mis_of(heuristic), cam, lights, d_sums, d_sq, A, Sp), scene, cam, d_xs, d_ys, n, hip_stream, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A, Sp));
}
int rl_rtiow_render_pixels_nee_mis_spheres(const rl_scene *scene, const rl_rtiow_camera *cam, uint64_t first_sample, const uint32_t *xs, const uint32_t *ys, uint64_t n,
                                           uint32_t n_lights, const double *lights, uint32_t n_sphere_lights, const double *sphere_lights, uint32_t light_samples,
                                           double seg_tmax, uint32_t heuristic, double *sums, double *sq, rl_stats *st) {
  DirectArgs A{n_lights, light_samples, seg_tmax, {}};
  const SphereArgs Sp{true, n_sphere_lights, sphere_lights};
  return pixel_list_host(nee_family(mis_of(heuristic), cam, lights, sums, sq, A, Sp), scene, cam, xs, ys, n, st, nee_run(mis_of(heuristic), scene, cam, first_sample, A, Sp));
}

}  // extern "C"
